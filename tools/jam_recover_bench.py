"""The index past damage and the salvage of a .jam archive resident in HBM against the calls that stop at a bad frame (DESIGN 4.6,
"Damaged archives"):

  (a)  Context.jam_recover_index against Context.jam_index on UNDAMAGED archives: the same frame walk, no scan launch -- the ratio
       says what the recover entry costs an archive that did not need it
  (b)  the scan of one damaged archive -- one frame of 64 MiB whose header lost its magic, so the search runs over every byte of it --
       as GB/s of archive bytes, beside jpk_dev_checksum over the same bytes (a kernel that also reads every byte once): device time of
       both from the context's profile counters, and the wall clock of jam_scan (count, prefix scan, two synchronisations) and of the
       whole jam_recover_index of that archive.  Those 16 MB stay in the Infinity Cache from round to round, so the same pair is
       measured once more over 1 GiB of random bytes, which do not
  (c)  Context.jam_salvage through a plain index against Context.jam_decompress (which this change leaves as it was) on the same
       undamaged archives
  (d)  stock-CLI archives (kind 1), 64 frames of 1 MiB: Context.jam_recover_index(kind 1) against Context.jam_cli_index on the undamaged
       archive -- the same passes, no scan launch --, the recover of that archive with 1 and with 8 lost headers (one pass fewer frames,
       one search per lost header), and Context.jam_repair of the index with 1 lost header against a device-to-device copy of the bytes
       it writes

Workloads: corpus text as 64 frames of 1 MiB and as 4 frames of 64 MiB.  After one warm-up of each, the variants are timed in turn (every round starts one
variant further on), --reps rounds, and the medians reported; every call ends in a device synchronise.  It is one GPU step: run it under a time limit of
its own,

  timeout -k 10 900 python tools/jam_recover_bench.py [--reps 5] [--parts plain,cli] [--out profiles/jam_recover.txt]

--parts cli measures (d) alone; its lines are appended to the profile behind those of the other parts.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1 << 20
SHAPES = ((64, 1 * MiB), (4, 64 * MiB))


def workload(torch, jam, frames, bs):
    """frames x bs bytes on the device: tiles of 64 MiB of corpus text, a byte in 4099 changed per frame"""
    base = torch.from_numpy(np.concatenate([jam.corpus.make("text", MiB, 8000 + i) for i in range(64)])).to("cuda")
    d = base.repeat((frames * bs + len(base) - 1) // len(base))[: frames * bs].contiguous()
    d.view(frames, bs)[:, ::4099] ^= torch.arange(frames, dtype=torch.uint8, device="cuda")[:, None]
    return d


def timed(order, run, reps, sync):
    """the variants in turn, every round starting one variant further on, so that none always runs behind the same neighbour"""
    times = {k: [] for k in order}
    for r in range(reps):
        for k in order[r % len(order):] + order[: r % len(order)]:
            sync()
            t0 = time.perf_counter()
            run(k)
            sync()
            times[k].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) * 1e3 for k, v in times.items()}, times


def cli_part(torch, jam, ctx, reps, sync):
    """(d): the lines of the stock-CLI measurements"""
    frames, bs = 64, MiB
    n = frames * bs
    d_raw = workload(torch, jam, frames, bs)
    bound = jam.jam_cli_compress_bound(n, bs)
    d_arch = torch.empty(bound + 64, dtype=torch.uint8, device="cuda")
    alen = ctx.jam_cli_compress(d_raw, n, bs, d_arch, bound)
    ref = ctx.jam_cli_index(d_arch, alen)
    assert (ref.frames, ref.raw_len, ref.bad_frame) == (frames, n, -1)
    starts = [ref.frame(k)[2] - 15 for k in range(frames)]
    lost = {1: [31], 8: list(range(3, 64, 8))}
    d_lost = {}
    for m, ks in lost.items():
        d_lost[m] = d_arch[:alen].clone()
        for k in ks:
            d_lost[m][starts[k]] ^= 1
    ix1 = ctx.jam_recover_index(d_lost[1], alen, jam.JAM_INDEX_CLI)
    assert ix1.frames == frames - 1 and len(ix1.gaps) == 1
    keep = alen - ix1.gaps[0][1]
    d_fix, d_copy = torch.empty(alen + 64, dtype=torch.uint8, device="cuda"), torch.empty(alen + 64, dtype=torch.uint8, device="cuda")

    def run(k):
        if k == "cli_index":
            jx = ctx.jam_cli_index(d_arch, alen)
            assert (jx.frames, jx.raw_len, jx.bad_frame) == (frames, n, -1)
            jx.close()
        elif k == "recover":
            jx = ctx.jam_recover_index(d_arch, alen, jam.JAM_INDEX_CLI)
            assert (jx.frames, jx.raw_len, jx.gaps) == (frames, n, [])
            jx.close()
        elif k in ("lost1", "lost8"):
            m = int(k[4:])
            jx = ctx.jam_recover_index(d_lost[m], alen, jam.JAM_INDEX_CLI)
            assert (jx.frames, len(jx.gaps)) == (frames - m, m)
            jx.close()
        elif k == "repair":
            assert ctx.jam_repair(ix1, d_lost[1], alen, d_fix, alen) == (keep, frames - 1)
        else:
            d_copy[:keep].copy_(d_lost[1][:keep])

    ctx.profile_enable(2)
    for k in ("cli_index", "recover"):                      # warm-up: arenas, scratch, code objects
        run(k)
    sync()
    scans = [r for r in ctx.profile_table() if r["name"] == "k_jam_scan_*"]
    ctx.profile_enable(0)
    assert not scans, scans                                 # an undamaged archive launches no scan
    for k in ("lost1", "lost8", "repair", "copy"):
        run(k)
    sync()
    gap = ix1.gaps[0]
    want = torch.cat([d_lost[1][: gap[0]], d_lost[1][gap[0] + gap[1]: alen]])
    assert torch.equal(d_fix[:keep], want)
    med, times = timed(("cli_index", "recover"), run, reps, sync)
    for order in (("lost1", "lost8"), ("repair", "copy")):
        m2, t2 = timed(order, run, reps, sync)
        med.update(m2)
        times.update(t2)
    ratio = med["recover"] / med["cli_index"]
    return [
        f"-- (d) stock-CLI archive, {frames} frames of {bs // MiB} MiB: archive {alen} bytes, raw {n} bytes; median of {reps} alternating rounds after one warm-up",
        f"(d) jam_cli_index                                {med['cli_index']:9.2f} ms",
        f"(d) jam_recover_index, kind 1 (no gap, no scan)  {med['recover']:9.2f} ms   recover / cli_index = {ratio:.3f}",
        f"(d) jam_recover_index, kind 1, 1 lost header     {med['lost1']:9.2f} ms",
        f"(d) jam_recover_index, kind 1, 8 lost headers    {med['lost8']:9.2f} ms",
        f"(d) jam_repair, 63 kept frames, {keep} bytes  {med['repair']:9.3f} ms   ({keep / med['repair'] / 1e6:.1f} GB/s)",
        f"(d) device-to-device copy of {keep} bytes     {med['copy']:9.3f} ms   ({keep / med['copy'] / 1e6:.1f} GB/s)   repair / copy = {med['repair'] / med['copy']:.2f}",
        "all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.3f}" for t in times[k]) for k in times),
        f"kind-1 recover of an undamaged archive within 3 % of the index creator: {'yes' if abs(ratio - 1) <= 0.03 else 'NO'} (recover / cli_index = {ratio:.3f})",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="plain,cli", help="plain: (a)-(c) on plain archives; cli: (d) on a stock-CLI archive")
    a = ap.parse_args()
    parts = a.parts.split(",")

    import torch                                            # first: torch brings its own HIP runtime, and the library must share it
    import jampack_amd as jam
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    if "plain" not in parts:
        lines = cli_part(torch, jam, ctx, a.reps, sync)
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text)
        ctx.close()
        return
    lines = ["tools/jam_recover_bench.py: plain archives of corpus text in HBM",
             f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise"]
    answers = []
    for frames, bs in SHAPES:
        d_raw = workload(torch, jam, frames, bs)
        n = frames * bs
        bound = jam.jam_compress_bound(n, bs)
        d_arch = torch.empty(bound + 64, dtype=torch.uint8, device="cuda")
        alen = ctx.jam_compress(d_raw, n, bs, d_arch, bound)
        out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        ix = ctx.jam_index(d_arch, alen)
        assert (ix.frames, ix.raw_len, ix.bad_frame) == (frames, n, -1)

        def run(k):
            if k == "index":
                jx = ctx.jam_index(d_arch, alen)
                assert (jx.frames, jx.raw_len, jx.bad_frame) == (frames, n, -1)
                jx.close()
            elif k == "recover":
                jx = ctx.jam_recover_index(d_arch, alen)
                assert (jx.frames, jx.raw_len, jx.gaps) == (frames, n, [])
                jx.close()
            elif k == "decompress":
                assert ctx.jam_decompress(d_arch, alen, out, n) == (n, frames, -1)
            else:
                assert ctx.jam_salvage(ix, d_arch, alen, out, n) == (n, [0] * frames)

        order = ("index", "recover", "decompress", "salvage")
        ctx.profile_enable(2)
        for k in order:                                     # warm-up: arenas, scratch, code objects
            out.zero_()
            run(k)
            sync()
            if k in ("decompress", "salvage"):
                assert torch.equal(out[:n], d_raw), k
        scans = [r for r in ctx.profile_table() if r["name"] == "k_jam_scan_*"]
        ctx.profile_enable(0)
        assert not scans, scans                             # an undamaged archive launches no scan
        # (a) and (c) in groups of their own: an index call behind a whole decode would find the chunk headers cold, one behind the other
        # index call warm, and with two variants the rotation lets each lead every other round
        med, times = timed(order[:2], run, a.reps, sync)
        med_c, times_c = timed(order[2:], run, a.reps, sync)
        med.update(med_c)
        times.update(times_c)
        lines += [
            f"-- {frames} frames of {bs // MiB} MiB: archive {alen} bytes, raw {n} bytes",
            f"(a) jam_index                                   {med['index']:9.3f} ms",
            f"(a) jam_recover_index (no gap, no scan launch)  {med['recover']:9.3f} ms   recover / index = {med['recover'] / med['index']:.3f}",
            f"(c) jam_decompress, whole archive               {med['decompress']:9.2f} ms   ({n / med['decompress'] / 1e6:.3f} GB/s)",
            f"(c) jam_salvage through the plain index         {med['salvage']:9.2f} ms   ({n / med['salvage'] / 1e6:.3f} GB/s)   salvage / decompress = "
            f"{med['salvage'] / med['decompress']:.3f}",
            "all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.3f}" for t in times[k]) for k in order),
        ]
        answers.append((frames, bs, med["recover"] / med["index"], med["salvage"] / med["decompress"]))
        ix.close()
        if frames == 4:
            # (b) the first frame of this archive alone, its magic gone: no frame is left, the search reads every byte once
            h = d_arch[:15].cpu().numpy()
            one = 15 + int(np.frombuffer(h[7:11].tobytes(), dtype="<i4")[0])
            d_one = d_arch[:one].clone()
            d_one[1] ^= 1
            assert ctx.jam_scan(d_one, one, 0, one) == []           # text: no plausible header inside the payload

            def run_b(k):
                if k == "scan":
                    ctx.jam_scan(d_one, one, 0, one)
                elif k == "checksum":
                    ctx.checksum(d_one, one)
                else:
                    jx = ctx.jam_recover_index(d_one, one)
                    assert (jx.frames, jx.gaps) == (0, [(0, one, 0, 0)])
                    jx.close()

            order_b = ("scan", "checksum", "recover")
            for k in order_b:
                run_b(k)
            medb, timesb = timed(order_b, run_b, a.reps, sync)
            ctx.profile_enable(2)
            run_b("scan")
            run_b("checksum")
            sync()
            prof = {r["name"]: r for r in ctx.profile_table()}
            ctx.profile_enable(0)
            ks, kc = prof["k_jam_scan_*"], prof["k_chk_*"]
            gbs = lambda ms: one / ms / 1e6
            lines += [
                f"-- (b) one frame of 64 MiB with a damaged header: {one} archive bytes, scanned from the first to the last",
                f"k_jam_scan_count, device time of {ks['launches']} launch(es)     {ks['ms']:9.3f} ms   ({gbs(ks['ms']):.1f} GB/s)",
                f"k_chk_* (jpk_dev_checksum), device time of {kc['launches']} launch(es) {kc['ms']:7.3f} ms   ({gbs(kc['ms']):.1f} GB/s)   scan / checksum rate = "
                f"{kc['ms'] / ks['ms']:.2f}",
                f"jam_scan, wall clock (count, prefix scan, read-backs) {medb['scan']:9.3f} ms   ({gbs(medb['scan']):.1f} GB/s)",
                f"checksum, wall clock                                  {medb['checksum']:9.3f} ms   ({gbs(medb['checksum']):.1f} GB/s)",
                f"jam_recover_index of it (walk, one search, one gap)   {medb['recover']:9.3f} ms",
                "all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.3f}" for t in timesb[k]) for k in order_b),
            ]
            answers.append(("scan, 16 MB (cache-resident)", kc["ms"] / ks["ms"]))
            del d_one
        del d_arch, out, d_raw
    # (b) again where neither kernel can be fed from the 256 MiB Infinity Cache: 1 GiB of random bytes, one window (the largest the scan takes)
    big = 1 << 30
    d_big = torch.randint(0, 256, (big,), dtype=torch.uint8, device="cuda")
    for _ in range(2):                                      # the second round under the profiler
        ctx.profile_enable(2)
        hits = ctx.jam_scan(d_big, big, 0, big)
        ctx.checksum(d_big, big)
        sync()
        prof = {r["name"]: r for r in ctx.profile_table()}
        ctx.profile_enable(0)
    ks, kc = prof["k_jam_scan_*"], prof["k_chk_*"]
    lines += [
        f"-- (b) 1 GiB of random bytes, one window: {len(hits)} plausible header(s); device time of one call each after a warm-up",
        f"k_jam_scan_*, {ks['launches']} launch(es)               {ks['ms']:9.3f} ms   ({big / ks['ms'] / 1e6:.1f} GB/s)",
        f"k_chk_* (jpk_dev_checksum), {kc['launches']} launch(es) {kc['ms']:9.3f} ms   ({big / kc['ms'] / 1e6:.1f} GB/s)   scan / checksum rate = {kc['ms'] / ks['ms']:.2f}",
    ]
    answers.append(("scan, 1 GiB (from HBM)", kc["ms"] / ks["ms"]))
    del d_big
    lines.append("-- the statements")
    for x in answers:
        if str(x[0]).startswith("scan"):
            lines.append(f"{x[0]}: the scan kernel runs at half of the checksum's rate or better: {'yes' if x[1] >= 0.5 else 'NO'} (scan rate / checksum rate = {x[1]:.2f})")
        else:
            frames, bs, ri, sd = x
            lines.append(f"{frames} x {bs // MiB} MiB: salvage within 3 % of the whole-archive call: {'yes' if abs(sd - 1) <= 0.03 else 'NO'} (salvage / decompress = {sd:.3f}); "
                         f"recover / index on an undamaged archive = {ri:.3f}")
    if "cli" in parts:
        lines += cli_part(torch, jam, ctx, a.reps, sync)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
