"""The index and the range reads of a staged .jam archive resident in HBM against decoding all of it ("Staged frames"):

  a   Context.jam_staged_decompress of the whole archive -- the only way to a slice without the index; the comparison
  i0  Context.jam_staged_index, verify=False: the passes of a up to the filters, then k_lz77_sizes -- no expansion, checksum or gather
  i1  Context.jam_staged_index, verify=True: the passes of a without an output buffer or a gather
  d   one range over the whole archive (every frame's last stage writes in place, nothing is gathered)
  e   one range of BlockSize across a frame boundary in the middle: two frames touched

and, from the context's profile counters over one i0 and one i1, the device time of k_lz77_sizes beside that of the stage that expands
the same frames (k_lzd_plan + k_lzd_copy, and k_pre_lz77 for a frame they leave to it).  Workloads: corpus text with a copy of a fifth of every frame inside it (what the dedupe is for), as 64 frames of 1 MiB and as 4
frames of 64 MiB, written by jam_staged_compress with flags 0 and 1 (JPK_CLI_DEDUPE).  After one warm-up of each, the five are timed in
turn, --reps rounds, and the medians reported; every call ends in a device synchronise and every result is compared with a's output.
It is one GPU step: run it under a time limit of its own,

  timeout -k 10 900 python tools/jam_staged_read_bench.py [--reps 5] [--out profiles/jam_staged_read_ranges.txt]
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
FLAGS = (0, 1)


def workload(torch, jam, frames, bs):
    """frames x bs bytes on the device: tiles of 64 MiB of corpus text, a byte in 4099 changed per frame, a fifth of every frame a copy of
    bytes in front of it"""
    base = torch.from_numpy(np.concatenate([jam.corpus.make("text", MiB, 8000 + i) for i in range(64)])).to("cuda")
    d = base.repeat((frames * bs + len(base) - 1) // len(base))[: frames * bs].contiguous()
    v = d.view(frames, bs)
    v[:, ::4099] ^= torch.arange(frames, dtype=torch.uint8, device="cuda")[:, None]
    fifth = bs // 5
    v[:, 3 * fifth + 1: 4 * fifth + 1] = v[:, 1234: 1234 + fifth].clone()
    return d


def tokens(s1):
    """the tokens of a valid stream of the first LZ77 stage, the end token included (the format of pre::parse_token)"""
    s, pos, count = bytes(s1), 0, 0

    def leb(pos):
        d = 0
        while not s[pos + d] & 0x80:
            d += 1
        x = 0
        for b in s[pos: pos + d + 1]:
            x = (x << 7) | (b & 0x7F)
        return x + ((127, 16510, 2113661, 270549116)[d - 1] if d else 0), pos + d + 1

    while pos < len(s):
        t = s[pos]
        off, pos = leb(pos + 1)
        ln, lit = t >> 3, t & 7
        count += 1
        if ln == 31:
            pos = leb(pos)[1]
        if lit == 7:
            e, pos = leb(pos)
            lit += e
        if off == 0:
            break
        pos += lit
    return count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch                                            # first: torch brings its own HIP runtime, and the library must share it
    import jampack_amd as jam
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = [f"tools/jam_staged_read_bench.py: staged archives of corpus text with a copy of a fifth of every frame inside it, in HBM",
             f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise"]
    answers = []
    for frames, bs in SHAPES:
        d_raw = workload(torch, jam, frames, bs)
        n = frames * bs
        for fl in FLAGS:
            bound = jam.jam_staged_compress_bound(n, bs)
            d_arch = torch.empty(bound + 64, dtype=torch.uint8, device="cuda")
            alen = ctx.jam_staged_compress(d_raw, n, bs, d_arch, bound, flags=fl)
            ref = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
            got, nf, bf, ix = ctx.jam_staged_decompress_ix(d_arch, alen, ref, n)
            assert (got, nf, bf, ix.frames, ix.raw_len, ix.kind) == (n, frames, -1, frames, n, 2) and torch.equal(ref[:n], d_raw)
            out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
            variants = {"d": [(0, n)], "e": [((frames // 2) * bs - bs // 2, bs)]}

            def run(k):
                if k == "a":
                    assert ctx.jam_staged_decompress(d_arch, alen, out, n) == (n, frames, -1)
                elif k in ("i0", "i1"):
                    jx = ctx.jam_staged_index(d_arch, alen, verify=k == "i1")
                    assert (jx.frames, jx.raw_len, jx.bad_frame) == (frames, n, -1)
                    jx.close()
                else:
                    st, bad = ctx.jam_read(ix, d_arch, alen, variants[k], [out.data_ptr()])
                    assert bad == -1

            def verify(k):
                if k in ("a", "d"):
                    assert torch.equal(out[:n], ref[:n]), k
                elif k == "e":
                    off, ln = variants[k][0]
                    assert torch.equal(out[:ln], ref[off: off + ln]), k

            order = ("a", "i0", "i1", "d", "e")
            for k in order:                                 # warm-up: arenas, scratch, code objects
                out.zero_()
                run(k)
                sync()
                verify(k)
            times = {k: [] for k in order}
            for _ in range(a.reps):
                for k in order:
                    sync()
                    t0 = time.perf_counter()
                    run(k)
                    sync()
                    times[k].append(time.perf_counter() - t0)
            med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
            # the last stage on the same frames, by the profile counters: one i0 (k_lz77_sizes) and one i1 (k_lzd_plan + k_lzd_copy, and
            # k_pre_lz77 only where they left a frame to it)
            ctx.profile_enable(2)
            run("i0")
            run("i1")
            sync()
            prof = {r["name"]: r for r in ctx.profile_table()}
            ctx.profile_enable(0)
            ks = prof.get("k_lz77_sizes")
            stage = [prof[k] for k in ("k_lzd_plan", "k_lzd_copy", "k_pre_lz77") if k in prof]
            assert ks and prof.get("k_lzd_plan") and ks["launches"] == prof["k_lzd_plan"]["launches"], (ks, stage)
            stage_ms = sum(r["ms"] for r in stage)
            lines += [
                f"-- {frames} frames of {bs // MiB} MiB, flags {fl}: archive {alen} bytes, raw {n} bytes",
                f"a   jam_staged_decompress, whole archive        {med['a']:9.2f} ms   ({n / med['a'] / 1e6:.3f} GB/s)",
                f"i0  jam_staged_index, verify=0 (sizes only)     {med['i0']:9.2f} ms",
                f"i1  jam_staged_index, verify=1 (one decode)     {med['i1']:9.2f} ms",
                f"d   one range over the whole archive            {med['d']:9.2f} ms   ({n / med['d'] / 1e6:.3f} GB/s)",
                f"e   one range of BlockSize across two frames    {med['e']:9.2f} ms",
                f"d / a = {med['d'] / med['a']:.3f}   i0 / a = {med['i0'] / med['a']:.3f}   i1 / a = {med['i1'] / med['a']:.3f}   a / e = {med['a'] / med['e']:.1f}",
                f"device time over {ks['launches']} pass(es) each: k_lz77_sizes {ks['ms']:.3f} ms, the expanding stage " + " + ".join(f"{r['name']} {r['ms']:.3f}" for r in stage)
                + f" = {stage_ms:.3f} ms  (sizes / stage = {ks['ms'] / stage_ms:.3f})",
                "all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.2f}" for t in times[k]) for k in order),
            ]
            answers.append((frames, bs, fl, med["d"] / med["a"], med["i0"] / med["a"]))
            ix.close()
            del d_arch, ref, out
        del d_raw
    # the token walk where it is long: the dedupe's S1' of a 300-byte period is about one token per 500 input bytes, near its bound of
    # n / 256 + 2 -- the archives above hold a handful of tokens per frame
    lines.append("-- one block of a 300-byte period through the dedupe: k_lz77_sizes beside k_pre_lz77 on its S1', device time of one launch each after a warm-up")
    period = np.random.default_rng(300).integers(0, 256, 300, dtype=np.uint8)
    for mib in (1, 64):
        n = mib * MiB
        d_t = torch.from_numpy(np.tile(period, n // 300 + 1)[:n].copy()).to("cuda")
        d_s1 = torch.empty(n + 66, dtype=torch.uint8, device="cuda")
        d_back = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        (s1_len,), (st,) = ctx.blocks_lz77_dedupe([d_t], [n], [d_s1], [n + 2])
        assert st == 0
        for rep in range(2):                                # the second round under the profiler
            if rep:
                ctx.profile_enable(2)
            assert ctx.blocks_lz77_sizes([d_s1], [s1_len], [n]) == ([n], [0])
            assert ctx.blocks_lz77_decompress([d_s1], [s1_len], [d_back], [n]) == ([n], [0])
        prof = {r["name"]: r for r in ctx.profile_table()}
        ctx.profile_enable(0)
        assert torch.equal(d_back[:n], d_t)
        ntok = tokens(d_s1[:s1_len].cpu().numpy())
        ks, kp = prof["k_lz77_sizes"]["ms"], prof["k_pre_lz77"]["ms"]
        lines.append(f"{mib:3d} MiB: |S1'| {s1_len} bytes, {ntok} tokens (bound {n // 256 + 2}): k_lz77_sizes {ks:9.3f} ms ({ks * 1e3 / ntok:.3f} us per token), "
                     f"k_pre_lz77 {kp:9.3f} ms  (sizes / serial = {ks / kp:.3f})")
        del d_t, d_s1, d_back
    lines.append("-- the two statements")
    for frames, bs, fl, da, ia in answers:
        lines.append(f"{frames} x {bs // MiB} MiB, flags {fl}: a range over the whole archive within 3 % of the whole-archive call: "
                     f"{'yes' if abs(da - 1) <= 0.03 else 'NO'} (d / a = {da:.3f}); the verify=0 index takes less than the whole-archive call: "
                     f"{'yes' if ia < 1 else 'NO'} (i0 / a = {ia:.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
