"""Staged frames ("Staged frames") against the entries the library already had, in one build:

  (a) writer    Context.jam_staged_compress with flags 0, 1 (dedupe) and 5 (dedupe + filters) against Context.jam_compress (plain frames)
                and Context.jam_cli_compress with the same flags (stock-CLI frames): GB/s, archive bytes, sa_rounds of the first block
  (b) reader    Context.jam_staged_decompress of those archives against Context.jam_decompress of the plain one
  (c) expander  Context.blocks_lz77_expand and Context.blocks_lz77_expand_deep (the staged reader's last stage) against
                Context.blocks_lz77_decompress on the same S1 streams -- stored (04 80 | R) and deduped (Context.blocks_lz77_dedupe) -- of
                1, 8 and 64 MiB blocks, one block and 16 blocks per call, with the blocks each path took and, from a token walk on the
                host, every stream's records and its deepest byte
  (w) worst     one 64 MiB block of matches at distance 3 stacked H deep (H = lz77_deep_limits()[0]), inside the record budget: every byte
                takes the per-byte chase through H records.  The deep entry against the serial one, once (--only w)

Inputs: corpus text (64 generations of 1 MiB; the 256 MiB input is that in four block orders) and corpus.system_sources, as 64 frames of
1 MiB and as 4 frames of 64 MiB.  Every workload runs in a process of its own under `timeout -k 10` (--limit seconds); the first that fails
or runs out of time ends the tool.  Times are the median of --reps alternating rounds after one warm-up, wall clock with a device synchronise.

  python tools/jam_staged_bench.py [--reps 5] [--limit 300] [--out profiles/jam_staged.txt]
"""
import argparse
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1 << 20
SHAPES = (("64x1", MiB, 64), ("4x64", 64 * MiB, 4))
INPUTS = (("text", "corpus text"), ("sources", "corpus.system_sources"))


def _text_piece(i):
    import jampack_amd.corpus as corpus
    return corpus.make("text", MiB, 8000 + i)


def make_inputs(tmp):
    """text.npy (64 MiB) and sources.npy (256 MiB) in tmp; the parent makes them once (on CPUs: it never opens the GPU)"""
    import jampack_amd.corpus as corpus
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        pieces = list(ex.map(_text_piece, range(64)))
    np.save(os.path.join(tmp, "text.npy"), np.concatenate(pieces))
    src = corpus.system_sources(256 * MiB)
    if src is None:
        raise SystemExit("corpus.system_sources holds less than 256 MiB on this image")
    np.save(os.path.join(tmp, "sources.npy"), src)


def load(tmp, key, nbytes):
    a = np.load(os.path.join(tmp, key + ".npy"))
    if key == "text" and nbytes > len(a):                      # four orders of the 64 pieces: every 64 MiB frame holds each piece once
        a = np.concatenate([np.roll(a.reshape(64, MiB), 16 * k, axis=0).reshape(-1) for k in range(nbytes // len(a))])
    return np.ascontiguousarray(a[:nbytes])


def medians(variants, reps, sync):
    """{name: callable} -> {name: (median ms, all rounds ms)}, alternating rounds after one warm-up each"""
    for f in variants.values():
        f()
        sync()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), v) for k, v in times.items()}


def measure_archive(tmp, key, shape, reps):
    import torch
    import jampack_amd as jam
    _, bs, frames = next(s for s in SHAPES if s[0] == shape)
    n = bs * frames
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    sync = torch.cuda.synchronize
    d_in = torch.from_numpy(load(tmp, key, n)).to("cuda")
    cap = jam.jam_staged_compress_bound(n, bs)
    names = ["plain"] + [f"staged {f}" for f in (0, 1, 5)] + [f"cli {f}" for f in (0, 1, 5)]
    d_arch = {k: torch.empty(cap + 64, dtype=torch.uint8, device="cuda") for k in names}
    d_back = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    size = {}

    def writer(k):
        kind, _, fl = k.partition(" ")
        fl = int(fl or 0)
        if kind == "plain":
            return lambda: size.__setitem__(k, ctx.jam_compress(d_in, n, bs, d_arch[k], cap))
        if kind == "staged":
            return lambda: size.__setitem__(k, ctx.jam_staged_compress(d_in, n, bs, d_arch[k], cap, flags=fl))
        return lambda: size.__setitem__(k, ctx.jam_cli_compress(d_in, n, bs, d_arch[k], cap, dedupe=bool(fl & 1), filters=bool(fl & 4)))

    w = medians({k: writer(k) for k in names}, reps, sync)

    def reader(k):
        if k == "plain":
            return lambda: ctx.jam_decompress(d_arch[k], size[k], d_back, n)
        return lambda: ctx.jam_staged_decompress(d_arch[k], size[k], d_back, n)

    rnames = names[:4]
    for k in rnames:                                            # every archive decodes to its input
        d_back.zero_()
        assert reader(k)()[0] == n and torch.equal(d_back[:n], d_in), k
    r = medians({k: reader(k) for k in rnames}, reps, sync)
    # sa_rounds of the first block: its BWT input through the single-block entry of this context (a staged frame's is its decoded payload)
    rounds = {}
    d_s2 = torch.empty(jam.cli_stages_bound(bs) + 64, dtype=torch.uint8, device="cuda")
    d_tmp = torch.empty(jam.ans_capacity(jam.cli_stages_bound(bs) + 480), dtype=torch.uint8, device="cuda")
    for k in rnames:
        if k == "plain":
            src, m = d_in, bs
        else:
            head = d_arch[k][:15].cpu().numpy()
            psize = int(np.frombuffer(head[7:11].tobytes(), dtype="<i4")[0])
            (m,), st = ctx.blocks_decompress([d_arch[k][15:]], [psize], [d_s2], [d_s2.numel()])
            assert st == [0], k
            src = d_s2
        ctx.block_compress(src, m, d_tmp, d_tmp.numel())
        rounds[k] = ctx.stats().sa_rounds
    lines = [f"device: {torch.cuda.get_device_name(0)}; raw {n} bytes, {frames} frames of {bs // MiB} MiB"]
    for k in names:
        ms, allr = w[k]
        lines.append(f"write {k:<9s} {ms:9.2f} ms  {n / ms / 1e6:7.3f} GB/s  archive {size[k]:>10d} bytes ({size[k] / size['plain']:.4f} of plain)"
                     + (f"  sa_rounds of block 0: {rounds[k]}" if k in rounds else "") + "   rounds: " + " ".join(f"{t:.2f}" for t in allr))
    for k in rnames:
        ms, allr = r[k]
        lines.append(f"read  {k:<9s} {ms:9.2f} ms  {n / ms / 1e6:7.3f} GB/s   rounds: " + " ".join(f"{t:.2f}" for t in allr))
    for f in (0, 1, 5):
        lines.append(f"staged {f}: write {w['plain'][0] / w[f'staged {f}'][0]:.3f} x plain, {w[f'cli {f}'][0] / w[f'staged {f}'][0]:.2f} x cli {f}; "
                     f"read {r['plain'][0] / r[f'staged {f}'][0]:.3f} x plain")
    ctx.close()
    return lines


LEB_OFF = (127, 16510, 2113661, 270549116)


def stream_shape(s1, raw_len):
    """(records, deepest byte) of a valid S1 stream by a token walk on the host: what decides the expander's path -- at most
    len(s1) / 64 + 4 records and no byte more than 8 hops from a literal.  A byte of a match is one hop deeper than its source byte,
    k mod off behind the match's start (the period repeats)."""
    s = bytes(s1)

    def rd(pos):
        d, x = 0, 0
        while not s[pos + d] & 0x80:
            x = (x << 7) | s[pos + d]
            d += 1
        x = (x << 7) | (s[pos + d] & 0x7F)
        return x + (LEB_OFF[d - 1] if d else 0), pos + d + 1

    depth = np.zeros(raw_len, dtype=np.uint8)
    pos, op, nrec, deepest = 0, 0, 0, 0
    while pos < len(s):
        t = s[pos]
        off, pos = rd(pos + 1)
        ln, lit = t >> 3, t & 7
        if ln == 31:
            e, pos = rd(pos)
            ln += e
        if lit == 7:
            e, pos = rd(pos)
            lit += e
        if off == 0:
            return nrec + (1 if pos < len(s) else 0), deepest
        ln += 4
        nrec += (1 if lit else 0) + 1
        pos += lit
        op += lit
        new = np.minimum(np.resize(depth[op - off: op], ln), 254) + 1
        depth[op: op + ln] = new
        deepest = max(deepest, int(new.max()))
        op += ln
    return nrec, deepest


def measure_expander(tmp, key, reps):
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    sync = torch.cuda.synchronize
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    hops, per, slack = jam.lz77_deep_limits()
    for mib in (1, 8, 64):
        n = mib * MiB
        raw = load(tmp, key, n)
        d_raw = torch.from_numpy(raw).to("cuda")
        d_s1 = {"stored": torch.from_numpy(np.concatenate([np.array([4, 0x80], dtype=np.uint8), raw])).to("cuda"),
                "deduped": torch.empty(n + 64, dtype=torch.uint8, device="cuda")}
        (m,), st = ctx.blocks_lz77_dedupe([d_raw], [n], [d_s1["deduped"]], [n + 2])
        assert st == [0]
        s1_len = {"stored": n + 2, "deduped": m}
        shape = {form: stream_shape(d_s1[form][: s1_len[form]].cpu().numpy(), n) for form in s1_len}
        for form, (nrec, deepest) in shape.items():
            lines.append(f"{mib:3d} MiB  {form:<8s} |S1| {s1_len[form]:>9d}  records {nrec} (cap {s1_len[form] // 64 + 4}; deep: {n // per + slack + 4})  "
                         f"deepest byte {deepest} hops (cap 8; deep: {hops})")
        for nblk in (1, 16):
            d_out = [torch.empty(n + 64, dtype=torch.uint8, device="cuda") for _ in range(nblk)]
            for form in ("stored", "deduped"):
                ins, lens, caps = [d_s1[form]] * nblk, [s1_len[form]] * nblk, [n] * nblk

                def expand():
                    ol, st = ctx.blocks_lz77_expand(ins, lens, d_out, caps)
                    assert st == [0] * nblk and ol == [n] * nblk

                def deep():
                    ol, st = ctx.blocks_lz77_expand_deep(ins, lens, d_out, caps)
                    assert st == [0] * nblk and ol == [n] * nblk

                def serial():
                    ol, st = ctx.blocks_lz77_decompress(ins, lens, d_out, caps)
                    assert st == [0] * nblk and ol == [n] * nblk

                for f in (serial, expand, deep):                # all give the raw block back
                    d_out[-1].zero_()
                    f()
                    assert torch.equal(d_out[-1][:n], d_raw), (form, f.__name__)
                path, dpath = ctx.lz77_expand_last(), ctx.lz77_deep_last()
                t = medians({"serial": serial, "expand": expand, "deep": deep}, reps, sync)
                tot = n * nblk
                lines.append(f"{mib:3d} MiB x {nblk:2d}  {form:<8s} |S1| {s1_len[form]:>9d}  serial {t['serial'][0]:9.3f} ms {tot / t['serial'][0] / 1e6:8.2f} GB/s   "
                             f"expand {t['expand'][0]:9.3f} ms {tot / t['expand'][0] / 1e6:8.2f} GB/s   serial / expand {t['serial'][0] / t['expand'][0]:7.2f}   "
                             f"blocks parallel {path[0]} serial {path[1]}   "
                             f"deep {t['deep'][0]:9.3f} ms {tot / t['deep'][0] / 1e6:8.2f} GB/s   serial / deep {t['serial'][0] / t['deep'][0]:7.2f}   "
                             f"blocks parallel {dpath[0]} serial {dpath[1]}   rounds: serial " + " ".join(f"{x:.3f}" for x in t["serial"][1])
                             + "; expand " + " ".join(f"{x:.3f}" for x in t["expand"][1]) + "; deep " + " ".join(f"{x:.3f}" for x in t["deep"][1]))
            del d_out
    ctx.close()
    return lines


def leb(v):
    """Utils::EncodeLeb128 as pre::leb_write has it"""
    if v < LEB_OFF[0]:
        return bytes([v | 0x80])
    for d in range(1, 5):
        if d == 4 or v < LEB_OFF[d]:
            x = v - LEB_OFF[d - 1]
            return bytes([(x >> (7 * (d - k))) & 0x7F for k in range(d)] + [0x80 | (x & 0x7F)])


def measure_worst():
    """one run of each entry after a warm-up of each: the block is made to be slow"""
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    sync = torch.cuda.synchronize
    hops = jam.lz77_deep_limits()[0]
    n, lit = 64 * MiB, 4096
    ln = (n - lit) // hops                                      # hops matches of ln bytes at distance 3 behind 4 KiB of literals
    rest = n - lit - hops * ln
    s = bytes([(31 << 3) | 7]) + leb(3) + leb(ln - 35) + leb(lit - 7) + np.random.default_rng(3).integers(0, 256, lit, dtype=np.uint8).tobytes()
    s += (bytes([31 << 3]) + leb(3) + leb(ln - 35)) * (hops - 1) + bytes([4, 0x80]) + bytes(rest)
    nrec, deepest = stream_shape(s, n)
    d_s1 = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).to("cuda")
    d_out = [torch.empty(n + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    ms = {}
    for k, (name, fn) in enumerate((("serial", ctx.blocks_lz77_decompress), ("deep", ctx.blocks_lz77_expand_deep))):
        for _ in range(2):                                      # warm-up, then the run that counts
            d_out[k].zero_()
            sync()
            t0 = time.perf_counter()
            ol, st = fn([d_s1], [len(s)], [d_out[k]], [n])
            sync()
            ms[name] = (time.perf_counter() - t0) * 1e3
            assert st == [0] and ol == [n], name
    assert torch.equal(d_out[0][:n], d_out[1][:n]) and ctx.lz77_deep_last() == (1, 0)
    ctx.close()
    return [f"device: {torch.cuda.get_device_name(0)}",
            f"64 MiB, {hops} matches of {ln} bytes at distance 3 behind {lit} literals: |S1| {len(s)}, records {nrec}, deepest byte {deepest} hops",
            f"serial {ms['serial']:9.3f} ms   deep {ms['deep']:9.3f} ms (parallel path)   serial / deep {ms['serial'] / ms['deep']:.2f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds for every workload")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated workload keys, e.g. a:text:64x1,c:sources")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)       # internal: one workload in a process of its own
    ap.add_argument("--data", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        part, key, *shape = a.step.split(":")
        if part == "w":
            print(json.dumps(measure_worst()))
        else:
            print(json.dumps(measure_archive(a.data, key, shape[0], a.reps) if part == "a" else measure_expander(a.data, key, a.reps)))
        return
    lines = [f"python tools/jam_staged_bench.py --reps {a.reps}" + (f" --only {a.only}" if a.only else ""),
             f"median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise"]
    steps = [(f"a:{key}:{shape}", f"(a, b) writer and reader, {frames} frames of {bs // MiB} MiB of {name}") for key, name in INPUTS for shape, bs, frames in SHAPES]
    steps += [(f"c:{key}", f"(c) expanders against the serial kernel, S1 of {name}") for key, name in INPUTS]
    if a.only and "w:" in a.only.split(","):                   # only on request: it is one slow block, timed once
        steps.append(("w:", "(w) the per-byte chase at its worst: distance 3, H deep, 64 MiB"))
    failed = None
    with tempfile.TemporaryDirectory() as tmp:
        if not a.only or any(k[0] != "w" for k in a.only.split(",")):
            make_inputs(tmp)
        for step, title in steps:
            if a.only and step not in a.only.split(","):
                continue
            lines += ["", title]
            print(title, file=sys.stderr, flush=True)
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", step, "--data", tmp],
                               capture_output=True, text=True)
            if r.returncode != 0:
                failed = f"{step}: the measuring process ended with {r.returncode}; nothing more is started"
                lines.append(failed)
                print(r.stdout[-2000:], r.stderr[-3000:], sep="\n", file=sys.stderr)
                break
            lines += json.loads(r.stdout.strip().splitlines()[-1])
    out = "\n".join(lines) + "\n"
    print(out, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    if failed:
        raise SystemExit(failed)


if __name__ == "__main__":
    main()
