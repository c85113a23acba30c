"""Range reads of a .jam archive resident in HBM against decoding all of it:

  a  Context.jam_decompress of the whole archive -- the only way to a slice without jpk_dev_jam_read; the baseline
  b  one 1 MiB range in the middle of a frame
  c  256 ranges of 64 KiB at seeded random offsets, one call
  d  one range over the whole archive (decoded in place, nothing gathered)

Workload: 256 MiB of corpus text, one seed per block, as 8 MiB frames.  After one warm-up of each, the four are timed in turn, five
rounds, and the medians reported; every call ends in a device synchronise and every result is compared with the input.  The index is
built once, outside the timings (a's call includes its own frame walk).

  python tools/jam_read_bench.py [--mib 256] [--frame-mib 8] [--reps 5] [--out profiles/jam_read_ranges.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MiB = 1 << 20
KiB = 1 << 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--frame-mib", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import jampack_amd as jam
    from jam_archive_bench import make_input

    n, bs = a.mib * MiB, a.frame_mib * MiB
    data = make_input(n, bs, 7000)                          # (worker processes: before the GPU is initialised)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    d_in = torch.from_numpy(data).to(dev)
    bound = jam.jam_compress_bound(n, bs)
    d_arch = torch.empty(bound, dtype=torch.uint8, device=dev)
    m = ctx.jam_compress(d_in.data_ptr(), n, bs, d_arch.data_ptr(), bound)
    ix = ctx.jam_index(d_arch, m)
    assert (ix.raw_len, ix.bad_frame) == (n, -1)

    rng = np.random.default_rng(11)
    mid = (ix.frames // 2) * bs + bs // 2 - MiB // 2
    variants = {
        "b": [(mid, MiB)],
        "c": [(int(o), 64 * KiB) for o in rng.integers(0, n - 64 * KiB, 256)],
        "d": [(0, n)],
    }
    out = torch.empty(n + 64, dtype=torch.uint8, device=dev)

    def place(ranges):
        ptrs, pos = [], 0
        for _, ln in ranges:
            ptrs.append(out.data_ptr() + pos)
            pos += ln
        return ptrs

    ptrs = {k: place(v) for k, v in variants.items()}

    def run(k):
        if k == "a":
            assert ctx.jam_decompress(d_arch, m, out.data_ptr(), n) == (n, ix.frames, -1)
        else:
            st, bad = ctx.jam_read(ix, d_arch, m, variants[k], ptrs[k])
            assert bad == -1

    def verify(k):
        if k in ("a", "d"):
            assert torch.equal(out[:n], d_in), k
            return
        pos = 0
        for off, ln in variants[k]:
            assert torch.equal(out[pos: pos + ln], d_in[off: off + ln]), (k, off)
            pos += ln

    order = ("a", "b", "c", "d")
    for k in order:                                         # warm-up: arenas, scratch, code objects
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

    def touched(ranges):
        return len({f for off, ln in ranges for f in range(off // bs, (off + ln - 1) // bs + 1)})

    lines = [
        f"tools/jam_read_bench.py: {a.mib} MiB of corpus text as {a.frame_mib} MiB frames ({ix.frames} frames, archive {m} bytes) in HBM",
        f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise",
        f"a  jam_decompress, whole archive              {med['a']:9.2f} ms   ({n / med['a'] / 1e6:.2f} GB/s)",
        f"b  one 1 MiB range inside a frame             {med['b']:9.2f} ms   frames touched: {touched(variants['b'])}",
        f"c  256 ranges of 64 KiB, one call             {med['c']:9.2f} ms   frames touched: {touched(variants['c'])}",
        f"d  one range over the whole archive           {med['d']:9.2f} ms   ({n / med['d'] / 1e6:.2f} GB/s)",
        f"d / a = {med['d'] / med['a']:.3f}   a / b = {med['a'] / med['b']:.1f}   a / c = {med['a'] / med['c']:.2f}",
        "all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.2f}" for t in times[k]) for k in order),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
