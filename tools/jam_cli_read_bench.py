"""Range reads of a stock-CLI .jam archive resident in HBM against decoding all of it:

  a  Context.jam_cli_decompress of the whole archive -- the only way to a slice without the index; the comparison
  i  Context.jam_cli_index: the index, made by decoding the archive once (the passes of a without an output buffer or a gather)
  b  ranges that add up to 1 frame's worth of bytes: one range of BlockSize across a frame boundary in the middle
  c  16 frames' worth: 16 ranges of BlockSize at seeded random offsets, one call
  d  all frames' worth: one range over the whole archive (every frame's last stage writes in place, nothing is gathered)

Workload: the first archive of tools/jam_cli_bench.py -- with the reference build under oracle/_ref, 64 frames of 1 MiB of corpus text
as `jampack c` writes them with its default settings (--archive DIR keeps it there and reads it back, --build-only builds it without a
GPU); without it, the same text through jam_cli_compress.  After one warm-up of each, the five are timed in turn, --reps rounds, and the
medians reported; every call ends in a device synchronise and every result is compared with a's output.

  python tools/jam_cli_read_bench.py [--reps 5] [--archive DIR] [--out profiles/jam_cli_read_ranges.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1 << 20
FRAMES = 64


def workload(jam, keep, build_only):
    """(name, archive): 64 frames of 1 MiB of corpus text"""
    from oracle.pyoracle import Ref
    path = os.path.join(keep, f"cli_{FRAMES}x1.npy") if keep else None
    if path and os.path.exists(path):
        return "reference build, default settings", np.load(path)
    blocks = [jam.corpus.make("text", MiB, 8000 + i) for i in range(FRAMES)]
    if Ref.available():
        ref = Ref()
        name, a = "reference build, default settings", np.concatenate([ref.jam_comp_block(b, MiB, 0, 1) for b in blocks])
    elif build_only:
        raise SystemExit("--build-only needs the reference build under oracle/_ref")
    else:
        name, a = "jam_cli_compress", jam.jam_cli_compress(np.concatenate(blocks), MiB)
    if path:
        os.makedirs(keep, exist_ok=True)
        np.save(path, a)
    return name, a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--archive", default=None)
    ap.add_argument("--build-only", action="store_true", help="build and keep the archive (needs --archive), no GPU")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    if not a.build_only:
        import torch                                        # first: torch brings its own HIP runtime, and the library must share it
    import jampack_amd as jam
    name, arch = workload(jam, a.archive, a.build_only)
    if a.build_only:
        print(f"{FRAMES} frames of 1 MiB, {name}: {len(arch)} bytes")
        return

    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    frames, bound, bad = jam.jam_cli_frames(arch)
    assert (frames, bad) == (FRAMES, -1)
    d_arch = torch.from_numpy(arch).to(dev)
    ref = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
    n, nf, bf, ix = ctx.jam_cli_decompress_ix(d_arch, len(arch), ref, bound)
    assert (nf, bf, ix.frames, ix.raw_len, ix.kind) == (frames, -1, frames, n, 1)
    bs = MiB

    rng = np.random.default_rng(11)
    variants = {
        "b": [((frames // 2) * bs - bs // 2, bs)],
        "c": [(int(o), bs) for o in rng.integers(0, n - bs, 16)],
        "d": [(0, n)],
    }
    out = torch.empty(bound + 64, dtype=torch.uint8, device=dev)

    def place(ranges):
        ptrs, pos = [], 0
        for _, ln in ranges:
            ptrs.append(out.data_ptr() + pos)
            pos += ln
        return ptrs

    ptrs = {k: place(v) for k, v in variants.items()}

    def run(k):
        if k == "a":
            assert ctx.jam_cli_decompress(d_arch, len(arch), out, bound) == (n, frames, -1)
        elif k == "i":
            jx = ctx.jam_cli_index(d_arch, len(arch))
            assert (jx.frames, jx.raw_len, jx.bad_frame) == (frames, n, -1)
            jx.close()
        else:
            st, bad = ctx.jam_read(ix, d_arch, len(arch), variants[k], ptrs[k])
            assert bad == -1

    def verify(k):
        if k == "i":
            return
        if k in ("a", "d"):
            assert torch.equal(out[:n], ref[:n]), k
            return
        pos = 0
        for off, ln in variants[k]:
            assert torch.equal(out[pos: pos + ln], ref[off: off + ln]), (k, off)
            pos += ln

    order = ("a", "i", "b", "c", "d")
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
        f"tools/jam_cli_read_bench.py: {frames} frames of 1 MiB of corpus text ({name}; archive {len(arch)} bytes, raw {n} bytes) in HBM",
        f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise",
        f"a  jam_cli_decompress, whole archive          {med['a']:9.2f} ms   ({n / med['a'] / 1e6:.3f} GB/s)",
        f"i  jam_cli_index, the index by one decode     {med['i']:9.2f} ms   ({n / med['i'] / 1e6:.3f} GB/s)",
        f"b  one range of 1 MiB across two frames       {med['b']:9.2f} ms   frames touched: {touched(variants['b'])}",
        f"c  16 ranges of 1 MiB, one call               {med['c']:9.2f} ms   frames touched: {touched(variants['c'])}",
        f"d  one range over the whole archive           {med['d']:9.2f} ms   ({n / med['d'] / 1e6:.3f} GB/s)",
        f"d / a = {med['d'] / med['a']:.3f}   i / a = {med['i'] / med['a']:.3f}   a / b = {med['a'] / med['b']:.1f}   a / c = {med['a'] / med['c']:.2f}",
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
