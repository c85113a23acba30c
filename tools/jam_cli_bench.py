"""Whole archives of the stock CLI: the batched call against the frame-by-frame loop:

  a  jam_cli_decompress        the Python loop around jpk_jam_cli_block_read: one frame per call, pre-stages on one host thread; the baseline
  b  Context.jam_cli_decompress  the archive resident in HBM, the output left there
  c  jam_cli_decompress_all    the host form of b: staged per pass, the output copied back

Workloads: with the reference build under oracle/_ref, 64 frames of 1 MiB and 16 frames of 8 MiB of corpus text (one seed per frame) as
`jampack c` writes them with its default settings; without it, the golden frames tiled to --tile frames.  --archive DIR keeps the built
archives there (and reads them back when they exist), so that the reference's compressor need not run where the GPU is.  After one
warm-up of each, the three are timed in turn, --reps rounds, and the medians reported; every call ends in a device synchronise and
every result is compared with the loop's.  One more call of b runs under the context's profiler for the per-kernel table.

  python tools/jam_cli_bench.py [--reps 5] [--tile 64] [--archive DIR] [--out profiles/jam_cli_decompress.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1 << 20


def workloads(jam, tile, keep):
    """[(name, archive)]"""
    from oracle.pyoracle import Ref
    out = []
    if Ref.available() or (keep and os.path.exists(os.path.join(keep, "cli_64x1.npy"))):
        for name, frames, bs in (("64 frames of 1 MiB", 64, MiB), ("16 frames of 8 MiB", 16, 8 * MiB)):
            path = os.path.join(keep, f"cli_{frames}x{bs // MiB}.npy") if keep else None
            if path and os.path.exists(path):
                out.append((name + " of corpus text, reference build, default settings", np.load(path)))
                continue
            ref = Ref()
            a = np.concatenate([ref.jam_comp_block(jam.corpus.make("text", bs, 8000 + i), bs, 0, 1) for i in range(frames)])
            if path:
                os.makedirs(keep, exist_ok=True)
                np.save(path, a)
            out.append((name + " of corpus text, reference build, default settings", a))
        return out
    gold = os.path.join(ROOT, "tests", "golden")
    z, man = np.load(os.path.join(gold, "golden_cli.npz")), json.load(open(os.path.join(gold, "golden_cli_manifest.json")))
    names = [c["name"] for c in man["frames"]]
    a = np.concatenate([z[names[i % len(names)]] for i in range(tile)])
    return [(f"{tile} golden frames (5 KB .. 300 KB raw, BlockSize 1 MiB)", a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--archive", default=None)
    ap.add_argument("--build-only", action="store_true", help="build and keep the archives (needs --archive), no GPU")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import jampack_amd as jam
    loads = workloads(jam, a.tile, a.archive)
    if a.build_only:
        for name, arch in loads:
            print(f"{name}: {len(arch)} bytes")
        return

    import torch
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = [f"tools/jam_cli_bench.py; device: {torch.cuda.get_device_name(0)}; median of {a.reps} alternating rounds after one warm-up, "
             "wall clock with a device synchronise"]
    for name, arch in loads:
        frames, bound, bad = jam.jam_cli_frames(arch)
        assert bad == -1
        d_arch = torch.from_numpy(arch).to(dev)
        d_out = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
        got = {}

        def run(k):
            if k == "a":
                got[k] = jam.jam_cli_decompress(arch)
            elif k == "b":
                n, nf, bf = ctx.jam_cli_decompress(d_arch, len(arch), d_out, bound)
                assert (nf, bf) == (frames, -1)
                got[k] = n
            else:
                got[k] = jam.jam_cli_decompress_all(arch)

        order = ("a", "b", "c")
        for k in order:                                     # warm-up: arenas, scratch, code objects
            run(k)
            sync()
        raw = len(got["a"])
        assert got["b"] == raw and np.array_equal(d_out[:raw].cpu().numpy(), got["a"]) and np.array_equal(got["c"], got["a"])
        times = {k: [] for k in order}
        for _ in range(a.reps):
            for k in order:
                sync()
                t0 = time.perf_counter()
                run(k)
                sync()
                times[k].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        ctx.profile_enable(2)
        run("b")
        table = ctx.profile_table()
        ctx.profile_enable(0)
        total = sum(r["ms"] for r in table)
        lines += [
            "",
            f"{name}: {frames} frames, archive {len(arch)} bytes, raw {raw} bytes",
            f"a  jam_cli_decompress, the loop over frames     {med['a']:9.2f} ms   ({raw / med['a'] / 1e6:.3f} GB/s)",
            f"b  Context.jam_cli_decompress, archive in HBM   {med['b']:9.2f} ms   ({raw / med['b'] / 1e6:.3f} GB/s)",
            f"c  jam_cli_decompress_all, host buffers         {med['c']:9.2f} ms   ({raw / med['c'] / 1e6:.3f} GB/s)",
            f"a / b = {med['a'] / med['b']:.2f}   a / c = {med['a'] / med['c']:.2f}",
            "all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.2f}" for t in times[k]) for k in order),
            f"one call of b under the context's profiler (HIP events on its stream; {total:.2f} ms in kernels):",
        ]
        for r in sorted(table, key=lambda r: -r["ms"]):
            lines.append(f"  {r['name']:<28s} {r['ms']:9.3f} ms  {100 * r['ms'] / max(total, 1e-9):5.1f} %  launches {r['launches']:5d}  units {r['units']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
