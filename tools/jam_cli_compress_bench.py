"""Writing archives the stock CLI decodes: the batched writer against the plain one (writing):

  a  Context.jam_cli_compress   jpk_dev_jam_cli_compress: k_enc_wrap + k_enc_lpx in front of the batch compress, input and archive in HBM
  b  Context.jam_compress       jpk_dev_jam_compress on the same bytes: the comparator (frames the stock CLI rejects)
  c  one call of a under the context's profiler: the per-kernel table, the share of k_enc_lpx and k_enc_wrap
  d  with the reference build under oracle/_ref: wall time and archive size of `jampack_ref c -m0 -f0` at the same block size

Workloads: 64 frames of 1 MiB and 16 frames of 8 MiB of corpus text (one seed per frame), device buffers.  Every workload is measured
in a process of its own under a time limit (--limit seconds), and so is every run of the reference program; the first step that fails
or runs out of time ends the tool.  After one warm-up of each, a and b are timed in turn, --reps rounds, and the medians reported;
every call ends in a device synchronise, and the archive of a is decoded back by the batched decoder and compared with the input.

  python tools/jam_cli_compress_bench.py [--reps 5] [--limit 240] [--out profiles/jam_cli_compress.txt]
"""
import argparse
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
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "jampack_ref")
WORKLOADS = (("64 frames of 1 MiB", 64, MiB), ("16 frames of 8 MiB", 16, 8 * MiB))
# k_enc_lpx, from its code object (prestage_dev.hip): tables 3 x 256 x 20 B + ring 80 KiB + tile 16 KiB
LPX_LDS = 3 * 256 * 20 + (80 << 10) + (16 << 10)
CU_LDS = 160 << 10


def text(jam, frames, bs):
    return np.concatenate([jam.corpus.make("text", bs, 8000 + i) for i in range(frames)])


def measure(frames, bs, reps):
    """one workload in this process -> the lines of its report"""
    import torch
    import jampack_amd as jam
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    data = text(jam, frames, bs)
    n = len(data)
    d_in = torch.from_numpy(data).to(dev)
    cap = max(jam.jam_cli_compress_bound(n, bs), jam.jam_compress_bound(n, bs))
    d_out = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    size = {}

    def run(k):
        size[k] = ctx.jam_cli_compress(d_in, n, bs, d_out, cap) if k == "a" else ctx.jam_compress(d_in, n, bs, d_out, cap)

    order = ("a", "b")
    for k in order:                                         # warm-up: arenas, scratch, worker contexts, code objects
        run(k)
        sync()
    run("a")
    d_back = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    assert ctx.jam_cli_decompress(d_out, size["a"], d_back, n) == (n, frames, -1)
    assert torch.equal(d_back[:n], d_in), "the archive of a does not decode to its input"
    times = {k: [] for k in order}
    for _ in range(reps):
        for k in order:
            sync()
            t0 = time.perf_counter()
            run(k)
            sync()
            times[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    ctx.profile_enable(2)
    run("a")
    sync()
    table = ctx.profile_table()
    ctx.profile_enable(0)
    total = sum(r["ms"] for r in table)
    lines = [
        f"device: {torch.cuda.get_device_name(0)}; raw {n} bytes",
        f"a  Context.jam_cli_compress (stock-CLI frames)   {med['a']:9.2f} ms   ({n / med['a'] / 1e6:.3f} GB/s)   archive {size['a']} bytes",
        f"b  Context.jam_compress (plain frames)           {med['b']:9.2f} ms   ({n / med['b'] / 1e6:.3f} GB/s)   archive {size['b']} bytes",
        f"a / b = {med['a'] / med['b']:.2f}",
        "all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.2f}" for t in times[k]) for k in order),
        f"c  one call of a under the context's profiler (HIP events on the calling context's stream, the workers' kernels of the batch "
        f"compress are not on it; {total:.2f} ms in kernels):",
    ]
    for r in sorted(table, key=lambda r: -r["ms"]):
        lines.append(f"  {r['name']:<28s} {r['ms']:9.3f} ms  {100 * r['ms'] / max(total, 1e-9):5.1f} %  launches {r['launches']:5d}  units {r['units']}")
    for k in ("k_enc_wrap", "k_enc_lpx"):
        ms = sum(r["ms"] for r in table if r["name"] == k)
        lines.append(f"  {k}: {ms:.3f} ms = {100 * ms / med['a']:.1f} % of a's wall time; a - b = {med['a'] - med['b']:.2f} ms")
    ctx.close()
    return lines


def reference(frames, bs, limit):
    """d: the stock compressor on the same bytes, on this box's CPUs"""
    import jampack_amd as jam
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "ref.jam")
        text(jam, frames, bs).tofile(src)
        t0 = time.perf_counter()
        r = subprocess.run([REF_CLI, "c", src, dst, f"-b{bs // MiB}", "-m0", "-f0"], capture_output=True, text=True, timeout=limit)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit(f"jampack_ref c failed ({r.returncode}): {r.stderr[-500:]}")
        return [f"d  jampack_ref c -b{bs // MiB} -m0 -f0 (default threads)     {dt * 1e3:9.2f} ms   ({frames * bs / dt / 1e9:.3f} GB/s)   "
                f"archive {os.path.getsize(dst)} bytes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for every measured step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)       # internal: one workload in a process of its own
    a = ap.parse_args()
    if a.step:
        frames, bs = (int(x) for x in a.step.split("x"))
        print(json.dumps(measure(frames, bs, a.reps)))
        return

    lines = [f"tools/jam_cli_compress_bench.py; median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise",
             f"k_enc_lpx: {LPX_LDS} bytes of LDS per workgroup (one chain), {CU_LDS // LPX_LDS} workgroup per CU of {CU_LDS} bytes"]
    for name, frames, bs in WORKLOADS:
        lines += ["", f"{name} of corpus text, block_size {bs // MiB} MiB"]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", f"{frames}x{bs}"], capture_output=True, text=True,
                           timeout=a.limit)
        if r.returncode != 0:
            raise SystemExit(f"{name}: the measuring process ended with {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        lines += json.loads(r.stdout.strip().splitlines()[-1])
        lines += reference(frames, bs, a.limit) if os.path.exists(REF_CLI) else ["d  not measured: oracle/_ref/jampack_ref is not built"]
    out = "\n".join(lines) + "\n"
    print(out, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
