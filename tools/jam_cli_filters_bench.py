"""The filter option of the stock-CLI writer ("Filters") against the same call without it, which is the writer as it was:

  off  Context.jam_cli_compress(..., filters=False)   jpk_dev_jam_cli_compress_ex, flags = 0: k_enc_wrap writes every piece stored
  on   Context.jam_cli_compress(..., filters=True)    flags = JPK_CLI_FILTERS: k_enc_filters in its place

Workloads, 64 frames of 1 MiB each: stereo16 (two corpus samples16 streams interleaved as 16-bit pairs: what the option is for), corpus
text (every piece stays stored: the price of the option) and corpus silesia (the project's mixed workload, 15 % samples16).  Per workload,
with the option off and on: archive size, GB/s (median of --reps alternating rounds after one warm-up, wall clock with a device
synchronise), and the per-kernel table of one profiled call with the share of k_enc_filters.  Every workload runs in a process of its own
under a time limit (--limit seconds); the first that fails or runs out of time ends the tool.

  python tools/jam_cli_filters_bench.py [--reps 5] [--limit 240] [--out profiles/jam_cli_filters.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1 << 20
FRAMES = 64
WORKLOADS = (("stereo16", "two samples16 streams interleaved as 16-bit pairs"), ("text", "corpus text"), ("silesia", "corpus silesia"))


def load(jam, key):
    n = FRAMES * MiB
    if key == "stereo16":
        a, b = jam.corpus.samples16(n // 2, 1).view(np.uint16), jam.corpus.samples16(n // 2, 2).view(np.uint16)
        return np.stack([a, b], axis=1).reshape(-1).view(np.uint8)[:n].copy()
    if key == "text":
        return np.concatenate([jam.corpus.make("text", MiB, 8000 + i) for i in range(FRAMES)])
    return jam.corpus.make("silesia", n, 5)


def measure(key, reps):
    import torch
    import jampack_amd as jam
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    data = load(jam, key)
    n = len(data)
    d_in = torch.from_numpy(data).to(dev)
    cap = jam.jam_cli_compress_bound(n, MiB)
    d_out = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    d_back = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    size = {}

    def run(k):
        size[k] = ctx.jam_cli_compress(d_in, n, MiB, d_out, cap, filters=(k == "on"))

    order = ("off", "on")
    for k in order:                                         # warm-up, and the archive decodes to its input
        run(k)
        sync()
        assert ctx.jam_cli_decompress(d_out, size[k], d_back, n)[0] == n and torch.equal(d_back[:n], d_in), k
    times = {k: [] for k in order}
    for _ in range(reps):
        for k in order:
            sync()
            t0 = time.perf_counter()
            run(k)
            sync()
            times[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    lines = [f"device: {torch.cuda.get_device_name(0)}; raw {n} bytes, {FRAMES} frames"]
    for k in order:
        lines.append(f"{k:<3s} jpk_dev_jam_cli_compress_ex  {med[k]:9.2f} ms   ({n / med[k] / 1e6:.3f} GB/s)   archive {size[k]} bytes")
    lines.append(f"on / off: time {med['on'] / med['off']:.3f}, archive {size['on'] / size['off']:.4f}")
    lines.append("all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t * 1e3:.2f}" for t in times[k]) for k in order))
    for k in order:
        ctx.profile_enable(2)
        run(k)
        sync()
        table = ctx.profile_table()
        ctx.profile_enable(0)
        total = sum(r["ms"] for r in table)
        lines.append(f"one call with the option {k} under the context's profiler (the calling context's stream; {total:.2f} ms in kernels):")
        for r in sorted(table, key=lambda r: -r["ms"]):
            lines.append(f"  {r['name']:<28s} {r['ms']:9.3f} ms  {100 * r['ms'] / max(total, 1e-9):5.1f} %  launches {r['launches']:5d}")
        first = "k_enc_filters" if k == "on" else "k_enc_wrap"
        ms = sum(r["ms"] for r in table if r["name"] == first)
        lpx = sum(r["ms"] for r in table if r["name"] == "k_enc_lpx")
        lines.append(f"  {first}: {ms:.3f} ms = {100 * ms / med[k]:.1f} % of the call's wall time (k_enc_lpx beside it: {lpx:.3f} ms); on - off = {med['on'] - med['off']:.2f} ms")
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for every workload")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated workload keys (stereo16, text, silesia)")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)       # internal: one workload in a process of its own
    a = ap.parse_args()
    if a.step:
        print(json.dumps(measure(a.step, a.reps)))
        return
    lines = [f"python tools/jam_cli_filters_bench.py --reps {a.reps}" + (f" --only {a.only}" if a.only else ""),
             f"median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise"]
    for key, name in WORKLOADS:
        if a.only and key not in a.only.split(","):
            continue
        lines += ["", f"({key}) {FRAMES} frames of 1 MiB of {name}"]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", key], capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            raise SystemExit(f"{name}: the measuring process ended with {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        lines += json.loads(r.stdout.strip().splitlines()[-1])
    out = "\n".join(lines) + "\n"
    print(out, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
