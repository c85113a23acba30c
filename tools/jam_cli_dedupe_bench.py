"""The dedupe option of the stock-CLI writer ("Dedupe") against the same call without it, which is the writer as it was:

  off  Context.jam_cli_compress(..., dedupe=False)   jpk_dev_jam_cli_compress_ex, flags = 0
  on   Context.jam_cli_compress(..., dedupe=True)    flags = JPK_CLI_DEDUPE: the k_dd_* launches in front of k_enc_wrap

Workloads: (a) 64 frames of 1 MiB and 16 frames of 8 MiB of corpus text -- nothing to find: the price of the option; (b) the first 100 MB
of this image's source and text files (corpus.system_sources, what tools/real_files.py writes; near-duplicate files, licence headers) as
frames of 64 MiB.  Per workload, with the option off and on: archive size, GB/s (median of --reps alternating rounds after one warm-up,
wall clock with a device synchronise), the per-kernel table of one profiled call, and for the first block sa_rounds and the time of
jpk_dev_bwt_forward on what the stage chain makes of it.  Every workload runs in a process of its own under a time limit (--limit
seconds); the first that fails or runs out of time ends the tool.

  python tools/jam_cli_dedupe_bench.py [--reps 5] [--limit 240] [--out profiles/jam_cli_dedupe.txt]
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
WORKLOADS = (("a1", "64 frames of 1 MiB of corpus text", MiB), ("a8", "16 frames of 8 MiB of corpus text", 8 * MiB),
             ("b", "100 MB of this image's source files, frames of 64 MiB", 64 * MiB))
DD = ("k_dd_anchor", "k_dd_cand", "k_dd_extend", "k_dd_select", "k_dd_emit")


def load(jam, key, bs):
    if key == "b":
        a = jam.corpus.system_sources(100_000_000)
        if a is None:
            raise SystemExit("the source trees hold less than 100 MB")
        return a
    return np.concatenate([jam.corpus.make("text", bs, 8000 + i) for i in range(64 * MiB // bs)])


def measure(key, bs, reps):
    import torch
    import jampack_amd as jam
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    data = load(jam, key, bs)
    n = len(data)
    frames = -(-n // bs)
    d_in = torch.from_numpy(data).to(dev)
    cap = jam.jam_cli_compress_bound(n, bs)
    d_out = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    d_back = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    size = {}

    def run(k):
        size[k] = ctx.jam_cli_compress(d_in, n, bs, d_out, cap, dedupe=(k == "on"))

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
    lines = [f"device: {torch.cuda.get_device_name(0)}; raw {n} bytes, {frames} frames"]
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
        if k == "on":
            ms = sum(r["ms"] for r in table if r["name"] in DD)
            lines.append(f"  k_dd_*: {ms:.3f} ms = {100 * ms / med['on']:.1f} % of the call's wall time; on - off = {med['on'] - med['off']:.2f} ms")
    # the first block alone: what the BWT is given, its rounds and its time
    m = min(bs, n)
    s4cap = jam.cli_stages_bound(m)
    d_s4 = torch.empty(s4cap + 64, dtype=torch.uint8, device=dev)
    d_img = torch.empty(s4cap + 480 + 64, dtype=torch.uint8, device=dev)
    for k in order:
        (ln,), (st,) = ctx.blocks_cli_stages_encode([d_in], [m], [d_s4], [s4cap], dedupe=(k == "on"))
        assert st == 0
        ctx.bwt_forward(d_s4, ln, d_img, s4cap + 480)
        sync()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.bwt_forward(d_s4, ln, d_img, s4cap + 480)
            sync()
            ts.append(time.perf_counter() - t0)
        lines.append(f"first block, option {k}: BWT input {ln} bytes of {m}, sa_rounds {ctx.stats().sa_rounds}, jpk_dev_bwt_forward {np.median(ts) * 1e3:.2f} ms")
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for every workload")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated workload keys (a1, a8, b)")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)       # internal: one workload in a process of its own
    a = ap.parse_args()
    if a.step:
        key, bs = a.step.split(":")
        print(json.dumps(measure(key, int(bs), a.reps)))
        return
    lines = [f"python tools/jam_cli_dedupe_bench.py --reps {a.reps}" + (f" --only {a.only}" if a.only else ""),
             f"median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise"]
    for key, name, bs in WORKLOADS:
        if a.only and key not in a.only.split(","):
            continue
        lines += ["", f"({key}) {name}, block_size {bs // MiB} MiB"]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", f"{key}:{bs}"], capture_output=True, text=True,
                           timeout=a.limit)
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
