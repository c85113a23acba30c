"""Updating a .jam archive resident in HBM (Context.jam_update; DESIGN 4.6, "Updating an archive") against the same result reached through
the entries that were there before it: a whole decode, the overlay of the new bytes, a whole compress and an index of the new archive.

Workload: corpus text as 64 frames of 1 MiB, as a plain archive (kind 0) and as a stock-CLI archive (kind 1).  An update writes 4 KiB
into the middle of 1, 2, 8 and 64 frames, spread evenly over the archive, so every touched frame is decoded, patched and encoded again.
Both paths are checked to give the same archive bytes once; then, after one warm-up of each, they are timed in alternating rounds (every
round starts with the other one), --reps rounds, wall clock with a device synchronise, and the medians and their ratio reported.  It is one
GPU step: run it under a time limit of its own,

  timeout -k 10 900 python tools/jam_update_bench.py [--reps 5] [--kinds 0,1] [--out profiles/jam_update.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1 << 20
FRAMES, BS, PATCH = 64, MiB, 4096
TOUCHED = (1, 2, 8, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch                                            # first: torch brings its own HIP runtime, and the library must share it
    import jampack_amd as jam
    sync = torch.cuda.synchronize
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    n = FRAMES * BS
    d_raw = torch.from_numpy(np.concatenate([jam.corpus.make("text", MiB, 8000 + i) for i in range(FRAMES)])).to("cuda")
    d_new = torch.randint(0, 256, (FRAMES * PATCH,), dtype=torch.uint8, device="cuda")
    lines = ["tools/jam_update_bench.py: archives of corpus text in HBM, 64 frames of 1 MiB; an update writes 4 KiB into the middle of each touched frame",
             f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} alternating rounds after one warm-up, wall clock with a device synchronise",
             "old path: whole decode + overlay + whole compress + index of the result; both paths give the same archive bytes (checked once per case)"]
    for kind in [int(k) for k in a.kinds.split(",")]:
        cli = kind == 1
        bound = (jam.jam_cli_compress_bound if cli else jam.jam_compress_bound)(n, BS)
        d_arch = torch.empty(bound + 64, dtype=torch.uint8, device="cuda")
        compress = ctx.jam_cli_compress if cli else ctx.jam_compress
        alen = compress(d_raw, n, BS, d_arch, bound)
        ix = ctx.jam_cli_index(d_arch, alen) if cli else ctx.jam_index(d_arch, alen)
        assert (ix.frames, ix.raw_len, ix.bad_frame) == (FRAMES, n, -1)
        d_dec = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        d_old, d_upd = torch.empty(bound + 64, dtype=torch.uint8, device="cuda"), torch.empty(bound + 64, dtype=torch.uint8, device="cuda")
        lines.append(f"-- kind {kind} ({'stock-CLI' if cli else 'plain'} frames): archive {alen} bytes, raw {n} bytes")
        for m in TOUCHED:
            frames = [k * (FRAMES // m) for k in range(m)]
            writes = [(f * BS + BS // 2, PATCH, d_new.data_ptr() + i * PATCH) for i, f in enumerate(frames)]
            cap = jam.jam_update_bound(ix, [(o, ln) for o, ln, _ in writes])
            assert cap <= bound + 64
            got = {}

            def run(k):
                if k == "update":
                    ln, nix, rw = ctx.jam_update(ix, d_arch, alen, writes, d_upd, cap, block_size=BS)
                    assert rw == m and nix.frames == FRAMES
                    nix.close()
                    got[k] = ln
                else:
                    res = (ctx.jam_cli_decompress if cli else ctx.jam_decompress)(d_arch, alen, d_dec, n)
                    assert res[0] == n
                    for i, f in enumerate(frames):
                        d_dec[f * BS + BS // 2: f * BS + BS // 2 + PATCH] = d_new[i * PATCH: (i + 1) * PATCH]
                    ln = compress(d_dec, n, BS, d_old, bound)
                    jx = ctx.jam_cli_index(d_old, ln) if cli else ctx.jam_index(d_old, ln)
                    assert jx.frames == FRAMES
                    jx.close()
                    got[k] = ln

            for k in ("update", "old"):                     # warm-up: arenas, scratch, code objects; and the two results are one
                run(k)
            sync()
            assert got["update"] == got["old"] and torch.equal(d_upd[: got["update"]], d_old[: got["old"]]), (kind, m)
            times = {"update": [], "old": []}
            for r in range(a.reps):
                for k in (("update", "old") if r % 2 == 0 else ("old", "update")):
                    sync()
                    t0 = time.perf_counter()
                    run(k)
                    sync()
                    times[k].append((time.perf_counter() - t0) * 1e3)
            mu, mo = float(np.median(times["update"])), float(np.median(times["old"]))
            lines += [f"kind {kind}, {m:2d} of {FRAMES} frames touched: jam_update {mu:9.2f} ms   old path {mo:9.2f} ms   old / update = {mo / mu:6.2f}",
                      "    all rounds (ms): " + "; ".join(f"{k} " + " ".join(f"{t:.2f}" for t in v) for k, v in times.items())]
        ix.close()
        del d_arch, d_dec, d_old, d_upd
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
