"""Whole .jam archives against the engines under them, on the same blocks:

  archive    jpk_dev_jam_compress / jpk_dev_jam_decompress: one call for the whole archive
  bare       jpk_dev_blocks_compress / jpk_dev_blocks_decompress on the same slices (payloads only: no crc, no frames)
  per-frame  the jpk_dev_jam_block_write / jpk_dev_jam_block_read loop, one frame at a time

Every call ends in a device synchronise and every output is compared (archive bytes = the per-frame loop's bytes; payloads = the
archive's payloads; decoded bytes = the input).  Workloads: 1 GiB of corpus text, one seed per block, as 8 MiB and as 64 MiB frames
(a repeated buffer would hit the sort's deep-repeat cliff).  Rates are input (raw) bytes per second, best of --reps calls.

  python tools/jam_archive_bench.py [--gib 1] [--frames-mib 8 64] [--reps 3] [--out profiles/jam_archive_bench.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1 << 20


def _block(args):
    from jampack_amd import corpus
    n, seed = args
    return corpus.make("text", n, seed)


def make_input(total, bs, seed0):
    sizes = [min(bs, total - o) for o in range(0, total, bs)]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return np.concatenate(list(ex.map(_block, [(n, seed0 + i) for i, n in enumerate(sizes)])))


def best_of(reps, fn, sync):
    ts, r = [], None
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts)), r


def run(torch, jam, ctx, data, bs, reps):
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    n = len(data)
    nb = (n + bs - 1) // bs
    d_in = torch.from_numpy(data).to(dev)
    lens = [min(bs, n - b * bs) for b in range(nb)]
    ins = [d_in.data_ptr() + b * bs for b in range(nb)]
    gb = n / 1e9
    res = {"frames_mib": bs // MiB, "frames": nb, "raw_bytes": n}

    # ---- compress ----
    bound = jam.jam_compress_bound(n, bs)
    d_arch = torch.empty(bound, dtype=torch.uint8, device=dev)
    t, tm, m = best_of(reps, lambda: ctx.jam_compress(d_in.data_ptr(), n, bs, d_arch.data_ptr(), bound), sync)
    res["archive_compress_gbs"], res["archive_compress_median_gbs"], res["archive_bytes"] = gb / t, gb / tm, m
    arch = d_arch[:m].cpu().numpy()

    cap = jam.ans_capacity(bs + jam.TRAILER)
    slots = torch.empty(nb * cap, dtype=torch.uint8, device=dev)
    outs = [slots.data_ptr() + b * cap for b in range(nb)]
    t, tm, (ol, st) = best_of(reps, lambda: ctx.blocks_compress(ins, lens, outs, [cap] * nb), sync)
    assert st == [0] * nb
    res["bare_compress_gbs"], res["bare_compress_median_gbs"] = gb / t, gb / tm
    starts, o = [], 0
    while o < len(arch):
        starts.append(o)
        o += 15 + int(np.frombuffer(arch[o + 7: o + 11].tobytes(), dtype="<i4")[0])
    host_slots = slots.cpu().numpy()
    for b in range(nb):                                  # the bare payloads are the archive's payloads
        assert np.array_equal(host_slots[b * cap: b * cap + ol[b]], arch[starts[b] + 15: starts[b] + 15 + ol[b]]), b

    fcap = 15 + cap
    d_frames = torch.empty(nb * fcap, dtype=torch.uint8, device=dev)

    def frame_loop():
        return [ctx.jam_block_write(ins[b], lens[b], bs, d_frames.data_ptr() + b * fcap, fcap) for b in range(nb)]
    t, tm, fl = best_of(reps, frame_loop, sync)
    res["per_frame_compress_gbs"], res["per_frame_compress_median_gbs"] = gb / t, gb / tm
    hf = d_frames.cpu().numpy()
    assert np.array_equal(np.concatenate([hf[b * fcap: b * fcap + fl[b]] for b in range(nb)]), arch)

    # ---- decompress ----
    d_back = torch.empty(n, dtype=torch.uint8, device=dev)
    t, tm, r = best_of(reps, lambda: ctx.jam_decompress(d_arch.data_ptr(), m, d_back.data_ptr(), n), sync)
    assert r == (n, nb, -1) and torch.equal(d_back, d_in)
    res["archive_decompress_gbs"], res["archive_decompress_median_gbs"] = gb / t, gb / tm

    d_back.zero_()
    outs_b = [d_back.data_ptr() + b * bs for b in range(nb)]
    pay = [d_arch.data_ptr() + s + 15 for s in starts]
    t, tm, (ol2, st2) = best_of(reps, lambda: ctx.blocks_decompress(pay, ol, outs_b, lens), sync)
    assert st2 == [0] * nb and ol2 == lens and torch.equal(d_back, d_in)
    res["bare_decompress_gbs"], res["bare_decompress_median_gbs"] = gb / t, gb / tm

    d_back.zero_()

    def read_loop():
        return [ctx.jam_block_read(d_arch.data_ptr() + starts[b], m - starts[b], outs_b[b], lens[b]) for b in range(nb)]
    t, tm, rl = best_of(reps, read_loop, sync)
    assert [x[0] for x in rl] == lens and torch.equal(d_back, d_in)
    res["per_frame_decompress_gbs"], res["per_frame_decompress_median_gbs"] = gb / t, gb / tm
    res["archive_vs_bare_compress"] = res["archive_compress_gbs"] / res["bare_compress_gbs"]
    res["archive_vs_bare_decompress"] = res["archive_decompress_gbs"] / res["bare_decompress_gbs"]
    res["archive_vs_per_frame_compress"] = res["archive_compress_gbs"] / res["per_frame_compress_gbs"]
    res["archive_vs_per_frame_decompress"] = res["archive_decompress_gbs"] / res["per_frame_decompress_gbs"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--frames-mib", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    total = int(a.gib * (1 << 30))
    rows = []
    for fm in a.frames_mib:
        data = make_input(total, fm * MiB, a.seed)
        row = run(torch, jam, ctx, data, fm * MiB, a.reps)
        row["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/jam_archive_bench.py", "gib": a.gib, "reps": a.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
