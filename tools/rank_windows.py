#!/usr/bin/env python3
"""window lengths of k_enc_mtf's rank count on the BWT image of the bench's first block (64 MiB of the default workload, 4 KiB tiles):
for every run head the number of heads between it and the previous head of its symbol in the tile -- what decides how many window
positions a head's own lane should test (RW_CAP, ans_enc_front.hip) and how many steps of 64 the wave spends on the rest.
    python tools/rank_windows.py [workload]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import jampack_amd as jam
from jampack_amd import corpus

ATILE = 4096
workload = sys.argv[1] if len(sys.argv) > 1 else "enwik8"
data, source = corpus.load_or_make(workload)
block = corpus.split_blocks(data, 64 << 20)[0]
n = len(block)
dev = torch.device("cuda", 0)
ctx = jam.Context(0, None)
d_bwt = torch.empty(n + jam.TRAILER, dtype=torch.uint8, device=dev)
ctx.bwt_forward(torch.from_numpy(np.ascontiguousarray(block)).to(dev), n, d_bwt, n + jam.TRAILER)
torch.cuda.synchronize()
B = d_bwt.cpu().numpy()
ctx.close()

i = np.arange(len(B))
head = np.ones(len(B), dtype=bool)
head[1:] = B[1:] != B[:-1]
head |= i % ATILE == 0
hp = np.flatnonzero(head)
hs = B[hp].astype(np.int64)
ht = hp // ATILE
first_of_tile = np.searchsorted(ht, np.arange(ht[-1] + 1))
k = np.arange(len(hp)) - first_of_tile[ht]
order = np.argsort(ht * 256 + hs, kind="stable")
same = (ht[order][1:] == ht[order][:-1]) & (hs[order][1:] == hs[order][:-1])
win = (k[order][1:] - k[order][:-1] - 1)[same]                 # heads with a previous head of their symbol in the tile
nfirst = len(hp) - len(win)
tiles = int(ht[-1]) + 1
print(f"# {workload} ({source}), block 0: {n} bytes, image {len(B)} bytes, {tiles} tiles")
print(f"heads {len(hp)} = {len(hp) / len(B):.3f} per byte, {len(hp) / tiles:.0f} per tile; first heads (no earlier head of the symbol in the tile) "
      f"{nfirst} = {nfirst / tiles:.1f} per tile")
print("window = heads between a head and its symbol's previous head in the tile:")
print("  " + "  ".join(f"{q} % {int(np.percentile(win, q))}" for q in (25, 50, 75, 90, 95, 99)) + f"  max {int(win.max())}  mean {win.mean():.1f}")
for cap in (8, 16, 24, 32, 64):
    rest = win[win > cap] - cap
    steps = (rest + 63) // 64
    print(f"  own-lane positions {cap:2d}: {100 * len(rest) / len(win):5.1f} % of the heads go on, {steps.mean():.2f} steps of 64 each, "
          f"{steps.sum() / tiles:.0f} steps per tile")
