"""jpk_dev_blocks_decompress of MANY SMALL blocks (>= 32 blocks of <= 4 MiB): the inverse BWTs of all of them go through one set of launches
(bwt_inv.hip jpk_inv_bwt_batch_enqueue: blockIdx.y = the block, one shared tile table and scan).  Every block must come back as the
reference's InverseBwt gives it (bwt.cpp:72-282), whatever the mix of sizes, and a block whose image is corrupt must fail alone.
JPK_INV_BATCH=0 (the lanes of per-block launches) must give the same bytes.  -m gpu"""
import os
import subprocess
import sys

import numpy as np
import pytest

import inv_walk_model

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


def _mixed_blocks(jam, seed, count):
    rng = np.random.default_rng(seed)
    kinds = ["text_survey", "text", "zero", "runs", "dna", "random", "two", "repeat4k", "geometric", "samples16"]
    sizes = [0, 1, 119, 120, 121, 239, 240, 4096, 65_537, 300_000, MiB - 1, MiB, MiB + 1, 2 * MiB + 77, 3 * MiB + 119, 4 * MiB]
    blocks = []
    for i in range(count):
        n = sizes[i] if i < len(sizes) else int(rng.choice(sizes + [int(rng.integers(1, 2 * MiB))]))
        blocks.append(jam.corpus.make(kinds[int(rng.integers(len(kinds)))], n, 500 * seed + i))
    return blocks


def _compress_each(torch, jam, ctx, blocks):
    dev = torch.device("cuda", 0)
    d_in = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) if len(b) else torch.empty(1, dtype=torch.uint8, device=dev) for b in blocks]
    caps = [jam.ans_capacity(len(b) + jam.TRAILER) for b in blocks]
    d_out = [torch.empty(c, dtype=torch.uint8, device=dev) for c in caps]
    n, st = ctx.blocks_compress(d_in, [len(b) for b in blocks], d_out, caps, 4)
    assert st == [0] * len(blocks)
    return [d_out[i][: n[i]] for i in range(len(blocks))], n


@pytest.mark.parametrize("seed", [1, 2])
def test_mixed_small_blocks_come_back(gpu, seed):
    torch, jam, ctx = gpu
    dev = torch.device("cuda", 0)
    blocks = _mixed_blocks(jam, seed, 60)
    comp, n = _compress_each(torch, jam, ctx, blocks)
    backs = [torch.empty(max(len(b), 1), dtype=torch.uint8, device=dev) for b in blocks]
    bn, st = ctx.blocks_decompress(comp, n, backs, [len(b) for b in blocks])
    assert st == [0] * len(blocks)
    for i, b in enumerate(blocks):
        assert bn[i] == len(b) and np.array_equal(backs[i][: len(b)].cpu().numpy(), b), (i, len(b))


def test_a_corrupt_image_fails_alone(gpu, oracle):
    """valid Ans streams of BWT images whose trailer index is 0 / beyond the block / names a chain that does not cover the block: those
    blocks report JPK_E_CORRUPT, every other block of the batch is returned"""
    torch, jam, ctx = gpu
    dev = torch.device("cuda", 0)
    blocks = [jam.corpus.make("text_survey", 200_000 + 1000 * i, 40 + i) for i in range(40)]
    streams = []
    bad = {3: "zero", 17: "beyond", 29: "other"}
    for i, b in enumerate(blocks):
        img = oracle.bwt_forward(b).copy()
        nl = len(b) - len(b) % 120
        tr = img[len(b):].view("<i4")
        if bad.get(i) == "zero":
            tr[0] = 0
        elif bad.get(i) == "beyond":
            tr[0] = nl + 5
        elif bad.get(i) == "other":
            img[1000], img[1001] = img[1001] ^ 0x55, img[1000] ^ 0x2A        # another multiset of bytes: the chain from trailer[0] closes early or not at all
            verdict29, text29 = inv_walk_model.verdict(img)                  # the Map is a permutation whatever the bytes: a short head path, or another text
        streams.append(oracle.ans_encode(img))
    d_c = [torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in streams]
    backs = [torch.empty(len(b), dtype=torch.uint8, device=dev) for b in blocks]
    bn, st = ctx.blocks_decompress(d_c, [len(s) for s in streams], backs, [len(b) for b in blocks])
    for i, b in enumerate(blocks):
        if i in (3, 17):
            assert st[i] == -3 and bn[i] == 0, (i, st[i])
        elif i == 29:                                                        # what inv_walk_model predicts for this exact image
            assert st[i] == verdict29["status"], (st[i], verdict29)
            if st[i] == 0:
                assert bn[i] == len(b) and backs[i].cpu().numpy().tobytes() == text29 != b.tobytes()
            else:
                assert bn[i] == 0
        else:
            assert st[i] == 0 and bn[i] == len(b) and np.array_equal(backs[i].cpu().numpy(), b), i


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
import jampack_amd as jam
dev = torch.device("cuda", 0)
ctx = jam.Context(0, None)
blocks = [jam.corpus.make(["text_survey", "dna", "runs", "random"][i %% 4], 100_000 + 37_001 * i, i) for i in range(36)]
d_in = [torch.from_numpy(b).to(dev) for b in blocks]
caps = [jam.ans_capacity(len(b) + jam.TRAILER) for b in blocks]
d_out = [torch.empty(c, dtype=torch.uint8, device=dev) for c in caps]
n, st = ctx.blocks_compress(d_in, [len(b) for b in blocks], d_out, caps, 4)
backs = [torch.empty(len(b), dtype=torch.uint8, device=dev) for b in blocks]
bn, st2 = ctx.blocks_decompress([d_out[i][: n[i]] for i in range(36)], n, backs, [len(b) for b in blocks])
ok = st == [0] * 36 and st2 == [0] * 36 and all(bn[i] == len(b) and np.array_equal(backs[i].cpu().numpy(), b) for i, b in enumerate(blocks))
print("LANES_OK" if ok else "LANES_BAD")
"""


def test_per_block_launches_remain_a_working_comparator():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, JPK_INV_BATCH="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % root], env=env, capture_output=True, text=True, timeout=600)
    assert "LANES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
