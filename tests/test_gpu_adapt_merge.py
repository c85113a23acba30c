"""The adaptive-model kernels write a segment from its merge point and re-walk only the prefix (k_adapt_a / tab / b / c).  -m gpu

Inputs: the crafted streams of adapt_segment_model, which test_adapt_segment_model.py shows to reach every kind of segment (exact
from the start, merged, plateau lane merged behind a quiet stretch, identity, table) and every residue of the merge step mod 16;
stream lengths whose last segment has 1, 15, 16, 17 items, is shorter than a warm-up, or is a whole segment; and two chunks through
the full encoder (the compact symbol layout -- ctx.model_pairs runs one chunk in the one-slot-per-byte layout).  Every (low, freq)
word, every byte, must equal the sequential reference's."""
import numpy as np
import pytest

import adapt_segment_model as M

pytestmark = pytest.mark.gpu

SEED = 3


@pytest.fixture(scope="module")
def ctx():
    import torch
    from jampack_amd import Context
    c = Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _pairs_equal(ctx, oracle, s, what):
    import torch
    s = np.ascontiguousarray(s, dtype=np.uint16)
    exp = oracle.model_pairs(s)
    d_s = torch.from_numpy(s.view(np.int16)).cuda()
    d_p = torch.zeros(2 * len(s), dtype=torch.int32, device="cuda")
    ctx.model_pairs(d_s, len(s), d_p)
    got = d_p.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} mismatches, first at pair words {bad[:6]} got {got[bad[:3]]} exp {exp[bad[:3]]}"


@pytest.mark.parametrize("which", [1, 2])
def test_model_pairs_on_the_crafted_streams(ctx, oracle, which):
    _pairs_equal(ctx, oracle, {1: M.stream1, 2: M.stream2}[which](SEED), f"stream {which}")


@pytest.mark.parametrize("n", [4096, 4097, 4111, 4112, 4113, 4416, 8192, 8193])
def test_model_pairs_at_segment_edges(ctx, oracle, n):
    _pairs_equal(ctx, oracle, M.mixed(np.random.default_rng(SEED), n), f"mixed({n})")


@pytest.mark.parametrize("kind", ["text", "geometric"])
def test_ans_encode_two_chunks_compact_layout(oracle, kind):
    import jampack_amd as jam
    img = oracle.bwt_forward(jam.corpus.make(kind, (1 << 20) + 4097, 24))
    got = jam.Ans().Encode(img)
    exp = oracle.ans_encode(img.copy())
    n = min(len(got), len(exp))
    d = np.nonzero(got[:n] != exp[:n])[0]
    assert len(got) == len(exp) and d.size == 0, f"{kind}: len {len(got)} vs {len(exp)}, first diff at {d[:4].tolist()} of {d.size}"
