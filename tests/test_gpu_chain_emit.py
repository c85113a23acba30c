"""The rANS encoder's back half (ans_enc_chain.hip: k_pairs' record and padding writes, k_rans_lanes, k_emit_count, k_emit_prefix,
k_put_payload) on the crafted inputs of chain_emit_model, bit-exact against the oracle (which test_oracle_vs_ref.py pins to the reference
build).  -m gpu

test_chain_emit_model.py shows, from the inputs alone, which index edges every input reaches -- chains padded by 0, 255 and 256 identity
steps, chains of unequal length, np at, one symbol past and one symbol short of whole emit tiles, tiles that emit nothing, 64 / 65 / 129 /
512 tiles for k_emit_prefix's windows, two-byte emits at both ends of a mask word, of a thread's sixteen pairs and of a tile, every
symbol a byte of a full chunk -- and which one-token changes of the scheme each input would expose.  Here the kernels encode them:
  * every case through ctx.ans_encode on guarded buffers at exact capacity, the input 0, 1, 3 and 15 bytes behind an aligned address (one
    lead for the cases above 100 000 symbols), the input unchanged, and the stream decoded back;
  * the model probe (one slot per byte: the other layout of the record arrays) on the same RLE0 streams, the pairs buffer guarded;
  * two-chunk images in the compact layout, whose second chunk's record prefetches read the first chunk's chains, through the device
    and the host entry -- the reach of each chunk asserted before the GPU is called;
  * eight small blocks through the grouped encode, and once more with one capacity a byte short: that block alone reports it;
  * one context that encodes a full chunk, one symbol, 131 073 and 512 symbols in this order: the arena grows and then shrinks in use, and
    the larger chunk's masks and states lie behind the smaller one's."""
import functools

import numpy as np
import pytest

import chain_emit_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
LEADS = (0, 1, 3, 15)
LARGE = 100_000
E_CAPACITY = -2


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _expect(name):
    """the oracle's stream of a case or image: computed once, shared, left unchanged"""
    from oracle.pyoracle import Oracle
    want = Oracle().ans_encode(M.case(name) if name in M.CASES else M.image(name))
    want.setflags(write=False)
    return want


def _encode_exact(torch, ctx, t, want, lead, what):
    g_in = Guarded(torch, np.array(t), lead)
    g_out = Guarded(torch, None, 5, cap=len(want))
    assert ctx.ans_encode(g_in.ptr, len(t), g_out.ptr, len(want)) == len(want), what
    g_out.check_output(want, used=len(want), what=what)
    g_in.check_unchanged(what)


@pytest.mark.parametrize("name", M.CASES)
def test_single_cases(gpu, name):
    torch, jam, ctx = gpu
    t, want = M.case(name), _expect(name)
    for lead in (LEADS if len(t) < LARGE else (3,)):
        _encode_exact(torch, ctx, t, want, lead, f"ans_encode {name} lead={lead}")
    g_s = Guarded(torch, np.array(want), 1)
    g_t = Guarded(torch, None, 7, cap=len(t))
    assert ctx.ans_decode(g_s.ptr, len(want), g_t.ptr, len(t)) == len(t), name
    g_t.check_output(t, what=f"ans_decode {name}")
    g_s.check_unchanged(f"ans_decode {name}")


@pytest.mark.parametrize("name", M.CASES)
def test_pairs_probe(gpu, oracle, name):
    """one chunk in the one-slot-per-byte layout; k_pairs' pad writes go past the chunk's 2 rlen records, the pairs buffer holds exactly
    2 rlen words"""
    torch, jam, ctx = gpu
    _, s, pairs = M.chunk_pairs(oracle, M.case(name))
    for lead16, lead32 in (((2, 4), (14, 12)) if len(s) < LARGE else ((6, 8),)):
        what = f"model_pairs {name} symbols at +{lead16} pairs at +{lead32}"
        g_s = Guarded(torch, s.astype("<u2"), lead16)
        g_p = Guarded(torch, None, lead32, cap=8 * len(s))
        ctx.model_pairs(g_s.ptr, len(s), g_p.ptr)
        g_p.check_output(pairs.astype("<u4"), what=what)
        g_s.check_unchanged(what)


@pytest.mark.parametrize("name", M.IMAGES)
def test_two_chunk_images(gpu, oracle, name):
    torch, jam, ctx = gpu
    img = M.image(name)
    assert jam.CHUNK == M.CHUNK < len(img) < 2 * M.CHUNK
    for k, c in enumerate(M.chunks(img)):
        _, s, pairs = M.chunk_pairs(oracle, c)
        assert len(s) == M.IMAGE_SPECS[name][2 + k]
        ev = M.reach(pairs)
        missing = [e for e in M.IMAGE_REACH[name][k] if not ev[e]]
        assert not missing, (name, k, missing)
    want = _expect(name)
    _encode_exact(torch, ctx, img, want, 3, f"ans_encode {name}")
    got = jam.Ans().Encode(np.array(img))
    assert np.array_equal(got, want), f"Ans().Encode {name}: {len(got)} vs {len(want)} bytes"


def _group(torch, ctx, blocks, caps):
    g_in = [Guarded(torch, np.array(b), (0, 1, 3, 15)[i % 4]) for i, b in enumerate(blocks)]
    g_out = [Guarded(torch, None, (5, 0, 9, 2)[i % 4], cap=c) for i, c in enumerate(caps)]
    n, st = ctx.blocks_compress([g.ptr for g in g_in], [len(b) for b in blocks], [g.ptr for g in g_out], list(caps))
    for i, g in enumerate(g_in):
        g.check_unchanged(f"blocks_compress input {i}")
    return n, st, g_out


def test_group(gpu, oracle):
    torch, jam, ctx = gpu
    blocks = M.group()
    want = [oracle.compress_block(b) for b in blocks]
    n, st, g_out = _group(torch, ctx, blocks, [len(w) for w in want])
    assert st == [0] * len(blocks) and n == [len(w) for w in want]
    for i, w in enumerate(want):
        g_out[i].check_output(w, used=len(w), what=f"blocks_compress block {i} ({len(blocks[i])} B)")
    # one capacity a byte short: that block alone says so and nothing of it is written; the others are exact
    short = 4                                                          # the block whose image has rlen 1535
    assert M.GROUP_RLENS[len(blocks[short])] == 1535
    caps = [len(w) - (i == short) for i, w in enumerate(want)]
    n, st, g_out = _group(torch, ctx, blocks, caps)
    assert st == [E_CAPACITY if i == short else 0 for i in range(len(blocks))], st
    for i, w in enumerate(want):
        if i == short:
            g_out[i].check_output(np.zeros(0, np.uint8), used=0, what="blocks_compress: the block that does not fit")
        else:
            assert n[i] == len(w)
            g_out[i].check_output(w, used=len(w), what=f"blocks_compress block {i} beside the short one")


def test_arena_grows_and_shrinks_in_use():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        for name in ("full-chunk", "norep-1", "norep-131073", "norep-512"):
            _encode_exact(torch, ctx, M.case(name), _expect(name), 3, f"ans_encode {name} on the context that grew")
    finally:
        ctx.close()
