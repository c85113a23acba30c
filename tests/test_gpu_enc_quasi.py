"""The rANS encoder's middle (ans_enc_model.hip: k_cls_count, k_cls_prefix, k_cls_ord, k_quasi_build; the QuasiModel half of k_pairs in
ans_enc_chain.hip; k_density, k_order and k_sym_layout in ans_enc.hip as far as they move those tables between chunks) on the crafted
inputs of enc_quasi_model, bit-exact against the oracle (which test_oracle_vs_ref.py pins to the reference build).  -m gpu

test_enc_quasi_model.py shows, from the inputs alone, which edges every input reaches -- class totals one short of, at and one past a
rebuild bound, tiles that start there, tiles inside one interval and across nine, a class's only symbol in a tile's first and last slot,
a wave a class skips, an iteration of one class and of all eight, ragged last tiles of 1 and 4095 symbols, the top mantissa of every
alphabet, symbol 256, histograms of one bin, widths of 1, interval 27 of a full chunk -- and which one-token change of the scheme each input
would expose.  Here the kernels code them:
  * the model probe (one slot per byte) on every case, each time BEHIND ITS DECOY on the same context -- the decoy has the case's length
    and classes, so the arena is laid out the same, and every mantissa mirrored, so every table the skip rule leaves out and every bin a
    short clear leaves behind is wrong for the case; symbols and pairs on guarded buffers at odd leads, the pairs buffer exactly 8 rlen
    bytes;
  * the probe's refusal of more than one chunk of symbols: an argument check, no kernel runs;
  * three chunks in the compact layout (class 7 on top, class 2 with zero runs, a short one with every class) through the device and the
    host entry at exact capacity, decoded back -- the reach of each chunk asserted before the GPU is called;
  * sixteen chunks on a context that is alone on its device: graded launch groups, the chunk map not the identity, two chunks tied;
  * eight blocks with different dominant classes through the grouped encode, and once more in reverse order on the same arena;
  * one context that encodes a dense chunk, 27 bytes, the three chunks and the 27 bytes again: the deep call's tables lie where a wrong
    skip rule would read the shallow one's."""
import functools

import numpy as np
import pytest

import enc_quasi_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
LARGE = 100_000
E_ARG = -1


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def _pairs(name, which):
    """the oracle's pairs of a case or of its decoy: computed once, shared, left unchanged"""
    p = _oracle().model_pairs(M.case(name) if which == "case" else M.decoy(name)).astype("<u4")
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _stream(name):
    """the oracle's stream of an image: computed once, shared, left unchanged"""
    want = _oracle().ans_encode(M.image(name))
    want.setflags(write=False)
    return want


def _encode_exact(torch, ctx, t, want, lead, what):
    g_in = Guarded(torch, np.array(t), lead)
    g_out = Guarded(torch, None, 5, cap=len(want))
    assert ctx.ans_encode(g_in.ptr, len(t), g_out.ptr, len(want)) == len(want), what
    g_out.check_output(want, used=len(want), what=what)
    g_in.check_unchanged(what)


def _decode_back(torch, ctx, want, t, what):
    g_s = Guarded(torch, np.array(want), 1)
    g_t = Guarded(torch, None, 7, cap=len(t))
    assert ctx.ans_decode(g_s.ptr, len(want), g_t.ptr, len(t)) == len(t), what
    g_t.check_output(t, what=what)
    g_s.check_unchanged(what)


@pytest.mark.parametrize("name", M.CASES)
def test_pairs_probe_behind_the_decoy(gpu, name):
    torch, jam, ctx = gpu
    n = len(M.case(name))
    for lead16, lead32 in (((2, 4), (14, 12)) if n < LARGE else ((6, 8),)):
        for which in ("decoy", "case"):
            s = M.decoy(name) if which == "decoy" else M.case(name)
            what = f"model_pairs {name} ({which}) symbols at +{lead16} pairs at +{lead32}"
            g_s = Guarded(torch, s.astype("<u2"), lead16)
            g_p = Guarded(torch, None, lead32, cap=8 * n)
            ctx.model_pairs(g_s.ptr, n, g_p.ptr)
            g_p.check_output(_pairs(name, which), what=what)
            g_s.check_unchanged(what)


def test_probe_refuses_more_than_a_chunk(gpu):
    """jpk_dev_model_pairs is a probe of ONE chunk: beyond JPK_ANS_CHUNK symbols a class can outrun the tabulated schedule.  The refusal is
    an argument check -- nothing is launched, the (small) buffers are not looked at"""
    torch, jam, ctx = gpu
    assert jam.CHUNK == M.CHUNK and M.qbound(M.NQ) > M.CHUNK
    g_s = Guarded(torch, np.full(32, 4, dtype="<u2"), 2)
    g_p = Guarded(torch, None, 4, cap=256)
    for rlen in (M.CHUNK + 1, 2 * M.CHUNK, 0x7FFFFFFF):
        with pytest.raises(jam.JampackError) as e:
            ctx.model_pairs(g_s.ptr, rlen, g_p.ptr)
        assert e.value.status == E_ARG, rlen
    g_s.check_unchanged("refused model_pairs")
    g_p.check_unchanged("refused model_pairs")
    ctx.model_pairs(g_s.ptr, 32, g_p.ptr)                                # and the context still works
    g_p.check_output(_oracle().model_pairs(np.full(32, 4, dtype=np.uint16)).astype("<u4"), used=256, what="model_pairs after a refusal")


def test_three_chunks_compact_layout(gpu, oracle):
    torch, jam, ctx = gpu
    img = M.image("three-chunks")
    cs = M.chunks(img)
    assert len(cs) == 3
    for k, c in enumerate(cs):
        ev = M.reach(M.chunk_symbols(oracle, c))
        missing = [e for e in M.IMAGE_REACH["three-chunks"][k] if not ev[e]]
        assert not missing, (k, missing)
    want = _stream("three-chunks")
    _encode_exact(torch, ctx, img, want, 3, "ans_encode three-chunks")
    got = jam.Ans().Encode(np.array(img))
    assert np.array_equal(got, want), f"Ans().Encode three-chunks: {len(got)} vs {len(want)} bytes"
    _decode_back(torch, ctx, want, img, "ans_decode three-chunks")


def test_sixteen_chunks_in_graded_groups(oracle):
    import torch
    import jampack_amd as jam
    img = M.image("sixteen-chunks")
    cs = M.chunks(img)
    dens = [M.density(c) for c in cs]
    order = M.launch_order(dens)
    assert len(cs) == 16 and order != list(range(16)), "the launch order is not the chunk order"
    assert dens[3] == dens[14] and order.index(14) == order.index(3) + 1, "a tie, broken by chunk number"
    assert jam.lib().jpk_debug_enc_groups(0, len(cs)) >= 2, "a block alone on its device with 16 chunks is cut into graded groups"
    want = _stream("sixteen-chunks")
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        _encode_exact(torch, ctx, img, want, 3, "ans_encode sixteen-chunks")
        _decode_back(torch, ctx, want, img, "ans_decode sixteen-chunks")
    finally:
        ctx.close()


def _group(torch, ctx, blocks, want, what):
    g_in = [Guarded(torch, np.array(b), (0, 1, 3, 15)[i % 4]) for i, b in enumerate(blocks)]
    g_out = [Guarded(torch, None, (5, 0, 9, 2)[i % 4], cap=len(w)) for i, w in enumerate(want)]
    n, st = ctx.blocks_compress([g.ptr for g in g_in], [len(b) for b in blocks], [g.ptr for g in g_out], [len(w) for w in want], 2)
    assert st == [0] * len(blocks) and n == [len(w) for w in want], (what, st, n)
    for i, w in enumerate(want):
        g_out[i].check_output(w, used=len(w), what=f"{what} block {i} ({len(blocks[i])} B)")
        g_in[i].check_unchanged(f"{what} input {i}")


def test_group(gpu, oracle):
    torch, jam, ctx = gpu
    blocks = list(M.group())
    assert len(blocks) == 8
    want = [oracle.compress_block(b) for b in blocks]
    _group(torch, ctx, blocks, want, "blocks_compress")
    _group(torch, ctx, blocks[::-1], want[::-1], "blocks_compress, reversed on the same arena")


def test_arena_order_deep_then_shallow(oracle):
    import torch
    import jampack_amd as jam
    dense = M.image("three-chunks")[: M.CHUNK]                           # one chunk, class 7 on top, tables down to interval 20
    short = np.array([(37 * i + 11) % 251 for i in range(27)], dtype=np.uint8)
    texts = (("a dense chunk", dense, oracle.ans_encode(dense)), ("27 bytes", short, oracle.ans_encode(short)),
             ("three-chunks", M.image("three-chunks"), _stream("three-chunks")), ("27 bytes again", short, oracle.ans_encode(short)))
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        for what, t, want in texts:
            _encode_exact(torch, ctx, t, want, 3, f"ans_encode {what} on the context that went deep")
    finally:
        ctx.close()
