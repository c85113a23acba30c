"""The rANS encoder's front (ans_enc_front.hip: k_enc_hist, k_enc_prep, k_enc_mtf; k_rle_lz, k_rle_ext, k_rle_tiles, k_tile_prefix) on the
crafted inputs of enc_front_model, bit-exact against the oracle (which test_oracle_vs_ref.py pins to the reference build).  -m gpu

test_enc_front_model.py shows, from the inputs alone, which arms every input reaches -- ranks found in each of the four list registers,
at both ends of each, first occurrences with 63, 64, 128, 192 and 255 symbols in the list, in tile 0 and from the stamps of a later tile,
tiles that start 64 deep or deeper and tiles that start inside a run, across a wave's and a block's edge, partial last groups, a tile of
one byte, frequency ties; zero runs over thread segments, over one and three whole tiles, to the chunk's end, of every length 2^k - 1,
2^k, 2^k + 1 -- and which one-token change of the scheme each input would expose.  Here the kernels encode them, all on guarded buffers:
  * the rank probe, in place, the text 0, 1, 3 and 15 bytes behind an aligned address, the frequency table 4 bytes off a 16-byte
    boundary; the ranks decoded back by the rank decoder;
  * the RLE0 probe on byte arrays 0, 1, 7 and 15 bytes behind an aligned address, the symbols 2 bytes off, the guard directly behind
    the rlen symbols;
  * the product path on two-chunk images at exact capacity (a chunk that ends in whole tiles of zeros, a second chunk of one byte and
    of 4097, a round robin of 193 across the chunk's edge), decoded back;
  * twelve small blocks through the grouped encode (the clen / cmap form of the same kernels), and once more in reverse order on the
    same context's arena;
  * the host entry."""
import functools

import numpy as np
import pytest

import enc_front_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
TEXT_LEADS = (0, 1, 3, 15)
RANK_LEADS = (0, 1, 7, 15)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _ranks_of(name):
    """(R, freq) of a text from the oracle: computed once, shared, left unchanged"""
    from oracle.pyoracle import Oracle
    r, f = Oracle().rank_encode(M.case(name))
    f = f.astype("<i4")
    r.setflags(write=False)
    f.setflags(write=False)
    return r, f


@pytest.mark.parametrize("name", M.CASES)
def test_rank_probe_in_place(gpu, name):
    torch, jam, ctx = gpu
    t = M.case(name)
    r, f = _ranks_of(name)
    for lead in TEXT_LEADS:
        what = f"rank_encode {name} lead={lead}"
        g_t = Guarded(torch, np.array(t), lead)
        g_f = Guarded(torch, None, 4, cap=1024)                          # int32[256]: 4-byte aligned, off the 16-byte boundary
        ctx.rank_encode(g_t.ptr, g_f.ptr, len(t))
        g_t.check_output(r, what=what)
        g_f.check_output(f, what=what + " freq")
    ctx.rank_decode(g_t.ptr, g_f.ptr, len(t))                            # and back, on the encoder's own output
    g_t.check_output(t, what=f"rank_decode {name}")
    g_f.check_output(f, what=f"rank_decode {name} freq")


@pytest.mark.parametrize("name", M.RANKS)
def test_rle_probe(gpu, oracle, name):
    torch, jam, ctx = gpu
    r = M.ranks(name)
    want = oracle.rle_encode(r).astype("<u2")
    for lead in RANK_LEADS:
        what = f"rle_encode {name} lead={lead}"
        g_r = Guarded(torch, np.array(r), lead)
        g_s = Guarded(torch, None, 2, cap=2 * len(want))                 # the guard stands directly behind rlen symbols
        assert ctx.rle_encode(g_r.ptr, len(r), g_s.ptr) == len(want), what
        g_s.check_output(want, what=what)
        g_r.check_unchanged(what)


@pytest.mark.parametrize("name", M.IMAGES)
def test_two_chunk_images_at_exact_capacity(gpu, oracle, name):
    torch, jam, ctx = gpu
    img = M.image(name)
    assert jam.CHUNK == M.CHUNK < len(img) <= M.CHUNK + M.ATILE + 1
    want = oracle.ans_encode(img)
    what = f"ans_encode {name}"
    g_in = Guarded(torch, np.array(img), 3)
    g_out = Guarded(torch, None, 5, cap=len(want))
    assert ctx.ans_encode(g_in.ptr, len(img), g_out.ptr, len(want)) == len(want), what
    g_out.check_output(want, used=len(want), what=what)
    g_in.check_unchanged(what)
    g_s = Guarded(torch, np.array(want), 1)
    g_t = Guarded(torch, None, 7, cap=len(img))
    assert ctx.ans_decode(g_s.ptr, len(want), g_t.ptr, len(img)) == len(img), name
    g_t.check_output(img, what=f"ans_decode {name}")
    g_s.check_unchanged(f"ans_decode {name}")


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
    assert jam.TRAILER == M.TRAILER and len(blocks) == 12
    want = [oracle.ans_encode(oracle.bwt_forward(b)) for b in blocks]
    _group(torch, ctx, blocks, want, "blocks_compress")
    _group(torch, ctx, blocks[::-1], want[::-1], "blocks_compress, reversed on the same arena")


@pytest.mark.parametrize("name", ["rr-193", "staircase", "runs-at-edges-long"])
def test_host_entry(gpu, name):
    torch, jam, ctx = gpu
    r, f = _ranks_of(name)
    got_r, got_f = jam.Postcoder().Encode(np.array(M.case(name)))
    assert np.array_equal(got_r, r) and np.array_equal(np.asarray(got_f, dtype="<i4"), f), name
