"""k_enc_mtf's window scheme (ans_enc_front.hip: the rank of every run head counted in its own window, no serial list walk) on the inputs of
rank_window_model, byte for byte against the oracle's ranks and Freq[] (test_oracle_vs_ref.py pins the oracle to the reference build).  -m gpu

test_rank_window_model.py shows on the CPU that the scheme gives a plain one-list MTF's ranks on these inputs and that they reach what
they are named for.  Here jpk_rank_encode runs them, on guarded buffers (a store outside the n bytes shows):
  * lengths 1, 63, 64, 65, 4095, 4096, 4097, 8193;
  * one symbol only; two alternating symbols (every byte a head, every window 1);
  * bytes 0..255 cycling over five tiles (every rank 255, every window 255: four steps of 64, windows across tile edges);
  * 256 symbols brought in in tile 0, tile 2 opening with all of them in reverse order (first heads, ranked from the carried stamps);
  * a symbol seen once in tile 0 and again at the last byte of tile 3;
  * a tile of 4096 heads and no repeats (i * 7 mod 256); random bytes over three tiles;
  * runs crossing tile edges, the edge 3|4 among them (a tile's first byte continues a run);
  * 64 KiB of BWT-like text;
  * 1 MiB + 4097 bytes of BWT-like text: as one buffer through jpk_rank_encode (257 tiles), and as two chunks through the product path,
    where the stamps restart, against the oracle's stream."""
import functools

import numpy as np
import pytest

import rank_window_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu


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


def _rank_encode(torch, ctx, name, lead):
    t = M.case(name)
    r, f = _ranks_of(name)
    what = f"rank_encode {name} lead={lead}"
    g_t = Guarded(torch, np.array(t), lead)
    g_f = Guarded(torch, None, 4, cap=1024)
    ctx.rank_encode(g_t.ptr, g_f.ptr, len(t))
    g_t.check_output(r, what=what)
    g_f.check_output(f, what=what + " freq")


@pytest.mark.parametrize("name", M.CASES)
def test_rank_encode(gpu, name):
    torch, jam, ctx = gpu
    for lead in (0, 3):
        _rank_encode(torch, ctx, name, lead)


def test_one_buffer_of_257_tiles(gpu):
    torch, jam, ctx = gpu
    _rank_encode(torch, ctx, M.TWO_CHUNKS, 1)


def test_two_chunks(gpu, oracle):
    torch, jam, ctx = gpu
    img = M.case(M.TWO_CHUNKS)
    assert jam.CHUNK == M.F.CHUNK and len(img) == M.F.CHUNK + M.ATILE + 1
    want = oracle.ans_encode(img)
    g_in = Guarded(torch, np.array(img), 3)
    g_out = Guarded(torch, None, 5, cap=len(want))
    assert ctx.ans_encode(g_in.ptr, len(img), g_out.ptr, len(want)) == len(want)
    g_out.check_output(want, used=len(want), what="ans_encode two-chunks")
    g_in.check_unchanged("ans_encode two-chunks")
