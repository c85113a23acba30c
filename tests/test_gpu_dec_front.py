"""The rANS decoder's front (k_dec_headers in ans_dec.hip, k_dec_rans with its ByteQueue in ans_dec_rans.hip, k_dec_rle in ans_dec_rank.hip, and
the batch plumbing around them in ans_dec.hip:
cbase, rle_off / out_off, the cleared rank arrays, k_dec_order) on the crafted streams of dec_front_model, bit-exact against the oracle
(which test_oracle_vs_ref.py pins to the reference build).  -m gpu

test_dec_front_model.py shows, from the streams alone, which arms every input reaches -- header values with one and two leading bytes in
the window before, for a frequency and for each length field, the header's end on lane 63 and on lane 0, surplus terminators that are
payload, headers at every start residue; the queue at every alignment, its first and second roll, a roll right after a four-byte
symbol, the partial and the absent dword at the input's end; every class and every byte pattern of a symbol, rebuilds of every class
with lg up to 5 and expn at its cap, the three class-7 registers, both pair models at both ends; digit groups over thread and pass
edges, of 1, 2, 19 and 20 digits -- and which one-token change of the scheme each input would expose.  Here the kernels decode them,
all valid streams, all on guarded buffers:
  * every case and chain at exact capacity, the stream 0, 1, 2, 3 and 15 bytes behind an aligned address (every queue alignment and both
    tail-dword arms for each: the model test says which lead gives which), the output 0, 1 and 7 bytes behind one; the input unchanged;
  * BATCH in one batched call, and once more in reverse order on the same context's arena: a zero-heavy block's ranks where a dense
    one's stood;
  * a chain of 1100 chunks, longer than the 1024 chains that run at once: the launch order is not the identity;
  * a capacity one byte short: JPK_E_CAPACITY from the header pass, nothing written;
  * the host entry."""
import functools

import numpy as np
import pytest

import dec_front_model as M
from stage_guard import Guarded

pytestmark = pytest.mark.gpu
NAMES = M.CASES + tuple(M.CHAINS)
OUT_LEADS = (0, 1, 7)
E_CAPACITY = -2


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _stream(name):
    """(stream, text) from the oracle: computed once, shared, left unchanged"""
    from oracle.pyoracle import Oracle
    return M.stream(Oracle(), name)


@pytest.mark.parametrize("name", NAMES)
def test_ans_decode_at_exact_capacity(gpu, name):
    torch, jam, ctx = gpu
    s, t = _stream(name)
    for i, lead in enumerate(M.IN_LEADS):
        what = f"ans_decode {name} lead={lead}"
        g_in = Guarded(torch, np.array(s), lead)
        g_out = Guarded(torch, None, OUT_LEADS[i % 3], cap=len(t))
        assert ctx.ans_decode(g_in.ptr, len(s), g_out.ptr, len(t)) == len(t), what
        g_out.check_output(t, what=what)
        g_in.check_unchanged(what)
    assert ctx.stats().ans_chunks == (len(M.CHAINS[name]) if name in M.CHAINS else 1)


def _batch(torch, ctx, names, what):
    pairs = [_stream(n) for n in names]
    g_in = [Guarded(torch, np.array(s), M.IN_LEADS[i % 5]) for i, (s, _) in enumerate(pairs)]
    g_out = [Guarded(torch, None, OUT_LEADS[i % 3], cap=len(t)) for i, (_, t) in enumerate(pairs)]
    n, st = ctx.blocks_ans_decode([g.ptr for g in g_in], [len(s) for s, _ in pairs], [g.ptr for g in g_out], [len(t) for _, t in pairs])
    assert st == [0] * len(names) and n == [len(t) for _, t in pairs], (what, st, n)
    for i, (_, t) in enumerate(pairs):
        g_out[i].check_output(t, what=f"{what} block {i} ({names[i]})")
        g_in[i].check_unchanged(f"{what} input {i} ({names[i]})")


def test_batch_then_reversed_on_the_same_arena(gpu):
    torch, jam, ctx = gpu
    _batch(torch, ctx, M.BATCH, "blocks_ans_decode")
    _batch(torch, ctx, M.BATCH[::-1], "blocks_ans_decode, reversed on the same arena")


def test_more_chains_than_run_at_once(gpu):
    torch, jam, ctx = gpu
    s, t = _stream("big-chain")
    g_in = Guarded(torch, np.array(s), 1)
    g_out = Guarded(torch, None, 7, cap=len(t))
    assert ctx.ans_decode(g_in.ptr, len(s), g_out.ptr, len(t)) == len(t)
    assert ctx.stats().ans_chunks == len(M.BIG_CHAIN) > 1024
    g_out.check_output(t, what="ans_decode big-chain")
    g_in.check_unchanged("ans_decode big-chain")


def test_capacity_one_byte_short_writes_nothing(gpu):
    torch, jam, ctx = gpu
    s, t = _stream("chain-two")
    g_in = Guarded(torch, np.array(s), 2)
    g_out = Guarded(torch, None, 1, cap=len(t) - 1)
    with pytest.raises(jam.JampackError) as e:
        ctx.ans_decode(g_in.ptr, len(s), g_out.ptr, len(t) - 1)
    assert e.value.status == E_CAPACITY, e.value
    g_out.check_output(np.zeros(0, dtype=np.uint8), used=0, what="ans_decode chain-two, one byte short")      # guards and the whole region
    g_in.check_unchanged("ans_decode chain-two, one byte short")


@pytest.mark.parametrize("name", ["class7", "chain-digits", "zeros-1MiB"])
def test_host_entry(gpu, name):
    torch, jam, ctx = gpu
    s, t = _stream(name)
    assert jam.ans_decoded_size(s) == (len(t), len(M.CHAINS[name]) if name in M.CHAINS else 1)
    assert np.array_equal(jam.Ans().Decode(np.array(s), len(t)), t), name
