"""The deep LZ77 expander on the device (jpk_dev_blocks_lz77_expand_deep: k_lzd_plan + k_lzd_copy, k_pre_lz77 for the blocks they leave
to it) against the host decoder jpk_lz77_decompress and the serial device entry: output, length and status, block by block, on the
crafted streams of lz_deep_cases.py and on every stream of lz_expand_cases.py.  jpk_debug_lz77_deep_last says which path the blocks
took, lz_deep_cases.deep_path_of which one they should, from the limits the library reports.  -m gpu

Every buffer sits in a guarded allocation (stage_guard.Guarded) at its own lead in front of a 256-byte-aligned address, odd ones
included: after the call the guards around every output hold their sentinel, so do the bytes behind out_len, and the inputs are unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import lz_deep_cases as lzd
import lz_expand_cases as lzc
from stage_guard import SENT, Guarded

pytestmark = pytest.mark.gpu

OK, E_ARG, E_CAPACITY, E_CORRUPT = 0, -1, -2, -3


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@pytest.fixture(scope="module")
def limits(gpu):
    lim = gpu[1].lz77_deep_limits()
    assert lim == lzd.LIMITS and lim[0] >= 32 and lim[0] & (lim[0] - 1) == 0
    return lim


def _u8(x):
    return np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def _host(jam, s, cap):
    """(status, output or None) of jpk_lz77_decompress"""
    s = _u8(s)
    out = np.full(max(cap, 1), SENT, dtype=np.uint8)
    n = C.c_int32(0)
    rc = jam.lib().jpk_lz77_decompress(s.ctypes.data if len(s) else None, len(s), out.ctypes.data, cap, C.byref(n))
    return rc, (out[: n.value].copy() if rc == OK else None)


def _exact(jam, cases):
    """[(name, stream, out_cap, path, host status, host output)]: out_cap None replaced by what the stream decodes to; the host decoder
    runs once per case here and its answer is shared by every test"""
    out = []
    for name, s, cap, path in cases:
        if cap is None:
            rc, exp = _host(jam, s, 1 << 22)
            assert rc == OK, name
            cap = len(exp)
        else:
            rc, exp = _host(jam, s, cap)
        out.append((name, s, cap, path, rc, exp))
    return out


def _run(gpu, cases, lead0=0, leads=None):
    """one batched call of the deep expander and one of the serial entry on the same streams; every block compared with the host decoder.
    Returns (statuses, (parallel, serial))"""
    torch, jam, ctx = gpu
    lead = leads if leads is not None else [(5 * i + 3 + lead0) % 16 for i in range(len(cases))]
    ins = [Guarded(torch, _u8(c[1]), (3 * i + 1 + lead0) % 16) for i, c in enumerate(cases)]
    outs = [Guarded(torch, None, lead[i], cap=c[2]) for i, c in enumerate(cases)]
    outs2 = [Guarded(torch, None, lead[i], cap=c[2]) for i, c in enumerate(cases)]
    d_in, lens, caps = [g.ptr for g in ins], [len(_u8(c[1])) for c in cases], [c[2] for c in cases]
    out_len, st = ctx.blocks_lz77_expand_deep(d_in, lens, [g.ptr for g in outs], caps)
    paths = ctx.lz77_deep_last()
    out_len2, st2 = ctx.blocks_lz77_decompress(d_in, lens, [g.ptr for g in outs2], caps)
    for i, (name, s, cap, _, rc, exp) in enumerate(cases):
        what = f"{name} (block {i}, in {lens[i]}, cap {cap}, lead {lead[i]})"
        assert st[i] == st2[i] == rc, f"{what}: status {st[i]}, serial entry {st2[i]}, host {rc}"
        assert out_len[i] == out_len2[i], what
        if rc == OK:
            assert out_len[i] == len(exp), f"{what}: out_len {out_len[i]}, host {len(exp)}"
            outs[i].check_output(exp, used=len(exp), what=what)
        else:
            outs[i].check_guards(what)
            # a refused block holds what the serial kernel left in it
            a, b = outs[i].host()[outs[i].off: outs[i].off + cap], outs2[i].host()[outs2[i].off: outs2[i].off + cap]
            assert np.array_equal(a, b), what
        ins[i].check_unchanged(what)
    return st, paths


@pytest.fixture(scope="module")
def valid(gpu, limits):
    cases = lzd.valid_cases(limits)
    assert {name: path for name, _, _, path in cases} == lzd.expected_paths(limits)
    return _exact(gpu[1], cases)


@pytest.fixture(scope="module")
def older(gpu, limits):
    """the expander's own cases with the deep rule's paths"""
    return _exact(gpu[1], [(name, s, cap, lzd.deep_path_of(s, limits)) for name, s, cap, _ in lzc.valid_cases()])


def _named(cases, name):
    return next(c for c in cases if c[0] == name)


def test_every_valid_stream_alone_takes_its_path(gpu, valid):
    for case in valid:
        st, (par, ser) = _run(gpu, [case])
        assert st == [OK], case[0]
        assert (par, ser) == ((1, 0) if case[3] == "parallel" else (0, 1)), (case[0], par, ser)


def test_the_depths_of_real_streams_and_the_cap_itself_stay_parallel(gpu, valid, limits):
    hops = limits[0]
    for d, want in ((9, (1, 0)), (15, (1, 0)), (hops, (1, 0)), (hops + 1, (0, 1))):
        for kind in ("deep chase", "generations"):
            st, paths = _run(gpu, [_named(valid, f"{kind} {d}")])
            assert st == [OK] and paths == want, (kind, d, paths)


def test_valid_streams_in_batched_calls_of_sixteen(gpu, valid):
    for b0 in range(0, len(valid), 16):
        cases = valid[b0: b0 + 16]
        cases = cases + valid[: 16 - len(cases)]                        # the last call is filled up from the front
        assert len(cases) == 16
        st, (par, ser) = _run(gpu, cases)
        assert st == [OK] * 16
        assert par == sum(c[3] == "parallel" for c in cases) and ser == 16 - par


def test_the_expanders_own_cases_through_the_deep_entry(gpu, older):
    """bytes and statuses equal the serial entry's whatever the path.  Those streams are small and dense: the ones with several short
    records are over the budget of the deep rule within their first tokens, chase(9) with its 64-byte matches among them"""
    st, (par, ser) = _run(gpu, older)
    assert st == [OK] * len(older)
    assert par == sum(c[3] == "parallel" for c in older) and ser == len(older) - par and par >= 10 and ser >= 4
    assert _named(older, "chase depth 9")[3] == "serial" and _named(older, "match period 3")[3] == "parallel"
    cases = _exact(gpu[1], lzc.corrupt_cases())
    st, (par, ser) = _run(gpu, cases)
    assert (par, ser) == (0, len(cases))
    assert st == [E_CORRUPT] * 5 + [E_CAPACITY] * 3, st


def test_every_output_alignment(gpu, valid, limits):
    """the word assembly at the two ends of the output and the per-byte chase: every lead 0..15 of d_out"""
    hops = limits[0]
    pick = [_named(valid, "short records"), _named(valid, f"period 3 depth {hops}"), _named(valid, f"period 17 depth {hops}"),
            _named(valid, f"deep chase {hops}"), _named(valid, "record edge 17")]
    for lead in range(16):
        st, (par, ser) = _run(gpu, pick, lead0=lead, leads=[lead] * len(pick))
        assert st == [OK] * len(pick) and (par, ser) == (len(pick), 0), lead


def test_a_mixed_batch_keeps_its_blocks_apart(gpu, valid, limits):
    """parallel blocks, a block one hop too deep and a corrupt block in one call: the good ones are untouched by the others (their bytes,
    guards and tails are checked by _run), the refused one holds what the serial kernel left"""
    hops = limits[0]
    bad = _exact(gpu[1], lzc.corrupt_cases())
    cases = [_named(valid, f"generations {hops}"), _named(valid, f"generations {hops + 1}"), bad[1], _named(valid, "short input"),
             bad[5], _named(valid, f"period 3 depth {hops}"), _named(valid, "one record over the budget"), _named(valid, "tiny 0")]
    st, (par, ser) = _run(gpu, cases)
    assert st == [OK, OK, E_CORRUPT, OK, E_CAPACITY, OK, OK, OK] and (par, ser) == (4, 4)
    empty = [("none", b"", 0, "parallel", OK, np.zeros(0, dtype=np.uint8))]
    assert _run(gpu, empty) == ([OK], (1, 0))


def test_argument_errors_come_before_any_device_call(gpu):
    torch, jam, ctx = gpu
    fn = jam.lib().jpk_dev_blocks_lz77_expand_deep
    P, I = C.c_void_p * 1, C.c_int32 * 1
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ol, st = I(), I()
    good = (P(buf.data_ptr()), I(2), P(buf.data_ptr() + 32), I(8), ol, st)
    assert fn(None, 1, *good) == E_ARG
    assert fn(ctx._h, -1, *good) == E_ARG
    assert fn(ctx._h, 1, None, *good[1:]) == E_ARG
    assert fn(ctx._h, 1, good[0], None, *good[2:]) == E_ARG
    assert fn(ctx._h, 1, good[0], good[1], None, *good[3:]) == E_ARG
    assert fn(ctx._h, 1, good[0], good[1], good[2], None, ol, st) == E_ARG
    assert fn(ctx._h, 1, good[0], good[1], good[2], good[3], None, st) == E_ARG
    assert fn(ctx._h, 1, good[0], I(-1), *good[2:]) == E_ARG
    assert fn(ctx._h, 1, good[0], good[1], good[2], I(-1), ol, st) == E_ARG
    assert fn(ctx._h, 1, P(None), *good[1:]) == E_ARG
    assert fn(ctx._h, 1, good[0], good[1], P(None), good[3], ol, st) == E_ARG
    assert fn(ctx._h, 0, None, None, None, None, None, None) == OK and ctx.lz77_deep_last() == (0, 0)
    p = C.c_int32(0)
    assert jam.lib().jpk_debug_lz77_deep_last(ctx._h, None, C.byref(p)) == E_ARG
    assert jam.lib().jpk_debug_lz77_deep_limits(None, C.byref(p), C.byref(p)) == E_ARG
