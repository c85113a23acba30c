"""The parallel LZ77 expander on the device (jpk_dev_blocks_lz77_expand: k_lzx_plan + k_lzx_copy, k_pre_lz77 for the blocks they leave to
it) against the host decoder jpk_lz77_decompress and the serial device entry: output, length and status, block by block of ONE batched
call, on the crafted streams of lz_expand_cases.py.  jpk_debug_lz77_expand_last says which path the blocks took.  -m gpu

Every buffer sits in a guarded allocation (stage_guard.Guarded) at its own lead in front of a 256-byte-aligned address, odd ones
included: after the call the guards around every output hold their sentinel, so do the bytes behind out_len, and the inputs are unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import dedupe_cases
import lz_expand_cases as lzc
from stage_guard import SENT, Guarded

pytestmark = pytest.mark.gpu

OK, E_CAPACITY, E_CORRUPT = 0, -2, -3


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


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
    """[(name, stream, out_cap, path)] with out_cap None replaced by what the stream decodes to"""
    out = []
    for name, s, cap, path in cases:
        if cap is None:
            rc, exp = _host(jam, s, 1 << 22)
            assert rc == OK, name
            cap = len(exp)
        out.append((name, s, cap, path))
    return out


def _run(gpu, cases, lead0=0):
    """one batched call of the expander and one of the serial entry on the same streams; every block compared with the host decoder.
    Returns (statuses, (parallel, serial))"""
    torch, jam, ctx = gpu
    ins = [Guarded(torch, _u8(s), (3 * i + 1 + lead0) % 16) for i, (_, s, _, _) in enumerate(cases)]
    outs = [Guarded(torch, None, (5 * i + 3 + lead0) % 16, cap=cap) for i, (_, _, cap, _) in enumerate(cases)]
    outs2 = [Guarded(torch, None, (5 * i + 3 + lead0) % 16, cap=cap) for i, (_, _, cap, _) in enumerate(cases)]
    d_in, lens, caps = [g.ptr for g in ins], [len(_u8(s)) for _, s, _, _ in cases], [cap for _, _, cap, _ in cases]
    out_len, st = ctx.blocks_lz77_expand(d_in, lens, [g.ptr for g in outs], caps)
    paths = ctx.lz77_expand_last()
    out_len2, st2 = ctx.blocks_lz77_decompress(d_in, lens, [g.ptr for g in outs2], caps)
    for i, (name, s, cap, _) in enumerate(cases):
        what = f"{name} (block {i}, in {lens[i]}, cap {cap})"
        rc, exp = _host(jam, s, cap)
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
def valid(gpu):
    return _exact(gpu[1], lzc.valid_cases())


def test_every_valid_stream_alone_takes_its_path(gpu, valid):
    for case in valid:
        st, (par, ser) = _run(gpu, [case])
        assert st == [OK], case[0]
        assert (par, ser) == ((1, 0) if case[3] == "parallel" else (0, 1)), (case[0], par, ser)


def test_valid_streams_at_every_output_alignment(gpu, valid):
    """the word assembly at the two ends of the output: every lead 0..15 of d_out, on the streams with short records"""
    pick = [c for c in valid if c[0] in ("literals 17", "match period 3", "straddling sources", "words across records", "chase depth 8")]
    assert len(pick) == 5
    for lead in range(16):
        st, (par, ser) = _run(gpu, pick, lead0=lead)
        assert st == [OK] * 5 and (par, ser) == (5, 0), lead


def test_corrupt_streams_get_the_serial_status_and_stay_inside(gpu):
    cases = lzc.corrupt_cases()
    st, (par, ser) = _run(gpu, cases)
    assert (par, ser) == (0, len(cases))
    want = [E_CORRUPT] * 5 + [E_CAPACITY] * 3
    assert st == want, st


def test_sixteen_mixed_blocks_in_one_call(gpu, valid):
    cases = valid[1::2][:8] + [c for c in valid if c[3] == "serial"] + lzc.corrupt_cases()[:6]
    assert len(cases) == 16 and {c[3] for c in cases} == {"parallel", "serial"}
    st, (par, ser) = _run(gpu, cases)
    assert par == sum(c[3] == "parallel" for c in cases) and ser == 16 - par
    empty = [("none", b"", 0, "parallel")]
    assert _run(gpu, empty) == ([OK], (1, 0))


def test_the_dedupe_writers_streams(gpu):
    """what the stage sees in a staged frame: jpk_lz77_dedupe's S1'.  Ordinary repeats stay far under the record cap and one or two matches
    deep; a short period repeated over the whole block (tile300: 394 tokens in 2.6 KB of S1', each a copy of the one in front) does not,
    and goes to the serial kernel -- lz_expand_cases.path_of works the path out from the tokens"""
    _, jam, _ = gpu
    d = dedupe_cases.cases()
    cases = []
    blocks = {name: d[name] for name in ("xyx/70000/1000", "xxxx", "abab", "lit/16518", "n/0")}
    blocks["tile300"] = dedupe_cases.tile(300, 200_000, 8)
    blocks["text|text"] = np.tile(jam.corpus.make("text", 100_000, 11), 2)
    for name, r in blocks.items():
        s1 = jam.Lz77().dedupe(r)
        assert len(s1) < len(r) or len(r) < 512, name
        cases.append((name, s1, len(r), lzc.path_of(s1)))
    want = [c[3] for c in cases]
    assert want == ["parallel"] * 5 + ["serial", "parallel"], want
    st, (par, ser) = _run(gpu, cases)
    assert st == [OK] * len(cases) and (par, ser) == (6, 1)
