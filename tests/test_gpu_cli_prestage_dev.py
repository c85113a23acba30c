"""The pre-stage decoders of the stock CLI on the device (jpk_dev_blocks_lz77_decompress / _lpx_decode / _filters_decode) against the host
decoders of prestage.cpp on the same bytes: output, length and status, block by block of ONE batched call per stage.  -m gpu

Every buffer sits in a guarded allocation (stage_guard.Guarded) at its own lead in front of a 256-byte-aligned address, odd ones
included: after the call the guards around every output hold their sentinel, so do the bytes behind out_len, and the inputs are unchanged.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from golden_util import GOLD
from stage_guard import SENT, Guarded

pytestmark = pytest.mark.gpu

OK, E_CAPACITY, E_CORRUPT = 0, -2, -3
FBS = 64 << 10


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "golden_cli.npz")), json.load(open(os.path.join(GOLD, "golden_cli_manifest.json")))


def _u8(x):
    return np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray, list)) else x, dtype=np.uint8)


def _host(jam, stage, s, cap):
    """(status, output or None) of the host decoder"""
    s = _u8(s)
    out = np.full(max(cap, 1), SENT, dtype=np.uint8)
    n = C.c_int32(0)
    p = s.ctypes.data if len(s) else None
    if stage == "lpx":
        rc = jam.lib().jpk_lpx_decode(p, len(s), out.ctypes.data)
        n.value = len(s)
    else:
        fn = jam.lib().jpk_lz77_decompress if stage == "lz77" else jam.lib().jpk_filters_decode
        rc = fn(p, len(s), out.ctypes.data, cap, C.byref(n))
    return rc, (out[: n.value].copy() if rc == OK else None)


def _run(gpu, stage, cases):
    """cases: [(name, stream, out_cap)] -> one batched device call; every block compared with the host decoder.  Returns the statuses."""
    torch, jam, ctx = gpu
    ins, outs = [], []
    for i, (_, s, cap) in enumerate(cases):
        ins.append(Guarded(torch, _u8(s), (3 * i + 1) % 16))
        outs.append(Guarded(torch, None, (5 * i + 3) % 16, cap=cap))
    d_in, d_out = [g.ptr for g in ins], [g.ptr for g in outs]
    lens, caps = [len(_u8(s)) for _, s, _ in cases], [cap for _, _, cap in cases]
    if stage == "lz77":
        out_len, st = ctx.blocks_lz77_decompress(d_in, lens, d_out, caps)
    elif stage == "filters":
        out_len, st = ctx.blocks_filters_decode(d_in, lens, d_out, caps)
    else:
        st = ctx.blocks_lpx_decode(d_in, lens, d_out)
        out_len = lens
    for i, (name, s, cap) in enumerate(cases):
        what = f"{stage} {name} (block {i}, in {lens[i]}, cap {cap})"
        rc, exp = _host(jam, stage, s, cap)
        assert st[i] == rc, f"{what}: status {st[i]}, host {rc}"
        if rc == OK:
            assert out_len[i] == len(exp), f"{what}: out_len {out_len[i]}, host {len(exp)}"
            outs[i].check_output(exp, used=len(exp), what=what)
        else:
            outs[i].check_guards(what)
        ins[i].check_unchanged(what)
    return st


def _exact_and_one_short(gpu, stage, cases):
    """every stream at the capacity the host decoder needs, then all of them one byte short"""
    _, jam, _ = gpu
    exact = []
    for name, s in cases:
        rc, exp = _host(jam, stage, s, 1 << 23)
        exact.append((name, s, len(exp) if rc == OK else 64))
    st = _run(gpu, stage, exact)
    short = [(name + " cap-1", s, cap - 1) for (name, s, cap), rc in zip(exact, st) if rc == OK and cap > 0]
    st2 = _run(gpu, stage, short)
    assert short and all(rc == E_CAPACITY for rc in st2), st2
    return st


# ---- golden vectors of the reference encoders -----------------------------------------------------------------------------------
def test_golden_stage_vectors_in_one_batch_per_stage(gpu, golden):
    _, jam, _ = gpu
    z, man = golden
    for stage, corrupt in (("lz77", [0x00, 0x85]), ("filters", [3, 1, 0, 0]), ("lpx", None)):
        cases = []
        for c in [c for c in man["stages"] if c["stage"] == stage]:
            cases.append((c["name"], z[c["name"]], c["n"] + (0 if stage == "lpx" else 64)))
            cases.append(("empty", [], 16))
            if corrupt:
                cases.append(("corrupt", corrupt, 100))
        assert len(cases) >= 6
        st = _run(gpu, stage, cases)
        assert st == ([OK, OK, E_CORRUPT] * 3 if corrupt else [OK] * 6), (stage, st)
        # (_run compared with the host decoder; the host decoder's answer is the manifest's input)
        for c in [c for c in man["stages"] if c["stage"] == stage]:
            rc, exp = _host(jam, stage, z[c["name"]], c["n"] + 64)
            assert rc == OK and np.array_equal(exp[: c["n"]], jam.corpus.make(c["kind"], c["n"], c["seed"])), c["name"]


# ---- LZ77: streams from a small token writer ------------------------------------------------------------------------------------
def _leb(v):
    """LEB128 with carry (Utils::EncodeLeb128): big-endian 7-bit groups, bit 7 on the last byte, class offsets per length"""
    for d, base in enumerate((0, 127, 16510, 2113661, 270549116)):
        top = (127, 16510, 2113661, 270549116, 1 << 40)[d]
        if v <= top:
            x = v - base
            return [(x >> (7 * (d - k))) & 0x7F for k in range(d)] + [0x80 | (x & 0x7F)]
    raise ValueError(v)


def _tok(lit, off, length):
    lit = list(lit)
    m = length - 4
    lc, tc = min(m, 31), min(len(lit), 7)
    return [(lc << 3) | tc] + _leb(off) + (_leb(m - 31) if lc == 31 else []) + (_leb(len(lit) - 7) if tc == 7 else []) + lit


def _end(tail=()):
    return [0x00, 0x80] + list(tail)


def _lz_streams():
    rng = np.random.default_rng(91)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tolist()
    cs = []
    for n in (4, 63, 64, 65, 257, 70_000):                              # a run: one literal, then off = 1
        cs.append((f"off1 len{n}", _tok([0x41], 1, n) + _tok([0x42, 0x43], 2, 9)))
    for off in (63, 64, 65, 255, 256, 257):                             # len below and above off
        cs.append((f"off{off} short", _tok(rnd(off), off, max(4, off // 2)) + _end([1, 2, 3])))
        cs.append((f"off{off} long", _tok(rnd(off), off, 3 * off + 5) + _tok([], off + 7, off + 9)))
    cs.append(("len class 31 ext 0", _tok(rnd(10), 3, 35)))
    cs.append(("len class 31 ext large", _tok(rnd(10), 7, 100_000)))
    cs.append(("lit class 7 ext 0", _tok(rnd(7), 5, 6)))
    cs.append(("lit class 7 ext large", _tok(rnd(50_000), 49_999, 12)))
    cs.append(("offset 1 byte", _tok(rnd(200), 127, 300)))
    cs.append(("offset 2 bytes", _tok(rnd(6000), 5000, 12_000) + _tok(rnd(3), 16_510, 40)))
    cs.append(("offset 3 bytes", _tok(rnd(20_000), 17_000, 100) + _tok([9], 16_511, 33)))
    big = _tok(rnd(4096), 4096, 2_200_000)                               # 2.2 MiB of output behind a few KiB of input
    cs.append(("offset 4 bytes", big + _tok([1, 2, 3], 2_113_662, 500) + _tok([], 2_200_000, 70) + _end([7])))
    cs.append(("end marker, raw tail", _tok(rnd(5), 2, 8) + _end(rnd(1000))))
    cs.append(("end marker, empty tail", _tok(rnd(5), 2, 8) + _end()))
    cs.append(("end marker first", _end(rnd(300))))
    cs.append(("ends at a token boundary", _tok(rnd(3), 3, 4) + _tok(rnd(2), 1, 5)))
    cs.append(("empty input", []))
    return cs


def test_lz77_token_streams_exact_capacity_and_one_byte_short(gpu):
    st = _exact_and_one_short(gpu, "lz77", _lz_streams())
    assert all(rc == OK for rc in st), st


def test_lz77_bad_streams_have_the_host_status(gpu):
    bad = [("truncated LEB", [0x08, 0x01], 100),
           ("LEB of six bytes", [0x08, 1, 1, 1, 1, 1, 0x81], 100),
           ("off > op", [0x00, 0x85], 100),
           ("off > op behind literals", _tok([1, 2, 3], 4, 8), 100),
           ("lit beyond the input", [0x05, 0x81, 1, 2], 100),
           ("negative length extension", [0xF8, 0x81, 0x08, 0x00, 0x00, 0x00, 0x80], 100),
           ("negative literal extension", [0x07, 0x81, 0x08, 0x00, 0x00, 0x00, 0x80], 100),
           ("token alone", [0x08], 100),
           ("good one in between", _tok([5], 1, 20) + _end([1]), 100),
           ("match does not fit", _tok([5], 1, 200), 100),
           ("tail does not fit", _end(range(50)), 10)]
    st = _run(gpu, "lz77", bad)
    assert st == [E_CORRUPT] * 8 + [OK, E_CAPACITY, E_CAPACITY], st


# ---- LPX: any byte string is a stream -------------------------------------------------------------------------------------------
def test_lpx_every_length_and_content(gpu):
    _, jam, _ = gpu
    rng = np.random.default_rng(92)
    cases = []
    for n in (0, 1, 2, 3, 4, 5, 7, 4096, 50_001, 70_003):               # 50 001 and 70 003: a fifth part; 70 003: parts longer than a tile
        for kind in ("text", "repeat4k", "zero"):
            cases.append((f"{kind} {n}", jam.corpus.make(kind, n, 93), n))
        cases.append((f"random {n}", rng.integers(0, 256, n, dtype=np.uint8), n))
    # parts longer than the 64 KiB + one tile of output history the kernel keeps
    cases.append(("text 360001", jam.corpus.make("text", 360_001, 94), 360_001))
    cases.append(("zero 400000", np.zeros(400_000, np.uint8), 400_000))
    # the seams of the kernel's walk: parts of exactly one tile (16 KiB), one tile + 1, exactly the ring (80 KiB), the ring + 1
    for n in (65_536, 65_540, 327_680, 327_684):
        cases.append((f"seam zero {n}", np.zeros(n, np.uint8), n))
        cases.append((f"seam repeat4k {n}", jam.corpus.make("repeat4k", n, 95), n))
    st = _run(gpu, "lpx", cases)
    assert all(rc == OK for rc in st), st


def test_lpx_decodes_what_the_reference_encoded(gpu, golden):
    """streams WITH predicted stretches: the golden vectors, cut to other lengths' worth of parts by decoding a prefix"""
    z, man = golden
    cases = []
    for c in [c for c in man["stages"] if c["stage"] == "lpx"]:
        for n in (c["n"], c["n"] // 2 + 1, 4099):
            cases.append((f"{c['name']}[:{n}]", z[c["name"]][:n], n))
    _run(gpu, "lpx", cases)


# ---- filters: streams encoded by numpy ------------------------------------------------------------------------------------------
def _reorder(x, width):
    return np.concatenate([x[c::width] for c in range(width)]) if len(x) else x


def _filter_block(x, ftype, width):
    x = np.asarray(x, dtype=np.uint8)
    if width == 0:
        e = x
    elif ftype == 0:                                                     # delta over the de-interleaved channels
        d = _reorder(x, width)
        e = d - np.concatenate([np.zeros(1, np.uint8), d[:-1]]) if len(d) else d
    elif ftype == 2:                                                     # delta per channel in place, behind a raw head
        k0 = len(x) % width
        body = x[k0:].reshape(-1, width)
        e = np.concatenate([x[:k0], (body - np.concatenate([np.zeros((1, width), np.uint8), body[:-1]])).reshape(-1)]) if len(body) else x
    else:                                                                # adaptive linear predictor over the de-interleaved channels
        d = _reorder(x, width).tolist()
        e, w, p1, p2 = [], 0, 0, 0
        for cur in d:
            err = (w + 2 * p1 - p2 - cur) & 0xFF
            e.append(err)
            w += (err - w) >> 6
            p2, p1 = p1, cur
        e = np.array(e, dtype=np.uint8)
    return np.concatenate([np.array([ftype, width], np.uint8), e.astype(np.uint8)])


def _filter_stream(x, plan):
    """plan(j) -> (type, width) of filter block j"""
    parts = [_filter_block(x[o: o + FBS], *plan(j)) for j, o in enumerate(range(0, len(x), FBS))]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def _filter_cases(jam):
    x = jam.corpus.make("samples16", 2 * FBS + 77, 95)
    cs = []
    for ftype in (0, 1, 2):
        for width in (1, 2, 3, 4, 7, 32):
            lens = (10_007, FBS, FBS + 1) if width in (1, 3, 32) else (10_007,)     # short block (len % width != 0), one block, one block + 1 byte
            for n in lens:
                cs.append((f"type {ftype} width {width} len {n}", _filter_stream(x[:n], lambda j: (ftype, width))))
    for n in (0, 1, 5, 31):                                              # blocks shorter than the channel count
        cs.append((f"type 0 width 32 len {n}", _filter_stream(x[:n], lambda j: (0, 32))))
        cs.append((f"type 1 width 7 len {n}", _filter_stream(x[:n], lambda j: (1, 7))))
        cs.append((f"type 2 width 32 len {n}", _filter_stream(x[:n], lambda j: (2, 32))))
    cs.append(("width 0", _filter_stream(x[: FBS + 9], lambda j: (j % 3, 0))))
    cs.append(("all types mixed", _filter_stream(x, lambda j: ((0, 4), (1, 2), (2, 3))[j])))
    cs.append(("header alone", [1, 2]))
    return cs


def test_filters_every_type_and_width_exact_capacity_and_one_byte_short(gpu):
    _, jam, _ = gpu
    x = jam.corpus.make("samples16", FBS + 1, 95)
    # the numpy encoders are right: the host decoder gives the input back
    for ftype, width in ((0, 3), (1, 7), (2, 32)):
        rc, back = _host(jam, "filters", _filter_stream(x, lambda j: (ftype, width)), len(x))
        assert rc == OK and np.array_equal(back, x), (ftype, width)
    cases = _filter_cases(jam)
    st = _exact_and_one_short(gpu, "filters", cases)
    assert all(rc == OK for rc in st), st


def test_filters_bad_streams_have_the_host_status(gpu):
    _, jam, _ = gpu
    x = jam.corpus.make("text", FBS + 100, 96)
    full = _filter_stream(x[:FBS], lambda j: (0, 2))
    two = _filter_stream(x, lambda j: (2, 4))
    bad3 = two.copy(); bad3[FBS + 2] = 3
    bad33 = two.copy(); bad33[FBS + 3] = 33
    bad = [("one-byte tail", np.concatenate([full, np.array([0], np.uint8)]), 2 * FBS),
           ("type 3", [3, 1, 0, 0], 100),
           ("width 33", [0, 33, 0, 0], 100),
           ("one byte", [0], 100),
           ("type 3 in the second block", bad3, 2 * FBS),
           ("width 33 in the second block", bad33, 2 * FBS),
           ("good one in between", two, len(x)),
           ("second block does not fit", two, FBS + 99),
           ("bad second header behind a first block that does not fit", bad3, 100)]
    st = _run(gpu, "filters", bad)
    assert st == [E_CORRUPT] * 6 + [OK, E_CAPACITY, E_CAPACITY], st
