"""The filter choice of the stock-CLI writer, host side (no GPU): jpk_filters_encode through this library's Filters::Decode and the
reference's, the choice of every piece against an argmin written here over jpk_filters_cost (which counts a candidate's output bytes
themselves, while the encoder derives its histograms from shared differences), the cost against numpy floats, the inputs that must stay
stored, what the option is for -- smaller blocks behind the BWT, with the CPU oracle -- and the flags of the _ex entries.
The cost bound: |lg12(v) - 4096 log2 v| <= 1 for both logarithms of a term h (lg12(len) - lg12(h)), so a term is off by at most 2 h and
the sum by at most 2 len."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from filter_cases import FBS, MiB, STORED_KINDS, headers, mixed, pieces, rec, rgb, round_trip_inputs, stereo16, structs12

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_CAPACITY = 0, -1, -2
NEW = ("jpk_filters_encode", "jpk_filters_cost", "jpk_dev_blocks_filters_encode")
TOKEN = np.array([0x04, 0x80], dtype=np.uint8)


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


def _argmin(jam, piece):
    """the rule, written out: raw keeps a sixteenth, type 0 at widths 1..32, then type 2, strictly below the best so far"""
    raw = jam.filters_cost(piece, 0, 0)
    best, choice = raw - (raw >> 4), (0, 0)
    for t in (0, 2):
        for w in range(1, 33):
            c = jam.filters_cost(piece, t, w)
            if c < best:
                best, choice = c, (t, w)
    return choice


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS and name in jam.ABI_SYMBOLS, f"{name} has no ctypes signature"
    assert re.search(r"#define\s+JPK_CLI_FILTERS\s+4\b", header) and jam.CLI_FILTERS == 4
    assert hasattr(jam.Filters, "Encode") and hasattr(jam.Context, "blocks_filters_encode") and callable(jam.filters_cost)
    names = [jam.lib().jpk_ctx_profile_name(i).decode() for i in range(jam.lib().jpk_ctx_profile_count())]
    assert "k_enc_filters" in names


def test_round_trip_through_both_decoders(jam):
    from oracle.pyoracle import Ref
    ref = Ref() if Ref.available() else None
    filtered = 0
    for name, x in round_trip_inputs():
        s2 = jam.Filters().Encode(x)
        assert len(s2) == len(x) + 2 * -(-len(x) // FBS), name
        assert np.array_equal(jam.Filters().Decode(s2, len(x)), x), name
        if ref is not None and len(x):
            assert np.array_equal(ref.filters_decode(s2, len(x)), x), name
        hs = headers(s2, len(x))
        assert all(t in (0, 2) and w <= 32 for t, w in hs), (name, hs)
        filtered += sum(1 for _, w in hs if w)
    assert filtered >= 40                                              # the round trip is not one of stored pieces


def test_the_choice_is_the_argmin_of_the_costs(jam):
    seen = set()
    for name, x in mixed().items():
        hs = headers(jam.Filters().Encode(x), len(x))
        want = [_argmin(jam, p) for p in pieces(x)]
        assert hs == want, (name, hs, want)
        assert len(set(hs)) >= 3, (name, hs)                           # neighbouring pieces chose differently
        seen.update(hs)
    assert (0, 0) in seen and {t for t, w in seen if w} == {0, 2}, seen    # raw, and both types won somewhere


@pytest.mark.parametrize("w", [2, 3, 4, 7, 12, 16, 29, 31, 32])
def test_records_of_width_w_are_filtered_at_width_w(jam, w):
    x = rec(2 * FBS, w, 20 + w)
    hs = headers(jam.Filters().Encode(x), len(x))
    assert [hw for _, hw in hs] == [w, w], hs


def test_cost_values(jam):
    assert jam.filters_cost(np.full(FBS, 7, np.uint8), 0, 0) == 0
    assert jam.filters_cost(np.full(1, 200, np.uint8), 0, 0) == 0
    assert jam.filters_cost(np.full(4097, 9, np.uint8), 2, 5) == jam.filters_cost(np.r_[np.full(7, 9), np.zeros(4090)].astype(np.uint8), 0, 0)
    every = np.tile(np.arange(256, dtype=np.uint8), 256)
    assert jam.filters_cost(every, 0, 0) == 65_536 * 8 * 4096
    assert jam.filters_cost(every, 0, 1) == jam.filters_cost(np.r_[0, np.ones(65_535)].astype(np.uint8), 0, 0)
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 255, 1000, 40_001, FBS - 1, FBS):
        for p in (rng.integers(0, 256, n), rng.integers(0, 3, n), np.minimum(rng.geometric(0.05, n), 255), rec(n, 3, n)):
            p = p.astype(np.uint8)
            h = np.bincount(p, minlength=256).astype(np.float64)
            h = h[h > 0]
            exact = 4096.0 * float(np.sum(h * np.log2(n / h)))
            got = jam.filters_cost(p, 0, 0)
            assert abs(got - exact) <= 2 * n, (n, got, exact)
    p = np.zeros(FBS + 1, np.uint8)
    c = C.c_int64(0)
    for n, t, w in ((0, 0, 0), (16, 1, 1), (16, 3, 1), (16, -1, 1), (16, 0, 33), (16, 2, -1), (FBS + 1, 0, 0)):
        assert jam.lib().jpk_filters_cost(p.ctypes.data, n, t, w, C.byref(c)) == E_ARG, (n, t, w)
    assert jam.lib().jpk_filters_cost(p.ctypes.data, 16, 1, 0, C.byref(c)) == OK and c.value == 0      # raw: the type is not looked at
    assert jam.lib().jpk_filters_cost(None, 16, 0, 0, C.byref(c)) == E_ARG and jam.lib().jpk_filters_cost(p.ctypes.data, 16, 0, 0, None) == E_ARG


def test_capacity_and_arguments_of_the_host_encoder(jam):
    x = rec(FBS + 9, 3, 2)
    s2 = jam.Filters().Encode(x)
    out = np.full(len(s2) + 8, 0xA5, dtype=np.uint8)
    m = C.c_int32(-1)
    assert jam.lib().jpk_filters_encode(x.ctypes.data, len(x), out.ctypes.data, len(s2) - 1, C.byref(m)) == E_CAPACITY
    assert (out == 0xA5).all()
    assert jam.lib().jpk_filters_encode(x.ctypes.data, len(x), out.ctypes.data, len(s2), C.byref(m)) == OK and m.value == len(s2)
    assert np.array_equal(out[: len(s2)], s2) and (out[len(s2):] == 0xA5).all()
    assert jam.lib().jpk_filters_encode(None, 0, None, 0, C.byref(m)) == OK and m.value == 0
    for args in ((None, 5, out.ctypes.data, 64, C.byref(m)), (x.ctypes.data, -1, out.ctypes.data, 64, C.byref(m)), (x.ctypes.data, 5, None, 64, C.byref(m)),
                 (x.ctypes.data, 5, out.ctypes.data, -1, C.byref(m)), (x.ctypes.data, 5, out.ctypes.data, 64, None)):
        assert jam.lib().jpk_filters_encode(*args) == E_ARG, args


def test_stored_inputs_stay_stored(jam):
    for kind in STORED_KINDS:
        x = jam.corpus.make(kind, MiB, 3)
        a, b = jam.cli_stages_encode(x, filters=True), jam.cli_stages_encode(x)
        assert np.array_equal(a, b), kind
    x = jam.corpus.make("text", 300_000, 3)
    assert all(hw == (0, 0) for hw in headers(jam.Filters().Encode(x), len(x)))


def test_the_chain_with_the_flag_decodes_and_flag_5_filters_the_dedupe_output(jam):
    x = np.concatenate([rgb(200_000, 3), jam.corpus.make("text", 70_000, 4), rgb(4096, 3)[:4096], stereo16(131_072)])
    x[150_000: 154_096] = x[1000: 5096]                                # a 4 KiB copy
    for dedupe in (False, True):
        s1 = jam.Lz77().dedupe(x) if dedupe else np.concatenate([TOKEN, x])
        s4 = jam.cli_stages_encode(x, dedupe=dedupe, filters=True)
        assert len(s4) == len(jam.cli_stages_encode(x, dedupe=dedupe)) <= jam.cli_stages_bound(len(x))
        assert np.array_equal(s4[:2], TOKEN)
        s2 = jam.Lpx().Decode(s4[2:])
        assert np.array_equal(s2, jam.Filters().Encode(s1)), dedupe    # with both bits set the dedupe's S1' is what gets filtered
        assert any(w for _, w in headers(s2, len(s1)))
        a = jam.Lz77().Decompress(s4, len(s4))
        c = jam.Filters().Decode(jam.Lpx().Decode(a), len(a))
        assert np.array_equal(jam.Lz77().Decompress(c, len(x)), x), dedupe
    assert len(jam.Lz77().dedupe(x)) < len(x) - 3000


# measured with these generators: stereo16 0.475, rgb 0.359, structs12 0.356 (stored S2 918 270 / 1 046 402 / 558 464 bytes behind
# the oracle's block compressor)
@pytest.mark.parametrize("name,make,bar", [("stereo16", stereo16, 0.60), ("rgb", lambda: rgb(MiB, 1), 0.50), ("structs12", lambda: structs12(MiB, 1), 0.50)])
def test_filtered_blocks_compress_smaller(jam, oracle, name, make, bar):
    s1 = np.concatenate([TOKEN, make()])
    stored = np.concatenate([np.concatenate([np.zeros(2, np.uint8), p]) for p in pieces(s1)])
    filtered = jam.Filters().Encode(s1)
    a, b = len(oracle.compress_block(filtered)), len(oracle.compress_block(stored))
    print(f"{name}: stored {b}, filtered {a}, ratio {a / b:.3f}; headers {sorted(set(headers(filtered, len(s1))))}")
    assert a <= bar * b, (name, a, b, a / b)


def test_flags(jam):
    lib = jam.lib()
    a = rec(64, 4, 1)
    out = np.zeros(4096, dtype=np.uint8)
    n32, n64 = C.c_int32(0), C.c_int64(0)
    ap, op = a.ctypes.data, out.ctypes.data
    for flags in (4, 5):                                               # accepted: past the flag check, on to the next one
        assert lib.jpk_cli_stages_encode_ex(ap, 64, op, 4096, C.byref(n32), flags) == OK and n32.value == 64 + 4 + 2
        assert lib.jpk_jam_cli_block_write_ex(ap, 64, MiB, op, 14, C.byref(n32), flags) == E_CAPACITY
        assert lib.jpk_jam_cli_compress_ex(ap, 64, MiB, op, 4096, C.byref(n64), 0, flags) in ((OK,) if lib.jpk_device_count() else (-6,))
        assert lib.jpk_dev_jam_cli_compress_ex(None, ap, 64, MiB, op, 4096, C.byref(n64), 0, flags) == E_ARG     # no context
        assert lib.jpk_dev_blocks_cli_stages_encode_ex(None, 0, None, None, None, None, None, None, flags) == E_ARG
    for flags in (2, 3, 6, 8, 0x80000000):
        assert lib.jpk_cli_stages_encode_ex(ap, 64, op, 4096, C.byref(n32), flags) == E_ARG
        assert lib.jpk_jam_cli_block_write_ex(ap, 64, MiB, op, 14, C.byref(n32), flags) == E_ARG
        assert lib.jpk_jam_cli_compress_ex(ap, 64, MiB, op, 4096, C.byref(n64), 0, flags) == E_ARG
        assert lib.jpk_dev_jam_cli_compress_ex(None, ap, 64, MiB, op, 4096, C.byref(n64), 0, flags) == E_ARG
    assert lib.jpk_dev_blocks_filters_encode(None, 0, None, None, None, None, None, None) == E_ARG
    assert np.array_equal(jam.cli_stages_encode(a, filters=False), jam.cli_stages_encode(a))

