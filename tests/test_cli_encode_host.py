"""The writer of stock-CLI frames, host side (no GPU): Lpx::Encode (jpk_lpx_encode) against the reference build and the committed golden
streams, the stored-form stage chain (jpk_cli_stages_bound / jpk_cli_stages_encode) through this library's four pre-stage decoders and
the reference's, and the argument checks of the new entries, which come before a device is looked for."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from golden_util import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
OK, E_ARG, E_CAPACITY = 0, -1, -2
NEW = ("jpk_lpx_encode", "jpk_cli_stages_bound", "jpk_cli_stages_encode", "jpk_jam_cli_block_write", "jpk_dev_blocks_lpx_encode",
       "jpk_dev_blocks_cli_stages_encode", "jpk_jam_cli_compress_bound", "jpk_dev_jam_cli_compress", "jpk_jam_cli_compress")
# the corpus kinds of the CLI goldens, + the two on which the model predicts at all: on the others Lpx::Encode returns its input
KINDS = ["text", "samples16", "repeat4k", "random", "runs", "geometric", "zero", "tile300"]
LPX_LENS = [0, 1, 2, 3, 4, 5, 7, 8] + list(range(65_535, 65_542)) + [4 * 81_920, 4 * 81_920 + 1, 4 * 81_920 + 5]
STAGE_NS = [0, 1, 65_533, 65_534, 65_535, 131_070, 131_071, MiB]


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


def make(jam, kind, n, seed):
    """corpus.make, + tile300: a 300-byte random tile repeated, one bit flipped every 1013 bytes (long predicted stretches with errors)"""
    if kind != "tile300":
        return jam.corpus.make(kind, n, seed)
    rng = np.random.default_rng(seed)
    t = np.tile(rng.integers(0, 256, 300, dtype=np.uint8), n // 300 + 1)[:n].copy()
    t[::1013] ^= 1
    return t


@pytest.fixture(scope="module")
def inputs(jam):
    return {(kind, n): make(jam, kind, n, 71) for kind in KINDS for n in LPX_LENS}


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS and name in jam.ABI_SYMBOLS, f"{name} has no ctypes signature"
    for name in ("blocks_lpx_encode", "blocks_cli_stages_encode", "jam_cli_compress"):
        assert hasattr(jam.Context, name), name
    for name in ("jam_cli_block_write", "jam_cli_compress", "jam_cli_compress_bound"):
        assert hasattr(jam, name), name
    assert hasattr(jam.Lpx, "encode")
    names = [jam.lib().jpk_ctx_profile_name(i).decode() for i in range(jam.lib().jpk_ctx_profile_count())]
    assert "k_enc_lpx" in names and "k_enc_wrap" in names


def test_argument_checks_come_before_the_device(jam):
    lib = jam.lib()
    a = np.zeros(64, dtype=np.uint8)
    out = np.zeros(256, dtype=np.uint8)
    n32, n64 = C.c_int32(0), C.c_int64(0)
    ap, op = a.ctypes.data, out.ctypes.data
    # the batch entries: as their decode siblings
    assert lib.jpk_dev_blocks_lpx_encode(None, 0, None, None, None, None) == lib.jpk_dev_blocks_lpx_decode(None, 0, None, None, None, None) == E_ARG
    assert lib.jpk_dev_blocks_cli_stages_encode(None, 0, None, None, None, None, None, None) == E_ARG
    assert lib.jpk_dev_blocks_lz77_decompress(None, 0, None, None, None, None, None, None) == E_ARG
    # the archive calls: as jpk_dev_jam_compress / jpk_jam_compress
    for cli, plain in ((lib.jpk_jam_cli_compress, lib.jpk_jam_compress),):
        for args in ((ap, -1, MiB, op, 256, C.byref(n64), 0),            # negative length
                     (ap, 64, MiB, op, -1, C.byref(n64), 0),             # negative capacity
                     (ap, 64, MiB, op, 256, None, 0),                    # no out_len
                     (None, 64, MiB, op, 256, C.byref(n64), 0),          # null input
                     (ap, 64, MiB, None, 256, C.byref(n64), 0),          # null output
                     (ap, 64, MiB - 1, op, 256, C.byref(n64), 0),        # block_size out of range
                     (ap, 64, (1000 << 20) + 1, op, 256, C.byref(n64), 0)):
            assert cli(*args) == plain(*args) == E_ARG, args
    assert lib.jpk_dev_jam_cli_compress(None, None, 0, MiB, None, 0, C.byref(n64), 0) == lib.jpk_dev_jam_compress(None, None, 0, MiB, None, 0, C.byref(n64), 0) == E_ARG
    for args in ((-1, MiB), (64, MiB - 1), (64, (1000 << 20) + 1)):
        assert lib.jpk_jam_cli_compress_bound(*args) == lib.jpk_jam_compress_bound(*args) == E_ARG
    assert lib.jpk_jam_cli_compress_bound(0, MiB) == 0
    # one frame: the rules of jpk_jam_block_write
    for args in ((ap, -1, MiB, op, 256, C.byref(n32)), (None, 64, MiB, op, 256, C.byref(n32)), (ap, 64, MiB, None, 256, C.byref(n32)),
                 (ap, 64, MiB, op, 256, None), (ap, 64, MiB, op, -1, C.byref(n32))):
        assert lib.jpk_jam_cli_block_write(*args) == lib.jpk_jam_block_write(*args) == E_ARG, args
    assert lib.jpk_jam_cli_block_write(ap, 64, MiB - 1, op, 256, C.byref(n32)) == E_ARG
    assert lib.jpk_jam_cli_block_write(ap, 64, (1000 << 20) + 1, op, 256, C.byref(n32)) == E_ARG
    big = np.zeros(MiB + 1, dtype=np.uint8)
    assert lib.jpk_jam_cli_block_write(big.ctypes.data, MiB + 1, MiB, op, 256, C.byref(n32)) == E_ARG      # in_len > block_size
    assert lib.jpk_jam_cli_block_write(ap, 64, MiB, op, 14, C.byref(n32)) == E_CAPACITY
    # the host stages
    assert lib.jpk_cli_stages_bound(-1) == E_ARG
    assert lib.jpk_lpx_encode(None, 5, op) == lib.jpk_lpx_decode(None, 5, op) == E_ARG
    assert lib.jpk_lpx_encode(ap, -1, op) == E_ARG
    assert lib.jpk_lpx_encode(ap, 5, None) == E_ARG
    assert lib.jpk_lpx_encode(None, 0, None) == OK
    assert lib.jpk_cli_stages_encode(ap, -1, op, 256, C.byref(n32)) == E_ARG
    assert lib.jpk_cli_stages_encode(None, 5, op, 256, C.byref(n32)) == E_ARG
    assert lib.jpk_cli_stages_encode(ap, 5, op, 256, None) == E_ARG
    if lib.jpk_device_count() == 0:
        assert lib.jpk_jam_cli_compress(ap, 64, MiB, op, 256, C.byref(n64), 0) == lib.jpk_jam_compress(ap, 64, MiB, op, 256, C.byref(n64), 0) == -6
        assert lib.jpk_jam_cli_compress(ap, 0, MiB, op, 256, C.byref(n64), 0) == lib.jpk_jam_compress(ap, 0, MiB, op, 256, C.byref(n64), 0)


def test_the_bound_is_the_arithmetic_of_the_stage_chain(jam):
    for n in STAGE_NS + [2, 65_536, 1000 << 20]:
        assert jam.cli_stages_bound(n) == n + 4 + 2 * -(-(n + 2) // 65_536), n
    # with the BWT trailer inside the reference decoder's (int)(BlockSize * 1.05) stage buffers, and inside this library's own bound
    for bs in (MiB, MiB + 1, 8 * MiB, 1000 << 20):
        assert jam.cli_stages_bound(bs) + 480 <= int(bs * 1.05) <= int(bs * 1.05) + 4096
    assert jam.cli_stages_bound(1000 << 20) < (1 << 30)


def test_lpx_encode_equals_the_golden_reference_streams(jam):
    """the three lpx_* arrays are the reference's Lpx::Encode outputs (tests/golden/make_golden_cli.py)"""
    z = np.load(os.path.join(GOLD, "golden_cli.npz"))
    man = json.load(open(os.path.join(GOLD, "golden_cli_manifest.json")))
    cases = [c for c in man["stages"] if c["stage"] == "lpx"]
    assert len(cases) == 3
    for c in cases:
        t = jam.corpus.make(c["kind"], c["n"], c["seed"])
        assert np.array_equal(jam.Lpx().encode(t), z[c["name"]]), c["name"]


@pytest.mark.parametrize("kind", KINDS)
def test_lpx_encode_matches_reference(jam, ref, inputs, kind):
    for n in LPX_LENS:
        if n < 4:
            continue                     # the reference's part loop never ends / divides by zero for len < 4 (lpx.cpp:150)
        t = inputs[kind, n]
        assert np.array_equal(jam.Lpx().encode(t), ref.lpx_encode(t)), (kind, n)


@pytest.mark.parametrize("kind", KINDS)
def test_lpx_decode_inverts_encode(jam, inputs, kind):
    changed = 0
    for n in LPX_LENS:
        t = inputs[kind, n]
        e = jam.Lpx().encode(t)
        assert len(e) == n
        assert np.array_equal(jam.Lpx().Decode(e), t), (kind, n)
        changed += int((e != t).sum())
    if kind in ("runs", "tile300"):
        assert changed > 100_000, "the model never predicted: these inputs are here because it does"


@pytest.fixture(scope="module")
def stage_cases(jam):
    """n -> (input, S4); mixed content so that the LPX model predicts inside the runs"""
    out = {}
    for n in STAGE_NS:
        t = np.concatenate([make(jam, "tile300", n // 2, 72), jam.corpus.make("text", n - n // 2, 73)]) if n else np.zeros(0, dtype=np.uint8)
        out[n] = (t, jam.cli_stages_encode(t))
    return out


def test_stages_length_is_the_bound_and_one_byte_less_is_capacity(jam, stage_cases):
    for n, (t, s4) in stage_cases.items():
        bound = jam.cli_stages_bound(n)
        assert len(s4) == bound, n
        assert s4[0] == 0x04 and s4[1] == 0x80, n
        out = np.full(bound + 8, 0xA5, dtype=np.uint8)
        m = C.c_int32(-1)
        p = t.ctypes.data if n else None
        assert jam.lib().jpk_cli_stages_encode(p, n, out.ctypes.data, bound - 1, C.byref(m)) == E_CAPACITY, n
        assert (out == 0xA5).all(), n
        assert jam.lib().jpk_cli_stages_encode(p, n, out.ctypes.data, bound, C.byref(m)) == OK and m.value == bound, n
        assert np.array_equal(out[:bound], s4) and (out[bound:] == 0xA5).all(), n


def test_stages_round_trip_through_the_four_decoders(jam, stage_cases):
    for n, (t, s4) in stage_cases.items():
        a = jam.Lz77().Decompress(s4, len(s4))
        assert len(a) == len(s4) - 2
        b = jam.Lpx().Decode(a)
        c = jam.Filters().Decode(b, len(b))
        assert len(c) == n + 2 and c[0] == 0x04 and c[1] == 0x80
        d = jam.Lz77().Decompress(c, n)
        assert np.array_equal(d, t), n


def test_stages_round_trip_through_the_reference_decoders(jam, ref, stage_cases):
    for n, (t, s4) in stage_cases.items():
        a = ref.lz77_decompress(s4, len(s4))
        b = ref.lpx_decode(a)
        c = ref.filters_decode(b, len(b))
        d = ref.lz77_decompress(c, n)
        assert np.array_equal(d, t), n
