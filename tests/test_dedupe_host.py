"""The dedupe of the stock-CLI writer, host side (no GPU): jpk_lz77_dedupe through this library's Lz77::Decompress and the reference's,
its size, coverage and token-count properties, the 1 MiB pathological inputs (a quadratic rule does not finish them inside a test), and
the _ex forms of the stage chain.  The coverage bound |S1'| <= |X| + |Y| + 2 + 16 + 128 for X | Y | X follows from the rule for random X:
the copy's first anchored window lies at most 63 bytes behind its start, a run grows eight windows and 63 bytes backward from its head, so
the head may be the copy's eighth window, and the forward end is reached by byte equality whatever the table lost."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

from dedupe_cases import LITS, MiB, PATHOLOGICAL, SMALL, XS, YS, cases, tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_CAPACITY = 0, -1, -2
NEW = ("jpk_lz77_dedupe", "jpk_dev_blocks_lz77_dedupe", "jpk_cli_stages_encode_ex", "jpk_dev_blocks_cli_stages_encode_ex",
       "jpk_jam_cli_block_write_ex", "jpk_dev_jam_cli_compress_ex", "jpk_jam_cli_compress_ex")


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


@pytest.fixture(scope="module")
def streams(jam):
    """name -> (block, S1'), computed once; the pathological inputs are timed"""
    out, took = {}, {}
    for name, r in cases().items():
        t0 = time.perf_counter()
        out[name] = (r, jam.Lz77().dedupe(r))
        took[name] = time.perf_counter() - t0
    out["_took"] = took
    return out


def _items(streams):
    return [(k, v) for k, v in streams.items() if k != "_took"]


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS and name in jam.ABI_SYMBOLS, f"{name} has no ctypes signature"
    assert re.search(r"#define\s+JPK_CLI_DEDUPE\s+1\b", header) and jam.CLI_DEDUPE == 1
    assert hasattr(jam.Lz77, "dedupe") and hasattr(jam.Context, "blocks_lz77_dedupe")
    names = [jam.lib().jpk_ctx_profile_name(i).decode() for i in range(jam.lib().jpk_ctx_profile_count())]
    for k in ("k_dd_anchor", "k_dd_cand", "k_dd_extend", "k_dd_select", "k_dd_emit"):
        assert k in names, k


def test_round_trip_and_never_larger_than_stored(jam, ref, streams):
    for name, (r, s1) in _items(streams):
        assert len(s1) <= len(r) + 2, name
        assert np.array_equal(jam.Lz77().Decompress(s1, len(r)), r), name
        assert np.array_equal(ref.lz77_decompress(s1, len(r)), r), name
        pos = 0
        for lit, ln, off in tokens(s1):                                # every offset inside what is already there, every match >= 256
            pos += lit
            assert 1 <= off <= pos and ln >= 256, (name, lit, ln, off, pos)
            pos += ln
        assert pos <= len(r), name


def test_nothing_to_find_gives_the_stored_form(streams):
    names = ["text", "random"] + [f"n/{n}" for n in SMALL] + [f"xyx/255/{ny}" for ny in YS]
    for name in names:
        r, s1 = streams[name]
        assert np.array_equal(s1, np.concatenate([np.array([0x04, 0x80], dtype=np.uint8), r])), name


def test_a_copy_is_covered_up_to_128_bytes(streams):
    for nx in XS:
        for ny in YS:
            r, s1 = streams[f"xyx/{nx}/{ny}"]
            if nx >= 512:
                assert len(s1) <= nx + ny + 2 + 16 + 128, (nx, ny, len(s1))
            if nx >= 256:
                assert len(tokens(s1)) == 1, (nx, ny)
    for name, n_unique in (("ends_at_last_byte", 777 + 3000), ("source_at_byte_0", 3000 + 777), ("abab", 3600), ("copy_2.2MiB", 2_300_000)):
        r, s1 = streams[name]
        assert len(s1) <= n_unique + 2 + 16 + 128, (name, len(s1))
    (lit, ln, off), = tokens(streams["copy_2.2MiB"][1])
    assert ln - 35 >= 2_113_661 and off == 2_300_000                   # the match extension took its four-byte code


def test_a_near_copy_of_text_is_covered_between_its_changed_bytes(jam):
    """T | T' with T' = T but for one byte in 100 000 (the block of the sort-round test).  Text repeats itself at short range: the slot of
    several windows in a hundred names an earlier copy of the same 64 bytes and not the window one MiB in front.  A run crosses such windows
    by byte equality in both directions, so what stays literal between two matches is the changed byte and at most 128 bytes around it."""
    t = jam.corpus.make("text", MiB, 61)
    t2 = t.copy()
    t2[::100_000] ^= 1
    toks = tokens(jam.Lz77().dedupe(np.concatenate([t, t2])))
    assert all(off == MiB for _, _, off in toks), toks
    assert toks[0][0] <= MiB + 128 and all(1 <= lit <= 128 for lit, _, _ in toks[1:]), toks
    assert sum(ln for _, ln, _ in toks) >= MiB - 128 * 11, toks


def test_literal_extension_classes(streams):
    """a | b | b | lit random bytes | a | tail: the second b and the second a are tokens, the second with `lit` literals in front"""
    for lit in LITS:
        r, s1 = streams[f"lit/{lit}"]
        toks = tokens(s1)
        assert len(toks) == 2, (lit, toks)
        assert toks[0][2] == 700 and toks[1][2] == 600 + 1400 + lit, (lit, toks)
        assert abs(toks[1][0] - lit) <= 2, (lit, toks)                 # a random byte may agree with the copy at either end
        assert len(s1) <= 600 + 700 + lit + 50 + 2 + 32, lit


def test_token_counts(streams):
    assert len(tokens(streams["xxxx"][1])) <= 3
    r, s1 = streams["repeat4k"]
    assert len(tokens(s1)) <= len(r) // 4096 + 1
    assert len(s1) < len(r) // 50


def test_pathological_inputs_are_linear(streams):
    """1 MiB each: about 0.1 s with the rule of DESIGN 4.7; forward extension by byte equality alone is minutes on repeat4k / tile100"""
    for name in PATHOLOGICAL:
        assert streams["_took"][name] < 5.0, (name, streams["_took"][name])


def test_capacity_is_exact(jam, streams):
    for name in ("xyx/4096/65", "random", "n/0"):
        r, s1 = streams[name]
        out = np.full(len(s1) + 8, 0xA5, dtype=np.uint8)
        m = C.c_int32(-1)
        p = r.ctypes.data if len(r) else None
        assert jam.lib().jpk_lz77_dedupe(p, len(r), out.ctypes.data, len(s1) - 1, C.byref(m)) == E_CAPACITY and m.value == 0, name
        assert (out == 0xA5).all(), name
        assert jam.lib().jpk_lz77_dedupe(p, len(r), out.ctypes.data, len(s1), C.byref(m)) == OK and m.value == len(s1), name
        assert np.array_equal(out[: len(s1)], s1) and (out[len(s1):] == 0xA5).all(), name


EX_NAMES = ["xyx/70000/65", "xxxx", "abab", "repeat4k", "tile300", "text", "n/0", "n/1", "lit/135"]


def test_ex_chain_with_the_flag_decodes_through_all_four_decoders(jam, ref, streams):
    for name in EX_NAMES:
        r, s1 = streams[name]
        s4 = jam.cli_stages_encode(r, dedupe=True)
        assert len(s4) <= jam.cli_stages_bound(len(r)), name
        assert len(s4) == len(s1) + 2 + 2 * -(-len(s1) // 65_536), name
        a = jam.Lz77().Decompress(s4, len(s4))
        c = jam.Filters().Decode(jam.Lpx().Decode(a), len(a))
        assert np.array_equal(c, s1), name                             # S1 = S1'
        assert np.array_equal(jam.Lz77().Decompress(c, len(r)), r), name
        a = ref.lz77_decompress(s4, len(s4))
        c = ref.filters_decode(ref.lpx_decode(a), len(a))
        assert np.array_equal(ref.lz77_decompress(c, len(r)), r), name


def test_ex_chain_without_the_flag_is_the_existing_entry(jam, streams):
    for name in EX_NAMES:
        r, _ = streams[name]
        bound = jam.cli_stages_bound(len(r))
        a, b = np.zeros(bound + 1, dtype=np.uint8), np.zeros(bound + 1, dtype=np.uint8)
        m, k = C.c_int32(0), C.c_int32(0)
        p = r.ctypes.data if len(r) else None
        assert jam.lib().jpk_cli_stages_encode(p, len(r), a.ctypes.data, bound, C.byref(m)) == OK
        assert jam.lib().jpk_cli_stages_encode_ex(p, len(r), b.ctypes.data, bound, C.byref(k), 0) == OK
        assert m.value == k.value == bound and np.array_equal(a, b), name
        assert np.array_equal(jam.cli_stages_encode(r), a[:bound]), name
    r, _ = streams["random"]
    assert np.array_equal(jam.cli_stages_encode(r, dedupe=True), jam.cli_stages_encode(r))      # nothing found: the same bytes


def test_argument_checks_come_before_the_device_and_bad_flags_are_refused(jam):
    lib = jam.lib()
    a = np.zeros(64, dtype=np.uint8)
    out = np.zeros(256, dtype=np.uint8)
    n32, n64 = C.c_int32(0), C.c_int64(0)
    ap, op = a.ctypes.data, out.ctypes.data
    for args in ((ap, -1, op, 256, C.byref(n32)), (None, 5, op, 256, C.byref(n32)), (ap, 5, None, 256, C.byref(n32)), (ap, 5, op, -1, C.byref(n32)),
                 (ap, 5, op, 256, None)):
        assert lib.jpk_lz77_dedupe(*args) == E_ARG, args
        assert lib.jpk_cli_stages_encode_ex(*args, 1) == E_ARG, args
    for flags in (2, 3, 0x80000000):
        assert lib.jpk_cli_stages_encode_ex(ap, 64, op, 256, C.byref(n32), flags) == E_ARG
        assert lib.jpk_jam_cli_block_write_ex(ap, 64, MiB, op, 256, C.byref(n32), flags) == E_ARG
        assert lib.jpk_jam_cli_compress_ex(ap, 64, MiB, op, 256, C.byref(n64), 0, flags) == E_ARG
        assert lib.jpk_dev_jam_cli_compress_ex(None, ap, 64, MiB, op, 256, C.byref(n64), 0, flags) == E_ARG
    assert lib.jpk_dev_blocks_lz77_dedupe(None, 0, None, None, None, None, None, None) == E_ARG
    assert lib.jpk_dev_blocks_cli_stages_encode_ex(None, 0, None, None, None, None, None, None, 1) == E_ARG
    assert lib.jpk_dev_jam_cli_compress_ex(None, None, 0, MiB, None, 0, C.byref(n64), 0, 1) == E_ARG
    for args in ((ap, -1, MiB, op, 256, C.byref(n64), 0, 1), (ap, 64, MiB, op, -1, C.byref(n64), 0, 1), (ap, 64, MiB, op, 256, None, 0, 1),
                 (None, 64, MiB, op, 256, C.byref(n64), 0, 1), (ap, 64, MiB - 1, op, 256, C.byref(n64), 0, 1)):
        assert lib.jpk_jam_cli_compress_ex(*args) == E_ARG, args
    for args in ((ap, -1, MiB, op, 256, C.byref(n32), 1), (None, 64, MiB, op, 256, C.byref(n32), 1), (ap, 64, MiB - 1, op, 256, C.byref(n32), 1)):
        assert lib.jpk_jam_cli_block_write_ex(*args) == E_ARG, args
    assert lib.jpk_jam_cli_block_write_ex(ap, 64, MiB, op, 14, C.byref(n32), 1) == E_CAPACITY
    if lib.jpk_device_count() == 0:
        assert lib.jpk_jam_cli_compress_ex(ap, 64, MiB, op, 256, C.byref(n64), 0, 1) == -6
