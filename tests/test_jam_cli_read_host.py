"""Range reads of stock-CLI .jam archives, host side (no GPU): the new entries are exported, declared and bound, jpk_jam_index_kind
tells the two kinds of index apart, and the argument checks of the stock-CLI index creators and of jpk_dev_jam_cli_decompress_ix come
before any device is looked for -- an empty archive gives an empty index of kind 1 without one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jpk_dev_jam_cli_index_create", "jpk_jam_cli_index_create", "jpk_jam_index_kind", "jpk_dev_jam_cli_decompress_ix")
OK, E_ARG, E_NODEVICE = 0, -1, -6
PLAIN, CLI = 0, 1


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


@pytest.fixture(scope="module")
def fake_ctx():
    """a context pointer that is not NULL: the checks under test return before they look at it"""
    return C.create_string_buffer(4096)


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS and name in jam.ABI_SYMBOLS, f"{name} has no ctypes signature"
    assert re.search(r"#define\s+JPK_JAM_INDEX_PLAIN\s+0\b", header) and re.search(r"#define\s+JPK_JAM_INDEX_CLI\s+1\b", header)
    assert hasattr(jam, "jam_cli_index")
    for name in ("jam_cli_index", "jam_cli_decompress_ix", "jam_read"):
        assert hasattr(jam.Context, name), name


def test_status_values(jam):
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    assert int(re.search(r"JPK_E_ARG\s*=\s*(-?\d+)", header).group(1)) == E_ARG
    assert int(re.search(r"JPK_E_NODEVICE\s*=\s*(-?\d+)", header).group(1)) == E_NODEVICE


def test_kind_of_a_plain_index_and_of_null(jam):
    lib = jam.lib()
    data = jam.corpus.make("text", 3000, 61)
    ix = jam.jam_index(np.zeros(0, dtype=np.uint8))
    assert lib.jpk_jam_index_kind(ix._h) == PLAIN and ix.kind == PLAIN
    assert lib.jpk_jam_index_kind(None) == E_ARG
    # a walk that stops at once is still a plain index
    ix = jam.jam_index(data)
    assert (ix.frames, ix.bad_frame, ix.kind) == (0, 0, PLAIN)


def _create_host(lib, a, in_len, with_index=True):
    h, bad = C.c_void_p(), C.c_int32(-7)
    rc = lib.jpk_jam_cli_index_create(a.ctypes.data if a is not None else None, in_len, C.byref(h) if with_index else None, C.byref(bad))
    return rc, h, bad.value


def _create_dev(lib, ctx, d_in, in_len, with_index=True):
    h, bad = C.c_void_p(), C.c_int32(-7)
    rc = lib.jpk_dev_jam_cli_index_create(ctx, d_in, in_len, C.byref(h) if with_index else None, C.byref(bad))
    return rc, h, bad.value


def test_index_create_argument_checks(jam, fake_ctx):
    lib = jam.lib()
    a = np.zeros(64, dtype=np.uint8)
    assert _create_host(lib, a, len(a), with_index=False)[0] == E_ARG
    assert _create_host(lib, a, -1)[0] == E_ARG
    assert _create_host(lib, None, 5)[0] == E_ARG
    ctx, d = C.addressof(fake_ctx), a.ctypes.data
    assert _create_dev(lib, None, d, len(a))[0] == E_ARG                 # NULL context
    assert _create_dev(lib, None, None, 0)[0] == E_ARG
    assert _create_dev(lib, ctx, d, len(a), with_index=False)[0] == E_ARG
    assert _create_dev(lib, ctx, d, -1)[0] == E_ARG
    assert _create_dev(lib, ctx, None, 5)[0] == E_ARG


def test_decompress_ix_argument_checks(jam, fake_ctx):
    lib = jam.lib()
    a, out = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    ctx, d, o = C.addressof(fake_ctx), a.ctypes.data, out.ctypes.data
    n, h = C.c_int64(0), C.c_void_p()
    call = lib.jpk_dev_jam_cli_decompress_ix
    assert call(None, d, len(a), o, len(out), C.byref(n), None, None, C.byref(h)) == E_ARG      # NULL context
    assert call(ctx, d, -1, o, len(out), C.byref(n), None, None, C.byref(h)) == E_ARG
    assert call(ctx, None, 5, o, len(out), C.byref(n), None, None, C.byref(h)) == E_ARG
    assert call(ctx, d, len(a), None, 5, C.byref(n), None, None, C.byref(h)) == E_ARG
    assert call(ctx, d, len(a), o, -1, C.byref(n), None, None, C.byref(h)) == E_ARG
    assert call(ctx, d, len(a), o, len(out), None, None, None, C.byref(h)) == E_ARG
    assert call(None, d, len(a), o, len(out), C.byref(n), None, None, None) == E_ARG
    assert not out.any() and not h


def _is_empty_cli(jam, h, bad):
    ix = jam.JamIndex(h, bad)
    assert (ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame, ix.kind) == (0, 0, 0, -1, CLI)
    return ix


def test_empty_archive_needs_no_device(jam, fake_ctx):
    lib = jam.lib()
    e = np.zeros(0, dtype=np.uint8)
    rc, h, bad = _create_host(lib, None, 0)
    assert rc == OK
    ix = _is_empty_cli(jam, h, bad)
    rc, h2, bad2 = _create_dev(lib, C.addressof(fake_ctx), None, 0)
    assert rc == OK
    _is_empty_cli(jam, h2, bad2).close()
    assert jam.jam_cli_index(e).kind == CLI
    # reads on the empty index: an empty range is fine, anything beyond raw_len (0) is not
    L, P = C.c_int64 * 1, C.c_void_p * 1
    out = np.zeros(16, dtype=np.uint8)
    st, bf = (C.c_int32 * 1)(7), C.c_int32(7)
    assert lib.jpk_jam_read(ix._h, None, 0, 1, L(0), L(0), P(out.ctypes.data), st, C.byref(bf)) == OK
    assert (st[0], bf.value) == (OK, -1)
    assert lib.jpk_jam_read(ix._h, None, 0, 0, None, None, None, None, None) == OK
    for off, ln in ((0, 1), (1, 0), (5, 3), (-1, 0)):
        assert lib.jpk_jam_read(ix._h, e.ctypes.data, 0, 1, L(off), L(ln), P(out.ctypes.data), st, C.byref(bf)) == E_ARG, (off, ln)
        assert lib.jpk_dev_jam_read(C.addressof(fake_ctx), ix._h, None, 0, 1, L(off), L(ln), P(out.ctypes.data), st, C.byref(bf)) == E_ARG
    assert [len(g) for g in jam.jam_read(e, [(0, 0)], index=ix)] == [0]
    assert not out.any()
    ix.close()
    ix.close()                                             # idempotent


def test_no_device_is_reported_after_the_argument_checks(jam):
    lib = jam.lib()
    a = np.full(64, 0x5A, dtype=np.uint8)
    assert _create_host(lib, a, -1)[0] == E_ARG
    assert _create_host(lib, a, len(a), with_index=False)[0] == E_ARG
    if lib.jpk_device_count() == 0:
        rc, h, _ = _create_host(lib, a, len(a))
        assert rc == E_NODEVICE and not h
        with pytest.raises(jam.JampackError) as e:
            jam.jam_cli_index(a)
        assert e.value.status == E_NODEVICE
