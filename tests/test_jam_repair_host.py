"""Repair of damaged .jam archives and the argument checks of a stock-CLI recover, host side (no GPU): jpk_jam_repair copies the spans of
the kept frames of an index back to back -- on the oracle-built archives and the damage of the recover tests the result is the
concatenation of those spans and indexes cleanly, a frame_status drops frames, a short capacity writes nothing --, the new entries are
exported and bound, and jpk_jam_index_recover takes kind 1 with verify 1, checking its arguments before it looks for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jam_resync_model as jm
from test_jam_archive_host import _archive, hostile_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
OK, E_ARG, E_CAPACITY, E_CORRUPT = 0, -1, -2, -3
SENT = 0xA5
NEW = ("jpk_dev_jam_repair", "jpk_jam_repair")


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


@pytest.fixture(scope="module")
def arch(jam, oracle):
    """the archive of test_jam_archive_host: five frames of 6 000 bytes, the last one short"""
    data = jam.corpus.make("text", 4 * 6000 + 2345, 71)
    return _archive(oracle, data, MiB, 6000), data


def _cases(a):
    return [("undamaged", a), ("deep_flip", jm.deep_flip(a))] + [(n, b) for n, b, _ in hostile_cases(a)] + jm.damage_cases(a)


def _spans(b, ix, keep=None):
    ks = range(ix.frames) if keep is None else keep
    parts = [b[ix.frame(k)[2] - 15: ix.frame(k)[2] + ix.frame(k)[3]] for k in ks]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS and name in jam.ABI_SYMBOLS, f"{name} has no ctypes signature"
    assert hasattr(jam, "jam_repair") and hasattr(jam.Context, "jam_repair")
    assert "continuing it is future work" not in header


def test_repair_is_the_kept_frames_back_to_back(jam, arch):
    a, data = arch
    seen = 0
    for name, b in _cases(a):
        ix = jam.jam_recover_index(b)
        out = jam.jam_repair(b, ix)
        assert np.array_equal(out, _spans(b, ix)), name
        rix = jam.jam_index(out)
        assert rix.bad_frame == -1 and rix.frames == ix.frames and rix.archive_len == len(out), name
        assert [rix.frame(k)[1::2] for k in range(rix.frames)] == [ix.frame(k)[1::2] for k in range(ix.frames)], name       # (raw, psize)
        assert [rix.frame(k)[0] for k in range(rix.frames)] == [ix.frame(k)[0] for k in range(ix.frames)], name             # raw offsets
        if not ix.gaps:
            assert np.array_equal(out, b), name
        seen += bool(ix.gaps)
    assert seen >= 15
    # an undamaged archive through the index of a plain creator: itself
    assert np.array_equal(jam.jam_repair(a, jam.jam_index(a)), a)


def test_a_frame_status_drops_exactly_the_frames_it_fails(jam, arch):
    a, data = arch
    b = dict(_cases(a))["magic"]                                       # frame 2 lost: the index holds frames 0, 1, 3, 4
    ix = jam.jam_recover_index(b)
    assert ix.frames == 4
    for drop in range(4):
        st = [OK] * 4
        st[drop] = E_CORRUPT
        out = jam.jam_repair(b, ix, st)
        assert np.array_equal(out, _spans(b, ix, [k for k in range(4) if k != drop])), drop
        rix = jam.jam_index(out)
        assert rix.bad_frame == -1 and rix.frames == 3
    assert len(jam.jam_repair(b, ix, [E_CORRUPT] * 4)) == 0
    assert np.array_equal(jam.jam_repair(b, ix, [OK] * 4), jam.jam_repair(b, ix))
    with pytest.raises(ValueError):
        jam.jam_repair(b, ix, [OK] * 3)


def _repair(lib, h, p, in_len, st, out, cap, n=True, k=True):
    n_, k_ = C.c_int64(-7), C.c_int32(-7)
    rc = lib.jpk_jam_repair(h, p, in_len, st, out.ctypes.data if out is not None else None, cap, C.byref(n_) if n else None, C.byref(k_) if k else None)
    return rc, n_.value, k_.value


def test_capacity_and_argument_checks(jam, arch):
    a, data = arch
    lib = jam.lib()
    b = dict(_cases(a))["magic"]
    ix = jam.jam_recover_index(b)
    want = _spans(b, ix)
    out = np.full(len(b) + 64, SENT, dtype=np.uint8)
    # one byte short: the size needed, nothing written
    assert _repair(lib, ix._h, b.ctypes.data, len(b), None, out, len(want) - 1) == (E_CAPACITY, len(want), 4)
    assert (out == SENT).all()
    assert _repair(lib, ix._h, b.ctypes.data, len(b), None, out, 0) == (E_CAPACITY, len(want), 4) and (out == SENT).all()
    # exact capacity: the bytes, and nothing behind them
    assert _repair(lib, ix._h, b.ctypes.data, len(b), None, out, len(want)) == (OK, len(want), 4)
    assert np.array_equal(out[: len(want)], want) and (out[len(want):] == SENT).all()
    assert _repair(lib, ix._h, b.ctypes.data, len(b), None, out, len(want), k=False)[:2] == (OK, len(want))       # frames may be NULL
    st = (C.c_int32 * 4)(OK, E_CORRUPT, OK, OK)
    assert _repair(lib, ix._h, b.ctypes.data, len(b), st, out, len(out)) == (OK, len(want) - 15 - ix.frame(1)[3], 3)
    # arguments
    assert _repair(lib, None, b.ctypes.data, len(b), None, out, len(out))[0] == E_ARG
    assert _repair(lib, ix._h, b.ctypes.data, len(b) - 1, None, out, len(out))[0] == E_ARG                         # not the indexed archive
    assert _repair(lib, ix._h, b.ctypes.data, len(b) + 1, None, out, len(out))[0] == E_ARG
    assert _repair(lib, ix._h, b.ctypes.data, len(b), None, out, len(out), n=False)[0] == E_ARG
    assert _repair(lib, ix._h, None, len(b), None, out, len(out))[0] == E_ARG
    assert _repair(lib, ix._h, b.ctypes.data, len(b), None, None, len(out))[0] == E_ARG
    assert _repair(lib, ix._h, b.ctypes.data, len(b), None, out, -1)[0] == E_ARG
    n = C.c_int64(-7)
    assert lib.jpk_dev_jam_repair(None, ix._h, b.ctypes.data, len(b), None, out.ctypes.data, len(out), C.byref(n), None) == E_ARG and n.value == -7


def test_an_empty_index_gives_no_bytes(jam, arch):
    a, data = arch
    lib = jam.lib()
    for b in (a[:14].copy(), a[:0].copy()):
        ix = jam.jam_recover_index(b)
        assert ix.frames == 0 and len(jam.jam_repair(b, ix)) == 0
        assert _repair(lib, ix._h, b.ctypes.data if len(b) else None, len(b), None, None, 0) == (OK, 0, 0)


# ---- a stock-CLI recover: the arguments, before a device is looked for -------------------------------------------------------------------
def _recover(lib, a, in_len, kind, verify, h=True):
    hp, gp = C.c_void_p(), C.c_int32(-7)
    rc = lib.jpk_jam_index_recover(a.ctypes.data if a is not None else None, in_len, kind, verify, C.byref(hp) if h else None, C.byref(gp))
    kind_of = lib.jpk_jam_index_kind(hp) if hp else None
    frames = C.c_int32(-7)
    if hp:
        lib.jpk_jam_index_info(hp, C.byref(frames), None, None)
        lib.jpk_jam_index_destroy(hp)
    return rc, gp.value, kind_of, frames.value


def test_kind_1_recover_argument_checks(jam, arch):
    a, data = arch
    lib = jam.lib()
    assert _recover(lib, None, 0, 1, 1) == (OK, 0, 1, 0)               # an empty index of kind 1, no gap, no device
    assert _recover(lib, a, len(a), 1, 1, h=False)[0] == E_ARG
    assert _recover(lib, None, len(a), 1, 1)[0] == E_ARG
    assert _recover(lib, a, -1, 1, 1)[0] == E_ARG
    assert _recover(lib, a, len(a), 1, 2)[0] == E_ARG
    assert _recover(lib, a, len(a), 1, 0)[0] == E_ARG                  # a stock-CLI index is always verified
    assert lib.jpk_dev_jam_index_recover(None, a.ctypes.data, len(a), 1, 1, C.byref(C.c_void_p()), None) == E_ARG
    # verify=None is the kind's own value
    e = np.zeros(0, dtype=np.uint8)
    ix = jam.jam_recover_index(e, jam.JAM_INDEX_CLI)
    assert (ix.kind, ix.frames, ix.gaps, ix.raw_len, ix.archive_len, ix.bad_frame) == (1, 0, [], 0, 0, -1)
    assert jam.jam_recover_index(e, jam.JAM_INDEX_STAGED).kind == 2 and jam.jam_recover_index(e).kind == 0
    with pytest.raises(jam.JampackError) as err:
        jam.jam_recover_index(e, jam.JAM_INDEX_CLI, False)
    assert err.value.status == E_ARG
    got, status = jam.jam_salvage(e, kind=jam.JAM_INDEX_CLI)
    assert len(got) == 0 and status == []
    # bytes without a structurally valid stock-CLI frame: one gap, and no device was looked for
    ix = jam.jam_recover_index(a[:14], jam.JAM_INDEX_CLI)
    assert (ix.kind, ix.frames, ix.gaps) == (1, 0, [(0, 14, 0, jam.JAM_GAP_NOFRAME)])
    junk = np.frombuffer(b"JAMJAMJAM" * 20, dtype=np.uint8)
    ix = jam.jam_recover_index(junk, jam.JAM_INDEX_CLI)
    assert (ix.kind, ix.frames, ix.gaps) == (1, 0, [(0, len(junk), 0, jam.JAM_GAP_NOFRAME)])
