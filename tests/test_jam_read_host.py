"""Range reads of .jam archives, host side (no GPU): the new entries are exported and bound, the host index of oracle-built archives
(frame table, raw offsets, damaged archives indexed up to the damage), and the argument checks of jpk_jam_read, which come before
any device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_jam_archive_host import _archive, _frame, _starts, hostile_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
NEW = ("jpk_dev_jam_index_create", "jpk_jam_index_create", "jpk_jam_index_info", "jpk_jam_index_frame", "jpk_jam_index_destroy",
       "jpk_dev_jam_read", "jpk_jam_read")
SIZES = [120, 121, 4096, 65535, 65536, 65537, 300000, 130]


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS, f"{name} has no ctypes signature"
    for name in ("JamIndex", "jam_index", "jam_read"):
        assert hasattr(jam, name), name
    for name in ("jam_index", "jam_read"):
        assert hasattr(jam.Context, name), name


@pytest.fixture(scope="module")
def sized(jam, oracle):
    """one frame per entry of SIZES (BlockSize 1 MiB), and the input"""
    data = jam.corpus.make("text", sum(SIZES), 81)
    parts, o = [], 0
    for n in SIZES:
        parts += list(_frame(oracle, data[o: o + n], MiB))
        o += n
    return np.concatenate(parts), data


@pytest.fixture(scope="module")
def arch(jam, oracle):
    """the archive of test_jam_archive_host: five frames of 6 000 bytes, the last one short"""
    data = jam.corpus.make("text", 4 * 6000 + 2345, 71)
    return _archive(oracle, data, MiB, 6000), data


def test_host_index_of_an_archive(jam, sized):
    a, data = sized
    nf, raw, bad = jam.jam_frames(a)
    assert (nf, raw, bad) == (len(SIZES), len(data), -1)
    ix = jam.jam_index(a)
    assert (ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame) == (nf, raw, len(a), -1)
    s = _starts(a)
    ro = 0
    for k, n in enumerate(SIZES):
        psize = int(np.frombuffer(a[s[k] + 7: s[k] + 11].tobytes(), dtype="<i4")[0])
        assert ix.frame(k) == (ro, n, s[k] + 15, psize), k
        ro += n
    ix.close()
    ix.close()                                             # idempotent
    e = jam.jam_index(np.zeros(0, dtype=np.uint8))
    assert (e.frames, e.raw_len, e.archive_len, e.bad_frame) == (0, 0, 0, -1)


def test_index_frame_out_of_range(jam, sized):
    a, _ = sized
    ix = jam.jam_index(a)
    lib = jam.lib()
    for k in (-1, len(SIZES), len(SIZES) + 1, 1 << 30):
        assert lib.jpk_jam_index_frame(ix._h, k, None, None, None, None) == -1, k
    assert lib.jpk_jam_index_frame(ix._h, len(SIZES) - 1, None, None, None, None) == 0
    assert lib.jpk_jam_index_frame(None, 0, None, None, None, None) == -1
    assert lib.jpk_jam_index_info(None, None, None, None) == -1
    with pytest.raises(jam.JampackError) as e:
        ix.frame(len(SIZES))
    assert e.value.status == -1


def test_index_of_hostile_archives(jam, arch):
    """an index over exactly the prefix jpk_jam_frames reports, JPK_OK, the same bad frame"""
    a, data = arch
    lib = jam.lib()
    for name, b, k in hostile_cases(a):
        nf, raw, bad = jam.jam_frames(b)
        assert bad == k, name
        h, bf = C.c_void_p(), C.c_int32(-7)
        assert lib.jpk_jam_index_create(b.ctypes.data, len(b), C.byref(h), C.byref(bf)) == 0, name
        ix = jam.JamIndex(h, bf.value)
        assert (ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame) == (nf, raw, len(b), k), name
        for f in range(nf):
            assert ix.frame(f)[:2] == (6000 * f, min(6000, len(data) - 6000 * f)), (name, f)
        ix.close()


def _read(lib, ix, a, in_len, off, ln):
    out = np.zeros(64, dtype=np.uint8)
    L, P = C.c_int64 * len(off), C.c_void_p * len(off)
    st, bad = (C.c_int32 * len(off))(), C.c_int32(0)
    rc = lib.jpk_jam_read(ix._h, a.ctypes.data, in_len, len(off), L(*off), L(*ln), P(*[out.ctypes.data] * len(off)), st, C.byref(bad))
    assert not out.any()                                   # nothing written
    return rc


def test_read_argument_checks_need_no_device(jam, sized):
    a, data = sized
    ix = jam.jam_index(a)
    lib = jam.lib()
    raw = len(data)
    assert _read(lib, ix, a, len(a), [raw - 3], [4]) == -1               # one byte past raw_len
    assert _read(lib, ix, a, len(a), [raw + 1], [0]) == -1
    assert _read(lib, ix, a, len(a), [-1], [4]) == -1
    assert _read(lib, ix, a, len(a), [0], [-1]) == -1
    assert _read(lib, ix, a, len(a), [0, 5, 1 << 62], [0, 0, 1 << 62]) == -1   # off + len would overflow
    assert _read(lib, ix, a, len(a) - 1, [0], [4]) == -1                  # not the index's archive length
    assert _read(lib, ix, a, len(a) + 1, [0], [4]) == -1
    assert lib.jpk_jam_read(None, a.ctypes.data, len(a), 0, None, None, None, None, None) == -1
    assert lib.jpk_dev_jam_read(None, ix._h, None, len(a), 0, None, None, None, None, None) == -1
    # legal and without work: no range, and empty ranges anywhere in [0, raw_len]
    assert lib.jpk_jam_read(ix._h, a.ctypes.data, len(a), 0, None, None, None, None, None) == 0
    assert _read(lib, ix, a, len(a), [0, raw, 77], [0, 0, 0]) == 0
    assert [len(g) for g in jam.jam_read(a, [(0, 0), (raw, 0)])] == [0, 0]
    with pytest.raises(jam.JampackError) as e:
        jam.jam_read(a, [(raw, 1)], index=ix)
    assert e.value.status == -1

