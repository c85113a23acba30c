"""Updating a .jam archive, host side (no GPU): the three entries are declared, exported and bound and the Python names exist; every refused
argument is JPK_E_ARG before a device is looked for; jpk_jam_update_bound is the sum the header states, on oracle-built archives; a host
call that rewrites no frame and has no tail makes no device call, gives jpk_jam_repair's bytes on the undamaged and the damaged archives of
the repair tests and the index jpk_jam_index_create makes of them; a short capacity writes nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jam_resync_model as jm
from test_jam_archive_host import _archive, _slot_cap, hostile_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
OK, E_ARG, E_CAPACITY, E_CORRUPT, E_NODEVICE = 0, -1, -2, -3, -6
SENT = 0xA5
NEW = ("jpk_jam_update_bound", "jpk_dev_jam_update", "jpk_jam_update")


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


@pytest.fixture(scope="module")
def arch(jam, oracle):
    """the archive of test_jam_archive_host: five frames of 6 000 bytes, the last one short (2 345)"""
    data = jam.corpus.make("text", 4 * 6000 + 2345, 71)
    return _archive(oracle, data, MiB, 6000), data


def _i64(v):
    return (C.c_int64 * max(len(v), 1))(*[int(x) for x in v])


def _update(lib, ix_h, a, in_len, off, ln, srcs, out, cap, tail=None, tail_len=0, tail_bs=MiB, flags=0, n=None, ptrs=True, res=(True, True)):
    """jpk_jam_update with host arrays -> (status, out_len, index handle, rewritten, bad frame); the result cells start at -7 / NULL"""
    k = len(off) if n is None else n
    P = (C.c_void_p * max(len(srcs), 1))(*[s.ctypes.data if s is not None else None for s in srcs])
    m, h, rw, bad = C.c_int64(-7), C.c_void_p(), C.c_int32(-7), C.c_int32(-7)
    rc = lib.jpk_jam_update(ix_h, a.ctypes.data if a is not None else None, in_len, k, _i64(off) if ptrs else None, _i64(ln) if ptrs else None, P if ptrs else None,
                            tail.ctypes.data if tail is not None else None, tail_len, tail_bs, flags, 0, out.ctypes.data if out is not None else None, cap,
                            C.byref(m) if res[0] else None, C.byref(h) if res[1] else None, C.byref(rw), C.byref(bad))
    return rc, m.value, h, rw.value, bad.value


def _full(ix):
    return [ix.frame(k) for k in range(ix.frames)], [ix.frame_kind(k) for k in range(ix.frames)], list(ix.gaps), ix.kind, ix.raw_len, ix.archive_len, ix.bad_frame


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS and name in jam.ABI_SYMBOLS, f"{name} has no ctypes signature"
    assert hasattr(jam, "jam_update") and hasattr(jam, "jam_update_bound") and hasattr(jam.Context, "jam_update")
    assert re.search(r"WRITTEN by this call, not decoded\s+\*\s+back", header)           # the contract says what a new index entry vouches for


def test_refused_arguments_are_e_arg_before_a_device_is_looked_for(jam, arch):
    a, data = arch
    lib = jam.lib()
    ix = jam.jam_index(a)
    out = np.full(2 * len(a) + 64, SENT, dtype=np.uint8)
    s = np.arange(64, dtype=np.uint8)
    cap = len(out)
    good = dict(off=[10], ln=[5], srcs=[s])

    def refused(**kw):
        args = dict(good, ix_h=ix._h, a=a, in_len=len(a), out=out, cap=cap)
        args.update(kw)
        rc, m, h, rw, bad = _update(lib, args.pop("ix_h"), args.pop("a"), args.pop("in_len"), args.pop("off"), args.pop("ln"), args.pop("srcs"), args.pop("out"),
                                    args.pop("cap"), **args)
        assert rc == E_ARG, (kw, rc)
        assert (m, bool(h), rw, bad) == (-7, False, -7, -7), kw               # nothing is written, the results included
        if {"off", "ln"} & set(kw) and "flags" not in kw:                                        # what the entry refuses of the writes, the bound refuses
            off, ln = kw.get("off", good["off"]), kw.get("ln", good["ln"])
            assert lib.jpk_jam_update_bound(ix._h, len(off), _i64(off), _i64(ln), 0, MiB) == E_ARG, kw

    # NULL pointers
    refused(ix_h=None)
    refused(a=None)
    refused(out=None)
    refused(res=(False, True))
    refused(res=(True, False))
    refused(ptrs=False)
    refused(srcs=[None])
    refused(tail=None, tail_len=5)
    # not the indexed archive
    refused(in_len=len(a) - 1)
    refused(in_len=len(a) + 1)
    refused(cap=-1)
    refused(n=-1)
    # writes: negative, oversized, outside, overlapping
    refused(off=[-1])
    refused(ln=[-1])
    refused(off=[len(data)], ln=[1])
    refused(off=[len(data) - 4])
    refused(off=[0], ln=[len(data) + 1], srcs=[np.zeros(len(data) + 1, dtype=np.uint8)])
    refused(off=[1 << 62], ln=[1 << 62])
    refused(off=[10, 14], ln=[5, 5], srcs=[s, s])
    refused(off=[10, 10], ln=[5, 5], srcs=[s, s])
    refused(off=[100, 10], ln=[5, 91], srcs=[s, np.zeros(91, dtype=np.uint8)])
    # flags are checked always, also where no frame would use them
    for fl in (2, 3, 6, 7, 8, 1 << 31):
        refused(flags=fl)
        refused(flags=fl, off=[], ln=[], srcs=[])
    # the tail's BlockSize counts only with a tail
    t = np.zeros(8, dtype=np.uint8)
    for bs in (0, -1, MiB - 1, (1000 << 20) + 1):
        refused(tail=t, tail_len=8, tail_bs=bs)
    refused(tail=t, tail_len=-1)
    assert lib.jpk_jam_update_bound(ix._h, 0, None, None, 8, MiB - 1) == E_ARG and lib.jpk_jam_update_bound(ix._h, 0, None, None, -1, MiB) == E_ARG
    assert lib.jpk_jam_update_bound(None, 0, None, None, 0, MiB) == E_ARG and lib.jpk_jam_update_bound(ix._h, 1, None, None, 0, MiB) == E_ARG
    assert lib.jpk_jam_update_bound(ix._h, 0, None, None, 0, 0) == len(a)                     # tail_len == 0 ignores tail_block_size
    assert (out == SENT).all()
    # the device entry without a context, and with the same checks in front of its first device call
    m, h = C.c_int64(-7), C.c_void_p()
    P = (C.c_void_p * 1)(s.ctypes.data)
    assert lib.jpk_dev_jam_update(None, ix._h, a.ctypes.data, len(a), 1, _i64([10]), _i64([5]), P, None, 0, MiB, 0, 0, out.ctypes.data, cap, C.byref(m), C.byref(h),
                                  None, None) == E_ARG and m.value == -7 and not h
    with pytest.raises(jam.JampackError) as err:
        jam.jam_update(a, [(10, s), (12, s)])
    assert err.value.status == E_ARG
    with pytest.raises(jam.JampackError) as err:
        jam.jam_update_bound(ix, [(len(data), 1)])
    assert err.value.status == E_ARG


def test_update_bound_is_the_sum_of_its_parts(jam, arch):
    a, data = arch
    lib = jam.lib()
    ix = jam.jam_index(a)
    span = [15 + ix.frame(k)[3] for k in range(5)]
    raw = [ix.frame(k)[1] for k in range(5)]
    assert raw == [6000] * 4 + [2345] and sum(span) == len(a)
    new = lambda k: 15 + _slot_cap(raw[k])
    b = lambda off, ln, tail=0, bs=MiB, h=ix._h: lib.jpk_jam_update_bound(h, len(off), _i64(off), _i64(ln), tail, bs)
    assert b([], []) == len(a)
    assert b([0, 6000, len(data)], [0, 0, 0]) == len(a)                                       # len == 0 touches nothing
    assert b([0], [1]) == new(0) + sum(span[1:])
    assert b([5999], [1]) == new(0) + sum(span[1:])
    assert b([5999], [2]) == new(0) + new(1) + sum(span[2:])
    assert b([6000], [6000]) == span[0] + new(1) + sum(span[2:])                              # wholly covered: the same bound
    assert b([len(data) - 1, 12000], [1, 1]) == sum(span[:2]) + new(2) + span[3] + new(4)     # any order
    assert b([0], [len(data)]) == sum(new(k) for k in range(5))
    assert b([], [], 1) == len(a) + lib.jpk_jam_compress_bound(1, MiB)
    assert b([7], [3], 5 * MiB // 2, MiB) == new(0) + sum(span[1:]) + lib.jpk_jam_compress_bound(5 * MiB // 2, MiB)
    assert b([], [], 3 * MiB, 2 * MiB) == len(a) + 15 + _slot_cap(2 * MiB) + 15 + _slot_cap(MiB)
    assert jam.jam_update_bound(ix, [(0, 1)]) == b([0], [1]) and jam.jam_update_bound(ix, [(0, b"x")], tail_len=9, block_size=MiB) == b([0], [1], 9)
    # an index of kind 2 over the same (plain) frames: a plain frame stays plain, the tail is staged frames
    sx = jam.jam_staged_index(a)
    assert sx.kind == 2
    assert b([0], [1], h=sx._h) == new(0) + sum(span[1:])
    assert b([], [], 70000, MiB, h=sx._h) == len(a) + lib.jpk_jam_staged_compress_bound(70000, MiB)
    assert lib.jpk_jam_staged_compress_bound(70000, MiB) > lib.jpk_jam_compress_bound(70000, MiB)
    # an empty index: a writer's bound
    e = jam.jam_index(np.zeros(0, dtype=np.uint8))
    assert b([], [], 0, MiB, h=e._h) == 0 and b([0], [0], 3 * MiB + 1, MiB, h=e._h) == lib.jpk_jam_compress_bound(3 * MiB + 1, MiB)
    assert b([0], [1], h=e._h) == E_ARG


def _cases(a):
    return [("undamaged", a), ("deep_flip", jm.deep_flip(a))] + [(n, b) for n, b, _ in hostile_cases(a)] + jm.damage_cases(a)


def test_a_call_that_rewrites_nothing_is_repair_and_makes_no_device_call(jam, arch):
    a, data = arch
    lib = jam.lib()
    seen = 0
    for name, b in _cases(a):
        ix = jam.jam_recover_index(b)
        want = jam.jam_repair(b, ix)
        zero = [(0, b""), (ix.raw_len, b""), (ix.raw_len // 2, b"")]
        for writes in ([], zero):
            got, nix = jam.jam_update(b, writes, ix)
            assert np.array_equal(got, want), name
            assert nix.gaps == [] and nix.bad_frame == -1 and nix.kind == 0, name
            assert _full(nix) == _full(jam.jam_index(got)), name
            assert [nix.frame(k)[:2] for k in range(nix.frames)] == [ix.frame(k)[:2] for k in range(ix.frames)], name       # raw offsets and sizes as in repair
        out = np.full(len(b) + 64, SENT, dtype=np.uint8)
        rc, m, h, rw, bad = _update(lib, ix._h, b if len(b) else None, len(b), [0], [0], [None], out, len(want))            # exact capacity, a NULL source of 0 bytes
        assert (rc, m, rw, bad) == (OK, len(want), 0, -1), name
        lib.jpk_jam_index_destroy(h)
        assert np.array_equal(out[: len(want)], want) and (out[len(want):] == SENT).all(), name
        seen += bool(ix.gaps)
    assert seen >= 15
    # through an index of kind 2 too (the archive has plain frames only: its index is made on the host)
    sx = jam.jam_staged_index(a)
    got, nix = jam.jam_update(a, [(5, b"")], sx)
    assert np.array_equal(got, a) and _full(nix) == _full(jam.jam_staged_index(got)) and nix.kind == 2


def test_a_short_capacity_writes_nothing(jam, arch):
    a, data = arch
    lib = jam.lib()
    b = dict(_cases(a))["magic"]                                       # frame 2 lost: the index holds frames 0, 1, 3, 4
    ix = jam.jam_recover_index(b)
    want = jam.jam_repair(b, ix)
    out = np.full(len(b) + 64, SENT, dtype=np.uint8)
    for cap in (len(want) - 1, 15, 0):
        rc, m, h, rw, bad = _update(lib, ix._h, b, len(b), [], [], [], out, cap)
        assert (rc, m, bool(h), rw) == (E_CAPACITY, len(want), False, 0) and (out == SENT).all(), cap
    # with a frame to rewrite: a capacity that cannot hold the kept frames and the new header is refused before a device is looked for,
    # with the bound as the size to ask for
    s = np.arange(8, dtype=np.uint8)
    bound = lib.jpk_jam_update_bound(ix._h, 1, _i64([3]), _i64([8]), 0, MiB)
    least = len(want) - ix.frame(0)[3]
    rc, m, h, rw, bad = _update(lib, ix._h, b, len(b), [3], [8], [s], out, least - 1)
    assert (rc, m, bool(h), rw) == (E_CAPACITY, bound, False, 1) and (out == SENT).all()
