"""The index and the range reads of archives with staged frames, host side: the new entries are declared, exported and bound; their
argument checks come before a device is looked for; the empty archive; the host creator on archives whose payloads the oracle's C
restatement makes -- an archive of plain frames is indexed without a device, one with a staged frame needs one --; and jpk_lz77_size.
The device side is test_gpu_jam_staged_read.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from jam_staged_cases import MiB, STAGED, s2_stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_CAPACITY, E_CORRUPT, E_NODEVICE = 0, -1, -2, -3, -6
NEW = ("jpk_lz77_size", "jpk_dev_blocks_lz77_sizes", "jpk_dev_jam_staged_index_create", "jpk_jam_staged_index_create", "jpk_dev_jam_staged_decompress_ix",
       "jpk_jam_index_frame_kind")


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    hdr = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", hdr), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS and name in jam.ABI_SYMBOLS, f"{name} has no ctypes signature"
    for name in ("jam_staged_index", "jam_staged_decompress_ix", "blocks_lz77_sizes"):
        assert hasattr(jam.Context, name), name
    for name in ("jam_staged_index", "lz77_size"):
        assert hasattr(jam, name), name
    assert hasattr(jam.JamIndex, "frame_kind")
    assert re.search(r"#define\s+JPK_JAM_INDEX_STAGED\s+2\b", hdr) and jam.JAM_INDEX_STAGED == 2
    assert "do not exist" not in hdr
    names = [jam.lib().jpk_ctx_profile_name(i).decode() for i in range(jam.lib().jpk_ctx_profile_count())]
    assert names.index("k_lz77_sizes") == names.index("k_lzx_plan") + 1          # a profile id of its own, next to the plan's


def test_argument_checks_come_before_the_device(jam):
    lib = jam.lib()
    a, out = np.zeros(64, dtype=np.uint8), np.zeros(4096, dtype=np.uint8)
    ap, op = a.ctypes.data, out.ctypes.data
    n32, n64, h = C.c_int32(0), C.c_int64(0), C.c_void_p()
    ctx = C.c_void_p(1)                                                # never looked into: every call below is refused for its arguments
    for verify in (0, 1):
        for args in ((ap, -1, verify, C.byref(h), None), (None, 64, verify, C.byref(h), None), (ap, 64, verify, None, None)):
            assert lib.jpk_jam_staged_index_create(*args) == E_ARG, args
            assert lib.jpk_dev_jam_staged_index_create(ctx, *args) == E_ARG, args
        assert lib.jpk_dev_jam_staged_index_create(None, ap, 64, verify, C.byref(h), None) == E_ARG          # no context
        assert lib.jpk_dev_jam_staged_index_create(None, None, 0, verify, C.byref(h), None) == E_ARG
    for verify in (-1, 2):
        assert lib.jpk_jam_staged_index_create(ap, 64, verify, C.byref(h), None) == E_ARG
        assert lib.jpk_jam_staged_index_create(None, 0, verify, C.byref(h), None) == E_ARG
        assert lib.jpk_dev_jam_staged_index_create(ctx, ap, 64, verify, C.byref(h), None) == E_ARG
    assert not h
    for args in ((ap, -1, op, 4096, C.byref(n64), None, None), (ap, 64, op, -1, C.byref(n64), None, None), (ap, 64, op, 4096, None, None, None),
                 (None, 64, op, 4096, C.byref(n64), None, None), (ap, 64, None, 4096, C.byref(n64), None, None)):
        assert lib.jpk_dev_jam_staged_decompress_ix(ctx, *args, C.byref(h)) == E_ARG, args
        assert lib.jpk_dev_jam_staged_decompress_ix(None, *args, None) == E_ARG, args
    assert lib.jpk_dev_jam_staged_decompress_ix(None, ap, 64, op, 4096, C.byref(n64), None, None, C.byref(h)) == E_ARG
    P, I = C.c_void_p * 1, C.c_int32 * 1
    ins, il, oc, ol = P(ap), I(64), I(4096), I(0)
    assert lib.jpk_dev_blocks_lz77_sizes(None, 1, ins, il, oc, ol, None) == E_ARG
    assert lib.jpk_dev_blocks_lz77_sizes(None, 0, None, None, None, None, None) == E_ARG
    for args in ((-1, ins, il, oc, ol), (1, None, il, oc, ol), (1, ins, None, oc, ol), (1, ins, il, None, ol), (1, ins, il, oc, None),
                 (1, ins, I(-1), oc, ol), (1, ins, il, I(-1), ol), (1, P(None), il, oc, ol)):
        assert lib.jpk_dev_blocks_lz77_sizes(ctx, *args, None) == E_ARG, args
    for args in ((ap, -1, 64, C.byref(n32)), (None, 2, 64, C.byref(n32)), (ap, 2, -1, C.byref(n32)), (ap, 2, 64, None)):
        assert lib.jpk_lz77_size(*args) == E_ARG, args
    assert lib.jpk_jam_index_frame_kind(None, 0) == E_ARG


def test_empty_archive_gives_an_empty_index_without_a_device(jam):
    lib = jam.lib()
    for verify in (False, True):
        ix = jam.jam_staged_index(np.zeros(0, dtype=np.uint8), verify=verify)
        assert (ix.kind, ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame) == (2, 0, 0, 0, -1)
        assert lib.jpk_jam_index_frame_kind(ix._h, 0) == E_ARG and lib.jpk_jam_index_frame_kind(ix._h, -1) == E_ARG
        assert lib.jpk_jam_read(ix._h, None, 0, 0, None, None, None, None, None) == OK
        assert jam.jam_read(np.zeros(0, dtype=np.uint8), [], index=ix) == []
        L, P = C.c_int64 * 1, C.c_void_p * 1
        assert lib.jpk_jam_read(ix._h, None, 0, 1, L(0), L(0), P(None), None, None) == OK          # a zero-length range at raw_len
        assert lib.jpk_jam_read(ix._h, None, 0, 1, L(0), L(1), P(None), None, None) == E_ARG
        ix.close()
    # the device creator looks for no device either (the context is never looked into)
    h, bad = C.c_void_p(), C.c_int32(7)
    assert lib.jpk_dev_jam_staged_index_create(C.c_void_p(1), None, 0, 0, C.byref(h), C.byref(bad)) == OK and h and bad.value == -1
    assert lib.jpk_jam_index_kind(h) == 2
    lib.jpk_jam_index_destroy(h)


# ---- the host creator on archives whose payloads the oracle makes (the frame_of recipe of test_jam_staged_host.py) ---------------------
def frame_of(oracle, r, block_size, staged):
    body = oracle.compress_block(s2_stored(r) if staged else np.asarray(r, dtype=np.uint8))
    return np.concatenate([np.frombuffer(oracle.block_header(oracle.checksum(r), len(body), block_size | (STAGED if staged else 0)), dtype=np.uint8), body])


@pytest.fixture(scope="module")
def texts(jam):
    return [jam.corpus.make("text", n, 30 + i) for i, n in enumerate((5000, 7000))]


def _table(ix):
    return [ix.frame(k) for k in range(ix.frames)]


def test_plain_archive_is_indexed_on_the_host_alone(jam, oracle, texts):
    """no device call: this test runs where there is no GPU"""
    arch = np.concatenate([frame_of(oracle, t, MiB, False) for t in texts])
    plain = jam.jam_index(arch)
    for verify in (False, True):
        ix = jam.jam_staged_index(arch, verify=verify)
        assert (ix.kind, ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame) == (2, 2, 12000, len(arch), -1)
        assert _table(ix) == _table(plain) and [f[:2] for f in _table(ix)] == [(0, 5000), (5000, 7000)]
        assert [ix.frame_kind(k) for k in range(2)] == [0, 0]
        with pytest.raises(jam.JampackError):
            ix.frame_kind(2)
    assert plain.kind == 0 and plain.frame_kind(1) == 0                # the other kinds answer with the index's own
    # trailing bytes are a bad frame 2; the frames in front of it are indexed
    ix = jam.jam_staged_index(np.concatenate([arch, arch[:9]]))
    assert (ix.frames, ix.raw_len, ix.bad_frame, ix.archive_len) == (2, 12000, 2, len(arch) + 9)


def test_a_staged_frame_needs_a_device(jam, oracle, texts):
    lib = jam.lib()
    arch = np.concatenate([frame_of(oracle, texts[0], MiB, False), frame_of(oracle, texts[1], MiB, True)])
    assert jam.jam_staged_frames(arch) == (2, 5000 + MiB, -1)
    # the creators of the other kinds go on refusing the staged frame
    assert jam.jam_index(arch).bad_frame == 1
    if lib.jpk_device_count() == 0:
        h = C.c_void_p()
        for verify in (0, 1):
            assert lib.jpk_jam_staged_index_create(arch.ctypes.data, len(arch), verify, C.byref(h), None) == E_NODEVICE and not h


def test_lz77_size_of_the_stored_form(jam, texts):
    r = texts[0]
    s1 = np.concatenate([np.array([0x04, 0x80], dtype=np.uint8), r])
    assert jam.lz77_size(s1, len(r)) == jam.lz77_size(s1, MiB) == len(r) == len(jam.Lz77().Decompress(s1, len(r)))
    n = C.c_int32(5)
    assert jam.lib().jpk_lz77_size(s1.ctypes.data, len(s1), len(r) - 1, C.byref(n)) == E_CAPACITY and n.value == 0
    assert jam.lz77_size(s1[:2], 0) == 0 and jam.lz77_size(np.zeros(0, dtype=np.uint8), 0) == 0
    assert jam.lib().jpk_lz77_size(s1.ctypes.data, 1, 64, C.byref(n)) == E_CORRUPT         # a token cut off behind its first byte
