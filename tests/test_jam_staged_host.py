"""Staged frames, host side: the argument checks of the new entries (which come before a device is looked for), the bounds, and the host
walk jpk_jam_staged_frames on archives of plain and staged frames whose payloads the oracle's C restatement makes, so the walk is tested
without a GPU.

The frame entries jpk_jam_staged_block_write / _read stage through the GPU (ForwardBwt + Ans::Encode), as jpk_jam_cli_block_write does:
without a device they answer JPK_E_NODEVICE, which is all this file can hold them to.  Their bytes -- the header, the stored S2, the
reference's stage decoders, the read -- are checked in test_gpu_jam_staged.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from jam_staged_cases import FLAGS, MiB, STAGED, s2_stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_CAPACITY, E_CORRUPT, E_NODEVICE = 0, -1, -2, -3, -6
BAD_FLAGS = (2, 3, 6, 8, 0x80000000)
NEW = ("jpk_jam_staged_block_write", "jpk_jam_staged_block_read", "jpk_jam_staged_compress_bound", "jpk_dev_jam_staged_compress", "jpk_jam_staged_compress",
       "jpk_jam_staged_frames", "jpk_dev_jam_staged_decompress", "jpk_jam_staged_decompress", "jpk_dev_blocks_lz77_expand", "jpk_debug_lz77_expand_last")


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
    for name in ("jam_staged_compress", "jam_staged_decompress", "blocks_lz77_expand"):
        assert hasattr(jam.Context, name), name
    for name in ("jam_staged_compress", "jam_staged_decompress", "jam_staged_frames", "jam_staged_block_write", "jam_staged_block_read"):
        assert hasattr(jam, name), name
    assert re.search(r"#define\s+JPK_JAM_STAGED\s+\(1 << 30\)", hdr) and jam.JAM_STAGED == STAGED
    assert (1000 << 20) < STAGED                                       # MAX_BLOCKSIZE leaves the bit free


def test_argument_checks_come_before_the_device(jam):
    lib = jam.lib()
    a, out = np.zeros(64, dtype=np.uint8), np.zeros(4096, dtype=np.uint8)
    n32, n64, used = C.c_int32(0), C.c_int64(0), C.c_int32(0)
    ap, op = a.ctypes.data, out.ctypes.data
    for fl in BAD_FLAGS:
        assert lib.jpk_jam_staged_block_write(ap, 64, MiB, op, 4096, C.byref(n32), fl) == E_ARG, fl
        assert lib.jpk_jam_staged_compress(ap, 64, MiB, op, 4096, C.byref(n64), 0, fl) == E_ARG, fl
        assert lib.jpk_dev_jam_staged_compress(None, ap, 64, MiB, op, 4096, C.byref(n64), 0, fl) == E_ARG, fl
    for fl in FLAGS:
        for args in ((ap, -1, MiB, op, 4096, C.byref(n32)), (None, 64, MiB, op, 4096, C.byref(n32)), (ap, 64, MiB, None, 4096, C.byref(n32)),
                     (ap, 64, MiB, op, 4096, None), (ap, 64, MiB, op, -1, C.byref(n32)), (ap, 64, MiB - 1, op, 4096, C.byref(n32)),
                     (ap, 64, (1000 << 20) + 1, op, 4096, C.byref(n32)), (ap, 64, MiB | STAGED, op, 4096, C.byref(n32))):
            assert lib.jpk_jam_staged_block_write(*args, fl) == E_ARG, (args, fl)
        assert lib.jpk_jam_staged_block_write(ap, 64, MiB, op, 14, C.byref(n32), fl) == E_CAPACITY
        for args in ((ap, -1, MiB, op, 4096, C.byref(n64), 0), (ap, 64, MiB, op, -1, C.byref(n64), 0), (ap, 64, MiB, op, 4096, None, 0),
                     (None, 64, MiB, op, 4096, C.byref(n64), 0), (ap, 64, MiB, None, 4096, C.byref(n64), 0), (ap, 64, MiB - 1, op, 4096, C.byref(n64), 0),
                     (ap, 64, (1000 << 20) + 1, op, 4096, C.byref(n64), 0)):
            assert lib.jpk_jam_staged_compress(*args, fl) == E_ARG, (args, fl)
    big = np.zeros(MiB + 1, dtype=np.uint8)
    assert lib.jpk_jam_staged_block_write(big.ctypes.data, MiB + 1, MiB, op, 4096, C.byref(n32), 0) == E_ARG          # in_len > block_size
    for args in ((None, 64, op, 4096, C.byref(n32), C.byref(used)), (ap, 64, None, 4096, C.byref(n32), C.byref(used)), (ap, 64, op, 4096, None, C.byref(used)),
                 (ap, -1, op, 4096, C.byref(n32), C.byref(used)), (ap, 64, op, -1, C.byref(n32), C.byref(used))):
        assert lib.jpk_jam_staged_block_read(*args) == E_ARG, args
    assert lib.jpk_jam_staged_block_read(ap, 14, op, 4096, C.byref(n32), C.byref(used)) == E_CORRUPT
    for args in ((ap, -1, op, 4096, C.byref(n64), None, None), (ap, 64, op, -1, C.byref(n64), None, None), (ap, 64, op, 4096, None, None, None),
                 (None, 64, op, 4096, C.byref(n64), None, None), (ap, 64, None, 4096, C.byref(n64), None, None)):
        assert lib.jpk_jam_staged_decompress(*args) == E_ARG, args
        assert lib.jpk_dev_jam_staged_decompress(None, *args) == E_ARG, args
    assert lib.jpk_dev_jam_staged_decompress(None, ap, 64, op, 4096, C.byref(n64), None, None) == E_ARG               # no context
    assert lib.jpk_jam_staged_frames(ap, -1, None, None, None) == lib.jpk_jam_staged_frames(None, 64, None, None, None) == E_ARG
    assert lib.jpk_jam_staged_frames(None, 0, None, None, None) == OK
    P, I = C.c_void_p * 1, C.c_int32 * 1
    ins, outs, il, oc, ol = P(ap), P(op), I(64), I(4096), I(0)
    assert lib.jpk_dev_blocks_lz77_expand(None, 1, ins, il, outs, oc, ol, None) == E_ARG
    assert lib.jpk_dev_blocks_lz77_expand(None, 0, None, None, None, None, None, None) == E_ARG
    assert lib.jpk_debug_lz77_expand_last(None, C.byref(n32), C.byref(used)) == E_ARG
    for args in ((-1, MiB), (64, MiB - 1), (64, (1000 << 20) + 1), (64, MiB | STAGED)):
        assert lib.jpk_jam_staged_compress_bound(*args) == E_ARG
    assert lib.jpk_jam_staged_compress_bound(0, MiB) == 0
    if lib.jpk_device_count() == 0:
        assert lib.jpk_jam_staged_compress(ap, 64, MiB, op, 4096, C.byref(n64), 0, 5) == E_NODEVICE
        assert lib.jpk_jam_staged_block_write(ap, 64, MiB, op, 4096, C.byref(n32), 1) == E_NODEVICE
        assert lib.jpk_jam_staged_compress(ap, 0, MiB, op, 4096, C.byref(n64), 0, 0) == lib.jpk_jam_compress(ap, 0, MiB, op, 4096, C.byref(n64), 0)


def test_the_bound_counts_the_stage_chain(jam):
    """a slice gives at most jpk_cli_stages_bound bytes of BWT input, as a frame of the stock-CLI writer does"""
    for n, bs in ((1, MiB), (MiB, MiB), (3 * MiB + 5, MiB), (20 * MiB, 8 * MiB)):
        full, rest = divmod(n, bs)
        assert jam.jam_staged_compress_bound(n, bs) == jam.jam_cli_compress_bound(n, bs) > n + 15 * (full + (1 if rest else 0))


# ---- the walk: archives whose payloads the oracle makes ---------------------------------------------------------------------------
def frame_of(oracle, r, block_size, staged):
    body = oracle.compress_block(s2_stored(r) if staged else np.asarray(r, dtype=np.uint8))
    return np.concatenate([np.frombuffer(oracle.block_header(oracle.checksum(r), len(body), block_size | (STAGED if staged else 0)), dtype=np.uint8), body])


@pytest.fixture(scope="module")
def walk_frames(jam, oracle):
    t = [jam.corpus.make("text", n, 30 + i) for i, n in enumerate((5000, 3000, 7000, 100))]
    return t, [frame_of(oracle, t[0], MiB, False), frame_of(oracle, t[1], 2 * MiB, True), frame_of(oracle, t[2], MiB, False), frame_of(oracle, t[3], MiB, True)]


def test_walk_of_plain_and_staged_frames(jam, walk_frames):
    t, (p0, s1, p2, s3) = walk_frames
    # plain | staged (shorter than its BlockSize) | plain: the staged frame counts at its BlockSize
    assert jam.jam_staged_frames(np.concatenate([p0, s1, p2])) == (3, 5000 + 2 * MiB + 7000, -1)
    assert jam.jam_staged_frames(np.concatenate([s1, s3])) == (2, 3 * MiB, -1)
    assert jam.jam_staged_frames(p0) == jam.jam_frames(p0) == (1, 5000, -1)
    assert jam.jam_staged_frames(np.zeros(0, dtype=np.uint8)) == (0, 0, -1)
    # the plain and the stock-CLI walk refuse the staged frame
    arch = np.concatenate([p0, s1, p2])
    assert jam.jam_frames(arch) == (1, 5000, 1)
    assert jam.jam_cli_frames(arch) == (1, MiB, 1)
    assert jam.jam_frames(s1) == (0, 0, 0) and jam.jam_cli_frames(s1) == (0, 0, 0)
    for extra in range(1, 15):
        assert jam.jam_staged_frames(np.concatenate([arch, arch[:extra]])) == (3, 5000 + 2 * MiB + 7000, 3), extra


def test_walk_refuses_bad_block_size_fields(jam, walk_frames):
    _, (p0, s1, p2, _) = walk_frames

    def with_field(f, field):
        g = f.copy()
        g[11:15] = np.frombuffer(struct.pack("<I", field & 0xFFFFFFFF), dtype=np.uint8)
        return g
    for field in (MiB | STAGED | (1 << 31), MiB | (1 << 31), (MiB - 1) | STAGED, ((1000 << 20) + 1) | STAGED, STAGED, 0):
        assert jam.jam_staged_frames(np.concatenate([p0, with_field(s1, field), p2])) == (1, 5000, 1), hex(field)
    assert jam.jam_staged_frames(np.concatenate([p0, with_field(s1, (1000 << 20) | STAGED), p2]))[0] == 3
