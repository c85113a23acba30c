"""Whole .jam archives, host side (no GPU): the archive entries are exported and bound, jpk_jam_compress_bound's arithmetic, and the
frame walk of jpk_jam_frames on archives built from the oracle -- the validation rules the device walk of jpk_dev_jam_decompress
shares (DecompReadBlock, jampack.cpp:140-163)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
NEW = ("jpk_dev_checksums", "jpk_jam_compress_bound", "jpk_dev_jam_compress", "jpk_dev_jam_decompress", "jpk_jam_compress",
       "jpk_jam_decompress", "jpk_jam_frames")


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


def _slot_cap(n):
    """the payload slot of a frame of n input bytes (abi_multi.hip jpk_multi_comp_cap, which jam_archive.hip sizes the frames with)"""
    m = n + 480
    return m * 5 // 4 + 4096 + 1400 * (m // MiB + 1)


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS, f"{name} has no ctypes signature"


def test_compress_bound(jam):
    b = jam.lib().jpk_jam_compress_bound
    assert b(0, MiB) == 0
    assert b(1, MiB) == 15 + _slot_cap(1)
    assert b(MiB, MiB) == 15 + _slot_cap(MiB)
    assert b(3 * MiB + 12345, MiB) == 3 * (15 + _slot_cap(MiB)) + 15 + _slot_cap(12345)
    big = (5 << 30) + 7                                  # above 2^31: 64-bit arithmetic
    bs = 64 * MiB
    assert b(big, bs) == (big // bs) * (15 + _slot_cap(bs)) + 15 + _slot_cap(big % bs)
    assert b(big, bs) > big
    assert b(-1, MiB) < 0 and b(10, MiB - 1) < 0 and b(10, (1000 << 20) + 1) < 0
    assert jam.jam_compress_bound(0) == 0


def _frame(oracle, t, bs):
    p = oracle.compress_block(t)
    return np.frombuffer(oracle.block_header(oracle.checksum(t), len(p), bs), dtype=np.uint8), p


def _archive(oracle, data, bs, step):
    parts = []
    for o in range(0, len(data), step):
        h, p = _frame(oracle, data[o: o + step], bs)
        parts += [h, p]
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def arch(jam, oracle):
    """five frames of 6 000 bytes (the last one short) with BlockSize 1 MiB, and their input"""
    data = jam.corpus.make("text", 4 * 6000 + 2345, 71)
    return _archive(oracle, data, MiB, 6000), data


def _starts(a):
    o, s = 0, []
    while o < len(a):
        s.append(o)
        o += 15 + int(np.frombuffer(a[o + 7: o + 11].tobytes(), dtype="<i4")[0])
    return s


def test_frames_count_and_raw_length(jam, arch):
    a, data = arch
    assert jam.jam_frames(a) == (5, len(data), -1)
    assert jam.jam_frames(np.zeros(0, dtype=np.uint8)) == (0, 0, -1)


def test_frames_of_two_concatenated_archives(jam, oracle, arch):
    a, data = arch
    d2 = jam.corpus.make("random", 9000, 72)
    b = _archive(oracle, d2, 8 * MiB, 4000)                 # other block size, three frames
    assert jam.jam_frames(np.concatenate([a, b])) == (8, len(data) + len(d2), -1)


def _put_i32(a, at, v):
    a[at: at + 4] = np.frombuffer(np.int32(v).tobytes(), dtype=np.uint8)


def hostile_cases(a):
    """(name, archive, bad frame) -- the frame walk must stop at exactly that frame"""
    s = _starts(a)
    out = []
    k = 2
    b = a.copy(); b[s[k]] ^= 1
    out.append(("magic", b, k))
    b = a.copy(); _put_i32(b, s[k] + 11, MiB - 1)
    out.append(("blocksize_low", b, k))
    b = a.copy(); _put_i32(b, s[k] + 11, (1000 << 20) + 1)
    out.append(("blocksize_high", b, k))
    b = a.copy(); _put_i32(b, s[k] + 7, -5)
    out.append(("negative_payload", b, k))
    b = a.copy(); _put_i32(b, s[k] + 7, (1000 << 20) + 1)
    out.append(("payload_above_max", b, k))
    b = a.copy(); _put_i32(b, s[-1] + 7, len(a) - s[-1])       # last payload runs past the end
    out.append(("payload_past_end", b, len(s) - 1))
    for extra in (1, 7, 14):
        out.append((f"trailing_{extra}", np.concatenate([a, a[:extra]]), len(s)))
    b = a[: s[k] + 9].copy()                                  # truncated inside a header
    out.append(("truncated_header", b, k))
    return out


def test_frames_hostile_cases(jam, arch):
    a, data = arch
    raw_before = [0, 6000, 12000, 18000, 24000, len(data)]
    lib = jam.lib()
    for name, b, k in hostile_cases(a):
        nf, raw, bad = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        rc = lib.jpk_jam_frames(b.ctypes.data, len(b), C.byref(nf), C.byref(raw), C.byref(bad))
        assert rc == -3, name
        assert (nf.value, raw.value, bad.value) == (k, raw_before[k], k), name


def test_frames_every_trailing_length(jam, arch):
    a, _ = arch
    for extra in range(1, 15):
        assert jam.jam_frames(np.concatenate([a, a[:extra]]))[2] == 5, extra
    assert jam.jam_frames(np.concatenate([a, a[:15]]))[2] == 5         # 15 bytes: a whole header, and a bad one (payload past the end)


def test_frames_payload_checks(jam, oracle, arch):
    """beyond the header: the payload's chunk headers (jpk_ans_decoded_size) and its raw size against BlockSize"""
    a, data = arch
    s = _starts(a)
    b = a.copy(); b[s[1] + 15: s[1] + 40] = 0                 # chunk header destroyed
    assert jam.jam_frames(b)[1:] == (6000, 1)
    h, p = _frame(oracle, jam.corpus.make("text", MiB + 100, 73), MiB)   # declares MiB + 100 raw bytes, BlockSize MiB
    assert jam.jam_frames(np.concatenate([a, h, p]))[1:] == (len(data), 5)
    h0 = np.frombuffer(oracle.block_header(0, 0, MiB), dtype=np.uint8)   # empty payload: no BWT trailer
    assert jam.jam_frames(h0) == (0, 0, 0)


def test_archive_entries_need_a_device(jam, arch):
    if jam.lib().jpk_device_count() > 0:
        pytest.skip("a GPU is visible")
    a, data = arch
    lib = jam.lib()
    out = np.zeros(len(a) + 4096, dtype=np.uint8)
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    assert lib.jpk_jam_compress(data.ctypes.data, len(data), MiB, out.ctypes.data, len(out), C.byref(n), 0) == -6
    assert lib.jpk_jam_decompress(a.ctypes.data, len(a), out.ctypes.data, len(out), C.byref(n), C.byref(nf), C.byref(bf)) == -6
    assert lib.jpk_dev_jam_compress(None, None, 0, MiB, None, 0, C.byref(n), 0) == -1
    assert lib.jpk_dev_jam_decompress(None, None, 0, None, 0, C.byref(n), None, None) == -1
    assert lib.jpk_dev_checksums(None, 0, None, None, None) == -1
    with pytest.raises(jam.JampackError) as e:
        jam.jam_compress(data, MiB)
    assert e.value.status == -6
    with pytest.raises(jam.JampackError) as e:
        jam.jam_decompress(a)
    assert e.value.status == -6
