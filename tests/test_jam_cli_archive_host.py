"""Archives of the stock CLI, host side (no GPU): the new entries are exported, declared and bound, the frame walk of jpk_jam_cli_frames on
archives built from the golden frames, and the argument checks of jpk_jam_cli_decompress, which come before it looks for a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from golden_util import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
NEW = ("jpk_dev_blocks_lz77_decompress", "jpk_dev_blocks_lpx_decode", "jpk_dev_blocks_filters_decode", "jpk_dev_jam_cli_decompress",
       "jpk_jam_cli_decompress", "jpk_jam_cli_frames")


@pytest.fixture(scope="module")
def jam():
    import jampack_amd
    return jampack_amd


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "golden_cli.npz")), json.load(open(os.path.join(GOLD, "golden_cli_manifest.json")))


@pytest.fixture(scope="module")
def arch40(golden):
    z, man = golden
    order = np.random.default_rng(97).permutation([c["name"] for c in man["frames"]] * 5)
    starts = np.cumsum([0] + [len(z[n]) for n in order]).tolist()
    return np.concatenate([z[n] for n in order]), starts


def test_new_entries_are_exported_declared_and_bound(jam):
    from jampack_amd._lib import _SIGS
    header = open(os.path.join(ROOT, "include", "jampack_abi.h")).read()
    lib = C.CDLL(jam.LIB_PATH)
    for name in NEW:
        assert re.search(r"JPK_API\s+[\w\s\*]+\b" + name + r"\(", header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _SIGS, f"{name} has no ctypes signature"
    for name in ("blocks_lz77_decompress", "blocks_lpx_decode", "blocks_filters_decode", "jam_cli_decompress"):
        assert hasattr(jam.Context, name), name
    names = [jam.lib().jpk_ctx_profile_name(i).decode() for i in range(jam.lib().jpk_ctx_profile_count())]
    assert names[-3:] == ["k_pre_lz77", "k_pre_lpx", "k_pre_filters"]        # appended behind the existing classes


def test_frames_of_the_golden_stream_and_the_40_frame_archive(jam, golden, arch40):
    z, man = golden
    assert jam.jam_cli_frames(z[man["stream"]["name"]]) == (2, 2 * MiB, -1)
    a, _ = arch40
    assert jam.jam_cli_frames(a) == (40, 40 << 20, -1)
    assert jam.jam_cli_frames(np.zeros(0, dtype=np.uint8)) == (0, 0, -1)


def test_a_stock_frame_may_decode_to_more_than_its_block_size_before_the_pre_stages(jam, golden):
    """jpk_jam_frames bounds the entropy-decoded size by BlockSize, the stock walk by 1.05 x BlockSize + 4096: a frame of the golden
    two-block stream (a full 1 MiB block of text, which the stock settings do not shrink in front of the BWT) tells them apart when it does"""
    z, man = golden
    a = z[man["stream"]["name"]]
    dec, _ = jam.ans_decoded_size(a[15: 15 + int(np.frombuffer(a[7:11].tobytes(), dtype="<i4")[0])])
    assert 0 <= dec - 480 <= int(MiB * 1.05) + 4096
    assert jam.jam_cli_frames(a)[2] == -1
    assert jam.jam_frames(a)[2] == (-1 if dec - 480 <= MiB else 0)


def _put_i32(a, at, v):
    a[at: at + 4] = np.frombuffer(np.int32(v).tobytes(), dtype=np.uint8)


def test_bad_frames(jam, arch40):
    a, s = arch40
    k = 7
    cases = []
    b = a.copy(); b[s[k] + 1] ^= 1
    cases.append(("magic", b, k))
    b = a.copy(); _put_i32(b, s[k] + 11, MiB - 1)
    cases.append(("blocksize_low", b, k))
    b = a.copy(); _put_i32(b, s[k] + 11, (1000 << 20) + 1)
    cases.append(("blocksize_high", b, k))
    b = a.copy(); _put_i32(b, s[-2] + 7, len(a))                 # the last payload runs past the end
    cases.append(("payload_past_end", b, 39))
    for extra in (1, 14):
        cases.append((f"trailing_{extra}", np.concatenate([a, a[:extra]]), 40))
    cases.append(("truncated", a[: len(a) - 3], 39))
    for name, b, bad in cases:
        b = np.ascontiguousarray(b)
        nf, bound, bf = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        rc = jam.lib().jpk_jam_cli_frames(b.ctypes.data, len(b), C.byref(nf), C.byref(bound), C.byref(bf))
        assert rc == -3, name
        assert (nf.value, bound.value, bf.value) == (bad, bad << 20, bad), name
        assert jam.jam_cli_frames(b) == (bad, bad << 20, bad), name


def test_argument_checks_come_before_the_device(jam, arch40):
    a, _ = arch40
    lib = jam.lib()
    out = np.zeros(64, dtype=np.uint8)
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    ap, op = a.ctypes.data, out.ctypes.data
    assert lib.jpk_jam_cli_decompress(ap, len(a), op, len(out), None, C.byref(nf), C.byref(bf)) == -1          # no out_len
    assert lib.jpk_jam_cli_decompress(None, len(a), op, len(out), C.byref(n), None, None) == -1               # null input
    assert lib.jpk_jam_cli_decompress(ap, -1, op, len(out), C.byref(n), None, None) == -1                     # negative sizes
    assert lib.jpk_jam_cli_decompress(ap, len(a), op, -1, C.byref(n), None, None) == -1
    assert lib.jpk_jam_cli_decompress(ap, len(a), None, 64, C.byref(n), None, None) == -1                     # null output
    assert lib.jpk_jam_cli_frames(None, 5, None, None, None) == -1
    assert lib.jpk_jam_cli_frames(ap, -1, None, None, None) == -1
    assert lib.jpk_jam_cli_frames(ap, len(a), None, None, None) == 0                                          # every result pointer may be NULL
    assert lib.jpk_dev_jam_cli_decompress(None, None, 0, None, 0, C.byref(n), None, None) == -1               # no context
    for fn in (lib.jpk_dev_blocks_lz77_decompress, lib.jpk_dev_blocks_filters_decode):
        assert fn(None, 0, None, None, None, None, None, None) == -1
    assert lib.jpk_dev_blocks_lpx_decode(None, 0, None, None, None, None) == -1
    if lib.jpk_device_count() == 0:
        assert lib.jpk_jam_cli_decompress(ap, len(a), op, len(out), C.byref(n), C.byref(nf), C.byref(bf)) == -6
        with pytest.raises(jam.JampackError) as e:
            jam.jam_cli_decompress_all(a)
        assert e.value.status == -6
