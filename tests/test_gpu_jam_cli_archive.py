"""Whole archives of the stock CLI in one batched call (jpk_dev_jam_cli_decompress / jpk_jam_cli_decompress): every frame through the
batched entropy decode + inverse BWT and the four pre-stage decoders on the device, against the frame-by-frame path
(jam_cli_block_read, pre-stages on the host).  Archives are built by concatenating the golden frames.  -m gpu"""
import json
import os

import numpy as np
import pytest

from golden_util import GOLD

pytestmark = pytest.mark.gpu

MiB = 1 << 20
OK, E_CAPACITY, E_CORRUPT = 0, -2, -3
SENT, GUARD = 0xA5, 4096


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "golden_cli.npz")), json.load(open(os.path.join(GOLD, "golden_cli_manifest.json")))


@pytest.fixture(scope="module")
def arch40(gpu, golden):
    """the eight golden frames five times over in shuffled order: (archive, frame starts, per-frame raw bytes from jam_cli_block_read)"""
    _, jam, _ = gpu
    z, man = golden
    back = {c["name"]: jam.jam_cli_block_read(z[c["name"]], c["block_size"])[0] for c in man["frames"]}
    order = np.random.default_rng(97).permutation([c["name"] for c in man["frames"]] * 5)
    assert len(order) == 40
    starts = np.cumsum([0] + [len(z[n]) for n in order]).tolist()
    return np.concatenate([z[n] for n in order]), starts, [back[n] for n in order]


def _dev(gpu, a, cap):
    """the device form with the archive in HBM and `cap` bytes of output in front of a guard -> (bytes, frames, bad, status, out_len, guard ok)"""
    torch, _, ctx = gpu
    d_in = torch.from_numpy(np.ascontiguousarray(a)).to("cuda") if len(a) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_out = torch.full((cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    n, nf, bf, rc = ctx.jam_cli_decompress(d_in, len(a), d_out, cap, check=False)
    img = d_out.cpu().numpy()
    return img[: n if rc in (OK, E_CORRUPT) else 0], nf, bf, rc, n, bool((img[cap:] == SENT).all())


def _both(gpu, a, cap):
    _, jam, _ = gpu
    yield "device", _dev(gpu, a, cap)[:4]
    yield "host", jam.jam_cli_decompress_all(a, check=False)


def test_golden_two_block_stream(gpu, golden):
    _, jam, _ = gpu
    z, man = golden
    a = z[man["stream"]["name"]]
    exp = jam.jam_cli_decompress(a)
    assert jam.jam_cli_frames(a) == (2, 2 * MiB, -1)
    for form, (got, nf, bf, rc) in _both(gpu, a, 2 * MiB):
        assert (rc, nf, bf) == (OK, 2, -1), form
        assert np.array_equal(got, exp), form
    assert np.array_equal(jam.jam_cli_decompress_all(a), exp)


def test_archive_of_40_frames(gpu, arch40):
    _, jam, _ = gpu
    a, _, frames = arch40
    exp = np.concatenate(frames)
    assert jam.jam_cli_frames(a) == (40, 40 << 20, -1)
    for form, (got, nf, bf, rc) in _both(gpu, a, 40 << 20):
        assert (rc, nf, bf) == (OK, 40, -1), form
        assert np.array_equal(got, exp), form


@pytest.mark.parametrize("damage", ["payload", "crc", "truncated"])
def test_damaged_archive_stops_at_the_bad_frame(gpu, arch40, damage):
    a, starts, frames = arch40
    b = a.copy()
    if damage == "payload":
        b[(starts[7] + 15 + starts[8]) // 2] ^= 0x04
        k = 7
    elif damage == "crc":
        b[starts[7] + 4] ^= 0x10
        k = 7
    else:
        b = b[: len(b) - 3]
        k = 39
    exp = np.concatenate(frames[:k])
    for form, (got, nf, bf, rc) in _both(gpu, b, 40 << 20):
        assert (rc, nf, bf) == (E_CORRUPT, k, k), (form, damage)
        assert np.array_equal(got, exp), (form, damage)


def test_capacity_exact_and_one_byte_short(gpu, arch40):
    _, jam, _ = gpu
    a, _, frames = arch40
    exp = np.concatenate(frames)
    got, nf, bf, rc, n, guard = _dev(gpu, a, len(exp))
    assert (rc, nf, bf, n) == (OK, 40, -1, len(exp)) and guard
    assert np.array_equal(got, exp)
    _, nf, bf, rc, n, guard = _dev(gpu, a, len(exp) - 1)
    assert (rc, n) == (E_CAPACITY, 40 << 20), (rc, n)
    assert guard, "bytes behind out_cap were written"
    # the host form: the same answers
    import ctypes as C
    out = np.full(len(exp) + GUARD, SENT, dtype=np.uint8)
    m, f, bad = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
    rc = jam.lib().jpk_jam_cli_decompress(a.ctypes.data, len(a), out.ctypes.data, len(exp), C.byref(m), C.byref(f), C.byref(bad))
    assert (rc, m.value, f.value, bad.value) == (OK, len(exp), 40, -1)
    assert np.array_equal(out[: len(exp)], exp) and (out[len(exp):] == SENT).all()
    out[:] = SENT
    rc = jam.lib().jpk_jam_cli_decompress(a.ctypes.data, len(a), out.ctypes.data, len(exp) - 1, C.byref(m), C.byref(f), C.byref(bad))
    assert (rc, m.value) == (E_CAPACITY, 40 << 20)
    assert (out[len(exp) - 1:] == SENT).all()


@pytest.fixture(scope="module")
def arch130(gpu):
    """130 one-frame archives of 1 000 bytes each, BlockSize 1 MiB, back to back: (archive, frame starts, input)"""
    _, jam, _ = gpu
    data = jam.corpus.make("text", 130 * 1000, 99)
    parts = [jam.jam_cli_block_write(data[o: o + 1000], MiB) for o in range(0, len(data), 1000)]
    return np.concatenate(parts), np.cumsum([0] + [len(p) for p in parts]).tolist(), data


def _host(jam, a, cap):
    """jpk_jam_cli_decompress with `cap` bytes of output -> (output buffer, out_len, frames, bad, status)"""
    import ctypes as C
    out = np.full(max(cap, 1), SENT, dtype=np.uint8)
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
    rc = jam.lib().jpk_jam_cli_decompress(a.ctypes.data, len(a), out.ctypes.data, cap, C.byref(n), C.byref(nf), C.byref(bf))
    return out, n.value, nf.value, bf.value, rc


@pytest.mark.parametrize("damage", ["crc", "trailing", "capacity"])
def test_second_pass_of_130_frames(gpu, arch130, damage):
    """the host form stages 128 frames, then 2: a bad frame there is numbered from the archive's start, and a pass that does not fit
    reports the frame it starts at"""
    _, jam, _ = gpu
    a, starts, data = arch130
    assert jam.jam_cli_frames(a) == (130, 130 * MiB, -1)
    if damage == "capacity":
        _, n, nf, bf, rc = _host(jam, a, len(data) - 1)
        assert (rc, n, nf) == (E_CAPACITY, 130 * MiB, 128)
        return
    if damage == "crc":
        b, k = a.copy(), 129
        b[starts[k] + 3] ^= 1
    else:
        b, k = np.concatenate([a, np.full(7, 0x5A, dtype=np.uint8)]), 130
    out, n, nf, bf, rc = _host(jam, b, len(data))
    assert (rc, n, nf, bf) == (E_CORRUPT, k * 1000, k, k)
    assert np.array_equal(out[: n], data[: n])
    got, nf, bf, rc, n, guard = _dev(gpu, b, len(data))
    assert (rc, n, nf, bf) == (E_CORRUPT, k * 1000, k, k) and guard
    assert np.array_equal(got, data[: n])


def test_empty_archive(gpu):
    _, jam, _ = gpu
    e = np.zeros(0, dtype=np.uint8)
    assert jam.jam_cli_frames(e) == (0, 0, -1)
    for form, (got, nf, bf, rc) in _both(gpu, e, 16):
        assert (rc, nf, bf, len(got)) == (OK, 0, -1, 0), form


def test_live_reference_archive(gpu, ref):
    """four frames of 1 MiB of text as the stock CLI writes them (match finder 0, filters 1: its defaults)"""
    _, jam, _ = gpu
    t = jam.corpus.make("text", 4 * MiB, 98)
    a = np.concatenate([ref.jam_comp_block(t[i * MiB: (i + 1) * MiB], MiB, 0, 1) for i in range(4)])
    assert jam.jam_cli_frames(a) == (4, 4 * MiB, -1)
    for form, (got, nf, bf, rc) in _both(gpu, a, 4 * MiB):
        assert (rc, nf, bf) == (OK, 4, -1), form
        assert np.array_equal(got, t), form
