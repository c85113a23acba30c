"""Whole .jam archives in one call (jpk_dev_jam_compress / jpk_dev_jam_decompress and their host forms) and the batched checksum:
the archive must be byte for byte the frames of the per-frame path (jpk_jam_block_write over consecutive slices) and of the oracle,
decode back to its input, honour the capacity contract, and stop at the first bad frame with the frames in front of it verified and in
place.  -m gpu"""
import ctypes as C

import numpy as np
import pytest

from test_jam_archive_host import _archive, hostile_cases

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SENT = 0xA5


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available()
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


def _dev(torch, a, lead=0, extra=0):
    """device copy of a at byte offset `lead` of a buffer with `extra` bytes behind it; returns (buffer, address)"""
    buf = torch.full((lead + len(a) + extra + 1,), SENT, dtype=torch.uint8, device="cuda")
    if len(a):
        buf[lead: lead + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return buf, buf.data_ptr() + lead


def _frame_loop(jam, data, bs):
    parts = [jam.jam_block_write(data[o: o + bs], bs) for o in range(0, len(data), bs)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def test_batched_checksum(gpu):
    torch, jam, ctx = gpu
    lens = list(range(0, 70)) + list(range(4095, 4114)) + list(range(65535, 65554)) + [64 * MiB]
    data = jam.corpus.make("text", sum(lens) + 4 * len(lens), 61)
    buf, base = _dev(torch, data)
    ptrs, pos, segs = [], 0, []
    for i, n in enumerate(lens):
        pos += 1 + i % 3                                  # starts at offsets 1, 2 and 3 from where the last one ended
        ptrs.append(base + pos)
        segs.append(data[pos: pos + n])
        pos += n
    got = ctx.checksums(ptrs, lens)
    assert got == [jam.checksum_host(s) for s in segs]
    assert ctx.checksums(ptrs[-1:], lens[-1:]) == [jam.checksum_host(segs[-1])]   # the batch of one (jpk_dev_checksum's path)


KINDS = ("text", "random", "zero", "silesia")


def _lengths(bs):
    return [0, 1, 119, 120, bs - 1, bs, bs + 1, 3 * bs + 12345]


@pytest.mark.parametrize("bs_mib", [1, 8, 64])
def test_compress_bytes_and_round_trip(gpu, oracle, bs_mib):
    torch, jam, ctx = gpu
    bs = bs_mib * MiB
    for i, n in enumerate(_lengths(bs)):
        kind = KINDS[i % len(KINDS)]
        data = jam.corpus.make(kind, n, 100 + i)
        bound = jam.jam_compress_bound(n, bs)
        d_in_buf, d_in = _dev(torch, data, lead=1)
        out_buf = torch.full((bound + 32,), SENT, dtype=torch.uint8, device="cuda")
        d_out = out_buf.data_ptr() + 3
        m = ctx.jam_compress(d_in, n, bs, d_out, bound)
        got = out_buf.cpu().numpy()
        assert (got[:3] == SENT).all() and (got[3 + m:] == SENT).all(), (kind, n)     # nothing written outside the archive
        arch = got[3: 3 + m].copy()
        assert np.array_equal(arch, _frame_loop(jam, data, bs)), (kind, n)
        # the oracle's frames for the slices it compresses quickly
        if n <= 4 * MiB:
            want = [np.zeros(0, dtype=np.uint8)]
            for o in range(0, n, bs):
                sl = data[o: o + bs]
                if len(sl) < 120:
                    want = None
                    break
                p = oracle.compress_block(sl)
                want += [np.frombuffer(oracle.block_header(oracle.checksum(sl), len(p), bs), dtype=np.uint8), p]
            if want is not None:
                assert np.array_equal(arch, np.concatenate(want)), (kind, n)
        # host form, and back again
        assert np.array_equal(jam.jam_compress(data, bs), arch), (kind, n)
        a_buf, d_a = _dev(torch, arch, lead=5)
        o_buf = torch.full((n + 32,), SENT, dtype=torch.uint8, device="cuda")
        r, nf, bad = ctx.jam_decompress(d_a, m, o_buf.data_ptr() + 1, n)
        assert (r, nf, bad) == (n, (n + bs - 1) // bs, -1), (kind, n)
        back = o_buf.cpu().numpy()
        assert np.array_equal(back[1: 1 + n], data) and back[0] == SENT and (back[1 + n:] == SENT).all(), (kind, n)
        assert np.array_equal(jam.jam_decompress(arch), data), (kind, n)


def test_many_small_frames_one_call(gpu):
    """512 frames of 1 MiB: grouped small blocks, four passes of 128 frames"""
    torch, jam, ctx = gpu
    data = jam.corpus.make("text", 512 * MiB, 62)
    d_buf, d_in = _dev(torch, data)
    bound = jam.jam_compress_bound(len(data), MiB)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    m = ctx.jam_compress(d_in, len(data), MiB, out.data_ptr(), bound)
    arch = out[:m].cpu().numpy()
    assert np.array_equal(arch, _frame_loop(jam, data, MiB))
    assert jam.jam_frames(arch) == (512, len(data), -1)
    back = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    assert ctx.jam_decompress(out.data_ptr(), m, back.data_ptr(), len(data)) == (len(data), 512, -1)
    assert torch.equal(back, d_buf[: len(data)])


def test_concatenated_archives_of_the_frame_path(gpu):
    torch, jam, ctx = gpu
    d1 = jam.corpus.make("text", 3 * MiB + 777, 63)
    d2 = jam.corpus.make("silesia", 9 * MiB + 5, 64)
    arch = np.concatenate([_frame_loop(jam, d1, MiB), _frame_loop(jam, d2, 8 * MiB)])     # archives made one frame at a time
    want = np.concatenate([d1, d2])
    _, d_a = _dev(torch, arch, lead=7)
    out = torch.empty(len(want), dtype=torch.uint8, device="cuda")
    assert ctx.jam_decompress(d_a, len(arch), out.data_ptr(), len(want)) == (len(want), 6, -1)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(jam.jam_decompress(arch), want)


def test_capacity_contract(gpu):
    torch, jam, ctx = gpu
    data = jam.corpus.make("text", 2 * MiB + 999, 65)
    arch = jam.jam_compress(data, MiB)
    _, d_a = _dev(torch, arch)
    assert ctx.jam_decompress(d_a, len(arch), None, 0, check=False) == (len(data), 0, -1, -2)        # the size query
    out = torch.full((len(data) + 16,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_decompress(d_a, len(arch), out.data_ptr(), len(data) - 1, check=False) == (len(data), 0, -1, -2)
    assert (out.cpu().numpy() == SENT).all()                                                        # nothing written
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    host = np.full(len(data), SENT, dtype=np.uint8)
    assert jam.lib().jpk_jam_decompress(arch.ctypes.data, len(arch), host.ctypes.data, len(data) - 1, C.byref(n), C.byref(nf), C.byref(bf)) == -2
    assert n.value == len(data) and (host == SENT).all()
    # compress side: an archive that does not fit
    d_buf, d_in = _dev(torch, data)
    small = torch.empty(len(arch) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(jam.JampackError) as e:
        ctx.jam_compress(d_in, len(data), MiB, small.data_ptr(), len(arch) - 1)
    assert e.value.status == -2


def _starts(a):
    o, s = 0, []
    while o < len(a):
        s.append(o)
        o += 15 + int(np.frombuffer(a[o + 7: o + 11].tobytes(), dtype="<i4")[0])
    return s


@pytest.mark.parametrize("what", ["payload", "crc"])
def test_corrupt_frame_stops_there(gpu, what):
    torch, jam, ctx = gpu
    data = jam.corpus.make("text", 5 * MiB, 66)
    arch = jam.jam_compress(data, MiB)
    s = _starts(arch)
    assert len(s) == 5
    for k in range(5):
        bad = arch.copy()
        if what == "payload":
            end = s[k + 1] if k + 1 < len(s) else len(arch)
            bad[(s[k] + 15 + end) // 2] ^= 0x40
        else:
            bad[s[k] + 3] ^= 1
        _, d_a = _dev(torch, bad, lead=1)
        out = torch.full((len(data),), SENT, dtype=torch.uint8, device="cuda")
        r, nf, bf, rc = ctx.jam_decompress(d_a, len(bad), out.data_ptr(), len(data), check=False)
        assert (rc, bf, nf, r) == (-3, k, k, k * MiB), (what, k)
        assert np.array_equal(out[: r].cpu().numpy(), data[: r]), (what, k)
        # the host form says the same
        host = np.zeros(len(data), dtype=np.uint8)
        n, hf, hb = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        assert jam.lib().jpk_jam_decompress(bad.ctypes.data, len(bad), host.ctypes.data, len(data), C.byref(n), C.byref(hf), C.byref(hb)) == -3
        assert (n.value, hf.value, hb.value) == (k * MiB, k, k) and np.array_equal(host[: n.value], data[: n.value])
        with pytest.raises(jam.JampackError) as e:
            jam.jam_decompress(bad)
        assert e.value.status == -3


@pytest.mark.parametrize("damage", ["crc", "trailing"])
def test_bad_frame_in_the_second_pass(gpu, oracle, damage):
    """130 frames of 1 000 bytes: the host form stages 128 frames, then 2, and numbers the bad frame from the archive's start"""
    torch, jam, ctx = gpu
    data = jam.corpus.make("text", 130 * 1000, 67)
    a = _archive(oracle, data, MiB, 1000)
    s = _starts(a)
    assert len(s) == 130
    if damage == "crc":
        bad, k = a.copy(), 129
        bad[s[k] + 3] ^= 1
    else:
        bad, k = np.concatenate([a, np.full(7, 0x5A, dtype=np.uint8)]), 130
    host = np.zeros(len(data), dtype=np.uint8)
    n, hf, hb = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    assert jam.lib().jpk_jam_decompress(bad.ctypes.data, len(bad), host.ctypes.data, len(data), C.byref(n), C.byref(hf), C.byref(hb)) == -3
    assert (n.value, hf.value, hb.value) == (k * 1000, k, k)
    assert np.array_equal(host[: k * 1000], data[: k * 1000])
    _, d_a = _dev(torch, bad, lead=1)
    out = torch.full((len(data),), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_decompress(d_a, len(bad), out.data_ptr(), len(data), check=False) == (k * 1000, k, k, -3)
    assert np.array_equal(out[: k * 1000].cpu().numpy(), data[: k * 1000])


def test_device_walk_agrees_with_host_walk(gpu, oracle):
    torch, jam, ctx = gpu
    data = jam.corpus.make("text", 4 * 6000 + 2345, 71)
    a = _archive(oracle, data, MiB, 6000)
    for name, b, k in hostile_cases(a):
        hf, hraw, hbad = jam.jam_frames(b)
        assert hbad == k, name
        _, d_b = _dev(torch, b, lead=3)
        out = torch.empty(len(data) + 16, dtype=torch.uint8, device="cuda")
        r, nf, bf, rc = ctx.jam_decompress(d_b, len(b), out.data_ptr(), len(data), check=False)
        assert (rc, bf, nf, r) == (-3, hbad, hf, hraw), name
        assert np.array_equal(out[:r].cpu().numpy(), data[:r]), name


@pytest.mark.slow
def test_archive_above_2_31_bytes(gpu):
    """2.25 GiB of text seeded per 64 MiB block (a repeated buffer would hit the sort's deep-repeat cliff) as 64 MiB frames"""
    torch, jam, ctx = gpu
    bs = 64 * MiB
    nblk = 36
    d_in = torch.empty(nblk * bs, dtype=torch.uint8, device="cuda")
    for b in range(nblk):
        d_in[b * bs: (b + 1) * bs] = torch.from_numpy(jam.corpus.make("text", bs, 1000 + b)).to("cuda")
    n = d_in.numel()
    assert n > (1 << 31)
    bound = jam.jam_compress_bound(n, bs)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    m = ctx.jam_compress(d_in.data_ptr(), n, bs, out.data_ptr(), bound)
    arch = out[:m].cpu().numpy()
    assert jam.jam_frames(arch) == (nblk, n, -1)
    back = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.jam_decompress(out.data_ptr(), m, back.data_ptr(), n) == (n, nblk, -1)
    assert torch.equal(back, d_in)
