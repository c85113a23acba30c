"""The staged reader with the deep expander as its last stage (jam_cli_pass of jam_archive.hip: k_lzd_plan + k_lzd_copy, k_pre_lz77 only
for the frames they leave to it), on frames built by hand around a crafted S1': the header with bit 30 and the crc of the raw bytes in
front of jam.block_compress(S2), S2 being every 64 KiB piece of S1' behind 00 00 (the stored filter form, jam_staged_cases.s2_stored).
BlockSize is 1 MiB.  The streams are lz_deep_cases.generations at the depths of real 8 and 64 MiB streams (9, 15), at the hop cap H and
one beyond it.  -m gpu"""
import struct

import numpy as np
import pytest

import lz_deep_cases as lzd
import lz_expand_cases as lzc
from jam_staged_cases import FBS, MiB, STAGED

pytestmark = pytest.mark.gpu

OK, E_CORRUPT = 0, -3
SENT = 0xA5


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


def _u8(x):
    return np.frombuffer(bytes(x), dtype=np.uint8)


def _frame(jam, s1, raw):
    """the staged frame of the stream s1, whose raw bytes the header's crc covers"""
    s1 = _u8(s1)
    s2 = np.concatenate([np.concatenate([np.zeros(2, dtype=np.uint8), s1[o: o + FBS]]) for o in range(0, len(s1), FBS)])
    payload = jam.block_compress(s2)
    head = struct.pack("<3sIii", b"JAM", jam.checksum_host(raw), len(payload), MiB | STAGED)
    return np.concatenate([_u8(head), payload])


@pytest.fixture(scope="module")
def deep(gpu):
    """depth -> (frame, raw bytes) of the generational stream; H from the library"""
    _, jam, _ = gpu
    hops = jam.lz77_deep_limits()[0]
    out = {}
    for d in (9, 15, hops, hops + 1):
        s1 = lzd.generations(d)
        raw = jam.Lz77().Decompress(s1, MiB)
        assert len(raw) == 4096 * (d + 1) and lzc.shape(s1)[1] == d
        out[d] = (_frame(jam, s1, raw), raw)
    return hops, out


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _launches(ctx):
    return {r["name"]: r["launches"] for r in ctx.profile_table()}


def _decode(gpu, arch, cap, check=True, lead=0):
    """(image of the cap + 64 bytes at d_out, result, launches by kernel) of Context.jam_staged_decompress into a buffer `lead` bytes
    behind a 256-byte-aligned address"""
    torch, jam, ctx = gpu
    buf = torch.full((lead + cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    d_arch = _dev(torch, arch)
    ctx.profile_enable(2)
    res = ctx.jam_staged_decompress(d_arch, len(arch), buf[lead:], cap, check=check)
    table = _launches(ctx)
    ctx.profile_enable(0)
    img = buf.cpu().numpy()
    assert (img[:lead] == SENT).all()
    return img[lead:], res, table


def test_deep_frames_decode_without_the_serial_kernel(gpu, deep):
    """fails on a reader whose last stage is k_pre_lz77"""
    _, jam, ctx = gpu
    hops, frames = deep
    for d in (9, 15, hops):
        f, raw = frames[d]
        img, res, table = _decode(gpu, f, MiB)
        assert res == (len(raw), 1, -1) and np.array_equal(img[: len(raw)], raw) and (img[len(raw):] == SENT).all(), d
        assert table.get("k_lzd_plan") == 1 and table.get("k_lzd_copy") == 1 and "k_pre_lz77" not in table, (d, table)
        assert ctx.lz77_deep_last() == (1, 0), d
    arch = np.concatenate([frames[d][0] for d in (9, 15, hops)])
    raw = np.concatenate([frames[d][1] for d in (9, 15, hops)])
    img, res, table = _decode(gpu, arch, 3 * MiB)
    assert res == (len(raw), 3, -1) and np.array_equal(img[: len(raw)], raw)
    assert table.get("k_lzd_plan") == 1 and table.get("k_lzd_copy") == 1 and "k_pre_lz77" not in table, table
    assert np.array_equal(jam.jam_staged_decompress(arch), raw)         # the host form runs the same pass


def test_a_frame_one_hop_too_deep_takes_the_serial_kernel(gpu, deep):
    _, _, ctx = gpu
    hops, frames = deep
    f, raw = frames[hops + 1]
    img, res, table = _decode(gpu, f, MiB)
    assert res == (len(raw), 1, -1) and np.array_equal(img[: len(raw)], raw) and (img[len(raw):] == SENT).all()
    assert table.get("k_lzd_plan") == 1 and table.get("k_lzd_copy") == 1 and table.get("k_pre_lz77") == 1, table
    assert ctx.lz77_deep_last() == (0, 1)


@pytest.fixture(scope="module")
def mixed(gpu, deep):
    """deep frame | plain frame | frame at depth H + 1 | frame with an offset beyond the output in its stream; the raw bytes of the first three"""
    _, jam, _ = gpu
    hops, frames = deep
    plain = jam.corpus.make("text", 300_001, 5)
    bad = lzc.corrupt_cases()[1]
    assert bad[0] == "offset beyond the output, late"
    parts = [frames[hops][1], plain, frames[hops + 1][1]]
    arch = np.concatenate([frames[hops][0], jam.jam_block_write(plain, MiB), frames[hops + 1][0], _frame(jam, bad[1], _u8(b"no such bytes"))])
    return arch, np.concatenate(parts), parts


def test_mixed_archive_stops_at_the_bad_stream_with_the_rest_in_place(gpu, mixed):
    _, jam, ctx = gpu
    arch, raw, parts = mixed
    bound = MiB + len(parts[1]) + 2 * MiB
    assert jam.jam_staged_frames(arch) == (4, bound, -1)
    img, res, table = _decode(gpu, arch, bound, check=False)
    assert res == (len(raw), 3, 3, E_CORRUPT), res
    assert np.array_equal(img[: len(raw)], raw)
    assert table.get("k_lzd_plan") == 1 and table.get("k_lzd_copy") == 1 and table.get("k_pre_lz77") == 1, table
    assert ctx.lz77_deep_last() == (1, 2)


def test_index_read_and_salvage_of_the_mixed_archive(gpu, mixed):
    torch, jam, ctx = gpu
    arch, raw, parts = mixed
    d_arch = _dev(torch, arch)
    ix = ctx.jam_staged_index(d_arch, len(arch), verify=True)
    assert (ix.frames, ix.bad_frame, ix.raw_len) == (3, 3, len(raw))
    assert [ix.frame(k)[1] for k in range(3)] == [len(p) for p in parts] and [ix.frame_kind(k) for k in range(3)] == [2, 0, 2]
    # a range inside the deep frame, one across the plain frame into the frame that takes the serial kernel
    # and one that holds the deep frame whole: its last stage writes straight into the caller's buffer
    ranges = [(4096 * 20 + 5, 9000), (len(parts[0]) - 77, 77 + len(parts[1]) + 5000), (0, len(parts[0]) + 10)]
    outs = [torch.full((n + 64,), SENT, dtype=torch.uint8, device="cuda") for _, n in ranges]
    ctx.profile_enable(2)
    first = torch.full((ranges[0][1],), SENT, dtype=torch.uint8, device="cuda")
    st, bad = ctx.jam_read(ix, d_arch, len(arch), ranges[:1], [first])
    table = _launches(ctx)
    ctx.profile_enable(0)
    assert st == [OK] and bad == -1 and table.get("k_lzd_copy") == 1 and "k_pre_lz77" not in table, table
    assert np.array_equal(first.cpu().numpy(), raw[ranges[0][0]: ranges[0][0] + ranges[0][1]])
    st, bad = ctx.jam_read(ix, d_arch, len(arch), ranges, [o[1:] for o in outs])       # odd destinations
    assert st == [OK] * 3 and bad == -1
    for (o, n), d in zip(ranges, outs):
        got = d.cpu().numpy()
        assert got[0] == SENT and np.array_equal(got[1: 1 + n], raw[o: o + n]) and (got[1 + n:] == SENT).all(), (o, n)
    ix.close()
    rx = ctx.jam_recover_index(d_arch, len(arch), kind=jam.JAM_INDEX_STAGED, verify=True)
    assert rx.frames == 3 and rx.raw_len == len(raw) and len(rx.gaps) == 1
    d_out = torch.full((len(raw) + 64,), SENT, dtype=torch.uint8, device="cuda")
    n, st = ctx.jam_salvage(rx, d_arch, len(arch), d_out, len(raw))
    got = d_out.cpu().numpy()
    assert n == len(raw) and st == [OK] * 3 and np.array_equal(got[: len(raw)], raw) and (got[len(raw):] == SENT).all()
    rx.close()


def test_decode_into_an_odd_address(gpu, deep, mixed):
    hops, frames = deep
    f, raw = frames[15]
    for lead in (1, 7):
        img, res, table = _decode(gpu, f, len(raw), lead=lead)
        assert res == (len(raw), 1, -1) and np.array_equal(img[: len(raw)], raw) and (img[len(raw):] == SENT).all(), lead
        assert "k_pre_lz77" not in table, table
    arch, raw, parts = mixed
    img, res, _ = _decode(gpu, arch, MiB + len(parts[1]) + 2 * MiB, check=False, lead=3)
    assert res == (len(raw), 3, 3, E_CORRUPT) and np.array_equal(img[: len(raw)], raw)
