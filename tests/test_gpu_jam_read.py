"""Range reads of a .jam archive (jpk_jam_index, jpk_dev_jam_read / jpk_jam_read): every range must equal the slice of the input
whatever its edges, order and destination alignment, nothing outside the ranges may be written, a frame is decoded in place when a
range holds it whole, and damage in a frame fails only the ranges that touch it.  -m gpu"""
import numpy as np
import pytest

from test_jam_archive_host import _frame, _starts

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SENT = 0xA5
SIZES = [1, 119, 120, 121, 4096, 65535, 65536, 65537, 1, 300000, 16, 15]
CORRUPT = -3


@pytest.fixture(scope="module")
def gpu():
    import torch
    import jampack_amd as jam
    assert torch.cuda.is_available()
    ctx = jam.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, jam, ctx
    ctx.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@pytest.fixture(scope="module")
def arch(gpu):
    """one frame per entry of SIZES (BlockSize 1 MiB): (archive, input, frame boundaries in raw coordinates, device copy, its index)"""
    torch, jam, ctx = gpu
    data = jam.corpus.make("text", sum(SIZES), 91)
    bounds = [0] + [int(x) for x in np.cumsum(SIZES)]
    a = np.concatenate([jam.jam_block_write(data[bounds[k]: bounds[k + 1]], MiB) for k in range(len(SIZES))])
    d_a = _dev(torch, a)
    ix = ctx.jam_index(d_a, len(a))
    assert (ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame) == (len(SIZES), len(data), len(a), -1)
    return a, data, bounds, d_a, ix


def edge_ranges(bounds):
    raw = bounds[-1]
    out = []
    for b in bounds:
        for off in sorted({min(max(b + d, 0), raw) for d in (-17, -16, -1, 0, 1)}):
            for ln in sorted({min(x, raw - off) for x in (0, 1, 15, 16, 17, 31, 33, 4097, 65536, raw - off)}):
                out.append((off, ln))
    return out


def read(torch, ctx, ix, d_a, alen, ranges, check=True):
    """the ranges into ONE sentinel-filled buffer, range i at byte offset i % 17 from a 16-byte-aligned address, gaps between them;
    returns (status, bad frame, the whole buffer, where every range starts in it)"""
    at, pos = [], 0
    for i, (_, ln) in enumerate(ranges):
        pos = (pos + 15) // 16 * 16 + i % 17
        at.append(pos)
        pos += ln + 1 + i % 5
    buf = torch.full((pos + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    st, bad = ctx.jam_read(ix, d_a, alen, ranges, [buf.data_ptr() + p for p in at], check=check)
    return st, bad, buf.cpu().numpy(), at


def image(data, ranges, at, size, skip=()):
    want = np.full(size, SENT, dtype=np.uint8)
    for i, ((off, ln), p) in enumerate(zip(ranges, at)):
        if i not in skip:
            want[p: p + ln] = data[off: off + ln]
    return want


def exact(torch, ctx, ix, d_a, alen, ranges, data):
    """every range equals the slice of the input, every other byte still holds the sentinel"""
    st, bad, got, at = read(torch, ctx, ix, d_a, alen, ranges)
    assert st == [0] * len(ranges) and bad == -1
    want = image(data, ranges, at, len(got))
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        r = max(k for k, p in enumerate(at) if p <= i) if at[0] <= i else -1
        raise AssertionError(f"byte {i} of the buffer differs (range {r}: {ranges[r]} at {at[r]})")


CALL = 256


def test_edges(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, d_a, ix = arch
    rs = edge_ranges(bounds)
    assert len(rs) > 2 * CALL
    for o in range(0, len(rs), CALL):
        exact(torch, ctx, ix, d_a, len(a), rs[o: o + CALL], data)


def test_order_and_sharing(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, d_a, ix = arch
    rs = edge_ranges(bounds) * 2                            # one call of ~1 000 ranges: a large piece table
    assert 2 * CALL < len(rs) <= 4096
    rng = np.random.default_rng(5)
    rs = [rs[i] for i in rng.permutation(len(rs))]
    exact(torch, ctx, ix, d_a, len(a), rs, data)
    lo, hi = bounds[9], bounds[10]                          # 64 ranges inside the 300 000-byte frame
    inside = []
    for _ in range(64):
        off = int(rng.integers(lo, hi))
        inside.append((off, int(rng.integers(0, min(hi - off, 5000) + 1))))
    exact(torch, ctx, ix, d_a, len(a), inside, data)


def _full_range_is_decompress(torch, ctx, a, data):
    d_a = _dev(torch, a)
    ix = ctx.jam_index(d_a, len(a))
    n = len(data)
    assert ix.raw_len == n
    ref = torch.full((n + 16,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_decompress(d_a, len(a), ref.data_ptr(), n)[0] == n
    for lead in (0, 3):
        out = torch.full((n + 16,), SENT, dtype=torch.uint8, device="cuda")
        st, bad = ctx.jam_read(ix, d_a, len(a), [(0, n)], [out.data_ptr() + lead])
        assert (st, bad) == ([0], -1)
        assert torch.equal(out[lead: lead + n], ref[:n]) and bool((out[:lead] == SENT).all()) and bool((out[lead + n:] == SENT).all())
    assert np.array_equal(ref[:n].cpu().numpy(), data)
    ix.close()


def test_full_range(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, d_a, ix = arch
    _full_range_is_decompress(torch, ctx, a, data)


def test_full_range_large_frames(gpu):
    """two 5 MiB frames and a 1-byte frame: few large blocks, the per-block inverse BWTs"""
    torch, jam, ctx = gpu
    data = jam.corpus.make("text", 10 * MiB + 1, 92)
    a = jam.jam_compress(data, 5 * MiB)
    assert jam.jam_frames(a) == (3, len(data), -1)
    _full_range_is_decompress(torch, ctx, a, data)


def test_more_than_one_pass(gpu, oracle):
    """300 frames: three passes of at most 128 touched frames"""
    torch, jam, ctx = gpu
    sizes = [200 + (k * 37) % 61 for k in range(300)]
    data = jam.corpus.make("text", sum(sizes), 93)
    bounds = [0] + [int(x) for x in np.cumsum(sizes)]
    parts = []
    for k in range(300):
        parts += list(_frame(oracle, data[bounds[k]: bounds[k + 1]], MiB))
    a = np.concatenate(parts)
    d_a = _dev(torch, a)
    ix = ctx.jam_index(d_a, len(a))
    assert (ix.frames, ix.raw_len) == (300, len(data))
    exact(torch, ctx, ix, d_a, len(a), [(0, len(data))], data)
    exact(torch, ctx, ix, d_a, len(a), [(bounds[k], sizes[k]) for k in range(300)], data)
    exact(torch, ctx, ix, d_a, len(a), [(bounds[k] + 1, sizes[k]) for k in range(299)], data)   # every range in two frames, none in place


def _damage(a, frame, what):
    s = _starts(a) + [len(a)]
    b = a.copy()
    if what == "payload":
        b[(s[frame] + 15 + s[frame + 1]) // 2] ^= 0x40
    else:
        b[s[frame] + 3] ^= 1
    return b


def _touches(r, bounds, f):
    return r[1] > 0 and r[0] < bounds[f + 1] and r[0] + r[1] > bounds[f]


def _check_damaged(torch, ctx, a, data, bounds, ranges, damaged):
    d_a = _dev(torch, a)
    ix = ctx.jam_index(d_a, len(a))
    assert (ix.frames, ix.bad_frame) == (len(SIZES), -1)     # the walk does not decode: the damage shows only in a read
    st, bad, got, at = read(torch, ctx, ix, d_a, len(a), ranges, check=False)
    hit = [[f for f in damaged if _touches(r, bounds, f)] for r in ranges]
    assert st == [CORRUPT if h else 0 for h in hit]
    lowest = min((h[0] for h in hit if h), default=-1)
    assert bad == lowest
    failed = {i for i, h in enumerate(hit) if h}
    want = image(data, ranges, at, len(got), skip=failed)
    keep = np.ones(len(got), dtype=bool)                    # the buffer of a failed range is unspecified, everything else is not
    for i in failed:
        keep[at[i]: at[i] + ranges[i][1]] = False
    assert np.array_equal(got[keep], want[keep])
    if failed:                                              # check=True raises the first failing range's status
        import jampack_amd as jam
        outs = [torch.empty(max(r[1], 1), dtype=torch.uint8, device="cuda") for r in ranges]
        with pytest.raises(jam.JampackError) as e:
            ctx.jam_read(ix, d_a, len(a), ranges, outs)
        assert e.value.status == CORRUPT
    ix.close()
    return bad


def _damage_ranges(bounds):
    raw = bounds[-1]
    rs = [(0, bounds[5]), (bounds[5] - 1, 1), (bounds[5] - 1, 2), (bounds[5], 1), (bounds[6] - 1, 1), (bounds[6], 1), (bounds[6] - 1, 2),
          (bounds[4], bounds[7] - bounds[4]), (bounds[6], raw - bounds[6]), (0, raw), (bounds[5] + 100, 0), (bounds[9] + 5, 100),
          (bounds[10], 16), (bounds[8], bounds[10] - bounds[8]), (bounds[2], 300)]
    return rs


@pytest.mark.parametrize("what", ["payload", "crc"])
def test_damage_away_from_the_range(gpu, arch, what):
    torch, jam, ctx = gpu
    a, data, bounds, _, _ = arch
    rs = _damage_ranges(bounds)
    assert _check_damaged(torch, ctx, _damage(a, 5, what), data, bounds, rs, [5]) == 5
    clean = [r for r in rs if not _touches(r, bounds, 5)]
    assert len(clean) >= 6
    assert _check_damaged(torch, ctx, _damage(a, 5, what), data, bounds, clean, [5]) == -1


def test_two_damaged_frames(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, _, _ = arch
    b = _damage(_damage(a, 5, "payload"), 9, "crc")
    rs = _damage_ranges(bounds)
    assert _check_damaged(torch, ctx, b, data, bounds, rs, [5, 9]) == 5
    only9 = [r for r in rs if not _touches(r, bounds, 5)]
    assert any(_touches(r, bounds, 9) for r in only9)
    assert _check_damaged(torch, ctx, b, data, bounds, only9, [5, 9]) == 9


def test_damaged_tail(gpu, arch):
    """7 stray bytes behind the archive: jam_decompress reports a corrupt archive, the index covers all frames and reads work"""
    torch, jam, ctx = gpu
    a, data, bounds, _, _ = arch
    b = np.concatenate([a, a[:7]])
    d_b = _dev(torch, b)
    ix = ctx.jam_index(d_b, len(b))
    assert (ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame) == (len(SIZES), len(data), len(b), len(SIZES))
    exact(torch, ctx, ix, d_b, len(b), edge_ranges(bounds)[:CALL], data)
    exact(torch, ctx, ix, d_b, len(b), [(0, len(data))], data)
    hx = jam.jam_index(b)
    assert (hx.frames, hx.bad_frame) == (len(SIZES), len(SIZES))
    assert np.array_equal(jam.jam_read(b, [(bounds[11], 15)], index=hx)[0], data[bounds[11]:])


def test_host_form(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, d_a, ix = arch
    rs = edge_ranges(bounds)[:CALL]
    hx = jam.jam_index(a)
    for k in range(len(SIZES)):
        assert hx.frame(k) == ix.frame(k)                   # the two walks agree
    got = jam.jam_read(a, rs, index=hx)
    assert len(got) == len(rs)
    for (off, ln), g in zip(rs, got):
        assert np.array_equal(g, data[off: off + ln]), (off, ln)
    few = [(bounds[9] + 7, 1000), (3, 0), (0, len(data))]     # few ranges: copied back one by one; the index built by the call
    for (off, ln), g in zip(few, jam.jam_read(a, few)):
        assert np.array_equal(g, data[off: off + ln]), (off, ln)
    with pytest.raises(jam.JampackError) as e:
        jam.jam_read(_damage(a, 5, "crc"), [(bounds[9], 10), (bounds[5], 1)])
    assert e.value.status == CORRUPT
    assert np.array_equal(jam.jam_read(_damage(a, 5, "crc"), [(bounds[9], 10)])[0], data[bounds[9]: bounds[9] + 10])
