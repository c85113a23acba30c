"""Range reads of stock-CLI .jam archives (jpk_dev_jam_cli_index_create, jpk_dev_jam_cli_decompress_ix, jpk_dev_jam_read / jpk_jam_read
on an index of kind 1): the index holds the raw sizes a decode finds, every range equals the slice of the decoded archive whatever its
edges, order and destination alignment, nothing outside the ranges is written, a frame a range holds whole has its last stage write in
place, damage fails only the ranges that touch the damaged frame -- also those in front of good later frames --, and a frame that
decodes to another size than the indexed one is corrupt.  Archives are built from the golden frames.  -m gpu"""
import numpy as np
import pytest

from test_gpu_jam_cli_archive import golden, gpu  # noqa: F401  (fixtures)
from test_gpu_jam_read import CALL, SENT, edge_ranges, exact, image, read
from test_jam_archive_host import _starts

pytestmark = pytest.mark.gpu

MiB = 1 << 20
OK, E_CAPACITY, E_CORRUPT = 0, -2, -3
PLAIN, CLI = 0, 1
SMALL = "frame_repeat4k_200000_74"


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _table(ix):
    return [ix.frame(k) for k in range(ix.frames)]


@pytest.fixture(scope="module")
def arch(gpu, golden):
    """archive A: the eight golden frames in a shuffled order, then the two frames of the golden stream ->
    (archive, decoded bytes, frame boundaries in raw coordinates, frame starts in the archive, device copy, its index)"""
    torch, jam, ctx = gpu
    z, man = golden
    names = [c["name"] for c in man["frames"]]
    order = [names[i] for i in np.random.default_rng(11).permutation(len(names))]
    stream = z[man["stream"]["name"]]
    s = _starts(stream) + [len(stream)]
    assert len(s) == 3
    frames = [z[n] for n in order] + [stream[s[0]: s[1]], stream[s[1]: s[2]]]
    sizes = [next(c["n"] for c in man["frames"] if c["name"] == n) for n in order] + [MiB, man["stream"]["n"] - MiB]
    raw = [jam.jam_cli_block_read(f, MiB)[0] for f in frames]
    assert [len(r) for r in raw] == sizes
    a = np.concatenate(frames)
    bounds = [0] + [int(x) for x in np.cumsum(sizes)]
    d_a = _dev(torch, a)
    ix = ctx.jam_cli_index(d_a, len(a))
    return a, np.concatenate(raw), bounds, _starts(a) + [len(a)], d_a, ix


def test_index(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, starts, d_a, ix = arch
    assert (ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame, ix.kind) == (10, len(data), len(a), -1, CLI)
    want = []
    for k in range(10):
        psize = int(np.frombuffer(a[starts[k] + 7: starts[k] + 11].tobytes(), dtype="<i4")[0])
        assert starts[k] + 15 + psize == starts[k + 1]
        want.append((bounds[k], bounds[k + 1] - bounds[k], starts[k] + 15, psize))
    assert _table(ix) == want
    hx = jam.jam_cli_index(a)                               # the host form: staged, the same table
    assert (hx.frames, hx.raw_len, hx.archive_len, hx.bad_frame, hx.kind) == (10, len(data), len(a), -1, CLI)
    assert _table(hx) == want
    # the whole-archive call hands the same table back, and its bytes are those of the call without an index
    cap = 10 * MiB
    ref = torch.full((cap,), SENT, dtype=torch.uint8, device="cuda")
    out = torch.full((cap,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_cli_decompress(d_a, len(a), ref, cap) == (len(data), 10, -1)
    n, nf, bf, dx = ctx.jam_cli_decompress_ix(d_a, len(a), out, cap)
    assert (n, nf, bf) == (len(data), 10, -1)
    assert torch.equal(out, ref) and np.array_equal(ref[:n].cpu().numpy(), data)
    assert (dx.frames, dx.raw_len, dx.archive_len, dx.bad_frame, dx.kind) == (10, len(data), len(a), -1, CLI)
    assert _table(dx) == want
    # too little room: the capacity answer of the plain call and no index
    n, nf, bf, rc, none = ctx.jam_cli_decompress_ix(d_a, len(a), out, len(data) - 1, check=False)
    assert (rc, n, none) == (E_CAPACITY, 10 * MiB, None)
    # an index of the other kind stays what it was
    assert ctx.jam_index(d_a, len(a)).kind == PLAIN


def test_edges(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, _, d_a, ix = arch
    rs = edge_ranges(bounds)
    assert len(rs) > CALL
    for o in range(0, len(rs), CALL):
        exact(torch, ctx, ix, d_a, len(a), rs[o: o + CALL], data)


def test_order_and_sharing(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, _, d_a, ix = arch
    rs = edge_ranges(bounds) * 2                            # one call of ~1 000 ranges: a large piece table
    assert 800 <= len(rs) <= 4096
    rng = np.random.default_rng(5)
    rs = [rs[i] for i in rng.permutation(len(rs))]
    exact(torch, ctx, ix, d_a, len(a), rs, data)
    f = [bounds[k + 1] - bounds[k] for k in range(10)].index(300000)
    lo, hi = bounds[f], bounds[f + 1]                       # 64 ranges inside the 300 000-byte frame
    inside = []
    for _ in range(64):
        off = int(rng.integers(lo, hi))
        inside.append((off, int(rng.integers(0, min(hi - off, 5000) + 1))))
    exact(torch, ctx, ix, d_a, len(a), inside, data)


def test_whole_range(gpu, arch):
    """one range over everything: every frame's last stage writes in place, at any alignment, and stays inside the buffer"""
    torch, jam, ctx = gpu
    a, data, bounds, _, d_a, ix = arch
    n = len(data)
    ref = torch.full((10 * MiB,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_cli_decompress(d_a, len(a), ref, 10 * MiB)[0] == n
    for lead in (0, 3):
        out = torch.full((lead + n + 4096,), SENT, dtype=torch.uint8, device="cuda")
        st, bad = ctx.jam_read(ix, d_a, len(a), [(0, n)], [out.data_ptr() + lead])
        assert (st, bad) == ([0], -1)
        assert torch.equal(out[lead: lead + n], ref[:n]) and bool((out[:lead] == SENT).all()) and bool((out[lead + n:] == SENT).all())
    # every frame as a range of its own, and the whole again: the second copies from the frames' homes
    rs = [(bounds[k], bounds[k + 1] - bounds[k]) for k in range(10)] + [(0, n)]
    exact(torch, ctx, ix, d_a, len(a), rs, data)


def _damage(a, starts, frame, what):
    b = a.copy()
    if what == "payload":
        b[(starts[frame] + 15 + starts[frame + 1]) // 2] ^= 0x40
    else:
        b[starts[frame] + 3] ^= 1
    return b


def _touches(r, bounds, f):
    return r[1] > 0 and r[0] < bounds[f + 1] and r[0] + r[1] > bounds[f]


def _damage_ranges(bounds):
    raw = bounds[-1]
    return [(0, bounds[3]), (bounds[3] - 1, 1), (bounds[3] - 1, 2), (bounds[3], 1), (bounds[4] - 1, 1), (bounds[4], 1), (bounds[4] - 1, 2),
            (bounds[2], bounds[5] - bounds[2]), (bounds[4], raw - bounds[4]), (0, raw), (bounds[3] + 100, 0), (bounds[6] + 5, 100),
            (bounds[9], 16), (bounds[7], bounds[9] - bounds[7]), (bounds[1], 300), (bounds[3], bounds[4] - bounds[3]), (bounds[5] + 1, 70000)]


def _check_failing(torch, ctx, ix, b, data, bounds, ranges, f):
    """reads of the archive b, whose frame f does not decode to what the index says: only the ranges that touch it fail"""
    d_b = _dev(torch, b)
    st, bad, got, at = read(torch, ctx, ix, d_b, len(b), ranges, check=False)
    failed = {i for i, r in enumerate(ranges) if _touches(r, bounds, f)}
    assert st == [E_CORRUPT if i in failed else OK for i in range(len(ranges))]
    assert bad == (f if failed else -1)
    want = image(data, ranges, at, len(got), skip=failed)
    keep = np.ones(len(got), dtype=bool)                    # the buffer of a failed range is unspecified, everything else is not
    for i in failed:
        keep[at[i]: at[i] + ranges[i][1]] = False
    assert np.array_equal(got[keep], want[keep])
    return d_b, failed


@pytest.mark.parametrize("what", ["payload", "crc"])
def test_damage_after_indexing(gpu, arch, what):
    torch, jam, ctx = gpu
    a, data, bounds, starts, _, ix = arch
    b = _damage(a, starts, 3, what)
    rs = _damage_ranges(bounds)
    d_b, failed = _check_failing(torch, ctx, ix, b, data, bounds, rs, 3)
    good_behind = [i for i, r in enumerate(rs) if i not in failed and r[1] > 0 and r[0] >= bounds[4]]
    assert len(failed) >= 6 and len(good_behind) >= 4       # delivered although they lie behind the bad frame
    # without a status array the call returns the first failing range's status
    import ctypes as C
    outs = [torch.empty(max(r[1], 1), dtype=torch.uint8, device="cuda") for r in rs]
    L, P = C.c_int64 * len(rs), C.c_void_p * len(rs)
    bf = C.c_int32(-1)
    rc = jam.lib().jpk_dev_jam_read(ctx._h, ix._h, d_b.data_ptr(), len(b), len(rs), L(*[r[0] for r in rs]), L(*[r[1] for r in rs]),
                                    P(*[o.data_ptr() for o in outs]), None, C.byref(bf))
    assert (rc, bf.value) == (E_CORRUPT, 3)
    with pytest.raises(jam.JampackError) as e:
        ctx.jam_read(ix, d_b, len(b), rs, outs)
    assert e.value.status == E_CORRUPT
    clean = [r for r in rs if not _touches(r, bounds, 3)]
    exact(torch, ctx, ix, d_b, len(b), clean, data)


@pytest.mark.parametrize("what", ["payload", "crc"])
def test_damage_before_indexing(gpu, arch, what):
    torch, jam, ctx = gpu
    a, data, bounds, starts, _, ix = arch
    b = _damage(a, starts, 3, what)
    d_b = _dev(torch, b)
    bx = ctx.jam_cli_index(d_b, len(b))
    assert (bx.frames, bx.raw_len, bx.archive_len, bx.bad_frame, bx.kind) == (3, bounds[3], len(b), 3, CLI)
    assert _table(bx) == _table(ix)[:3]
    rs = edge_ranges(bounds[:4])[:CALL]
    exact(torch, ctx, bx, d_b, len(b), rs + [(0, bounds[3])], data[: bounds[3]])
    hx = jam.jam_cli_index(b)
    assert (hx.frames, hx.raw_len, hx.bad_frame) == (3, bounds[3], 3) and _table(hx) == _table(bx)
    # the whole-archive call stops at the same frame and hands back the same index
    out = torch.empty(10 * MiB, dtype=torch.uint8, device="cuda")
    n, nf, bf, rc, dx = ctx.jam_cli_decompress_ix(d_b, len(b), out, 10 * MiB, check=False)
    assert (rc, n, nf, bf) == (E_CORRUPT, bounds[3], 3, 3)
    assert (dx.frames, dx.bad_frame, dx.kind) == (3, 3, CLI) and _table(dx) == _table(bx)


def test_truncated_archive(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, starts, _, ix = arch
    b = a[: (starts[5] + starts[6]) // 2].copy()
    d_b = _dev(torch, b)
    bx = ctx.jam_cli_index(d_b, len(b))
    assert (bx.frames, bx.raw_len, bx.archive_len, bx.bad_frame) == (5, bounds[5], len(b), 5)
    exact(torch, ctx, bx, d_b, len(b), [(bounds[4] - 3, 40), (0, bounds[5])], data)
    hx = jam.jam_cli_index(b)
    assert (hx.frames, hx.bad_frame) == (5, 5)


def test_changed_archive(gpu, arch, golden):
    """index archive A, read A' with frame 2 replaced by a golden frame of another raw size, padded or trimmed at its end to A's
    length: the frame behind the indexed payload offset is not the indexed one"""
    torch, jam, ctx = gpu
    z, man = golden
    a, data, bounds, starts, _, ix = arch
    old = a[starts[2]: starts[3]]
    other = next(z[c["name"]] for c in man["frames"] if c["n"] != bounds[3] - bounds[2] and len(z[c["name"]]) != len(old))
    b = np.concatenate([a[: starts[2]], other, a[starts[3]:]])
    b = b[: len(a)] if len(b) >= len(a) else np.concatenate([b, np.zeros(len(a) - len(b), dtype=np.uint8)])
    assert len(b) == len(a)
    d_b = _dev(torch, b)
    rs = [(bounds[2], bounds[3] - bounds[2]), (bounds[2] + 5, 10), (bounds[3] - 1, 1), (bounds[1], bounds[3] - bounds[1]), (0, bounds[2]), (bounds[1] + 9, 100)]
    st, bad, got, at = read(torch, ctx, ix, d_b, len(b), rs, check=False)
    assert st == [E_CORRUPT] * 4 + [OK] * 2 and bad == 2
    want = image(data, rs, at, len(got), skip={0, 1, 2, 3})
    keep = np.ones(len(got), dtype=bool)
    for i in range(4):
        keep[at[i]: at[i] + rs[i][1]] = False
    assert np.array_equal(got[keep], want[keep])


def test_same_payload_size_other_raw_size(gpu):
    """two frames of the writer with payloads of one size and raw sizes that differ, swapped behind the index: the last stage's capacity
    is the indexed raw size exactly, so the longer one does not fit and the shorter one does not fill it -- both are corrupt, and neither
    writes outside its range"""
    torch, jam, ctx = gpu
    by_len = {}
    for n in range(4990, 5060):
        f = jam.jam_cli_block_write(np.zeros(n, dtype=np.uint8), MiB)
        by_len.setdefault(len(f), []).append((n, f))
    pair = next((v for v in by_len.values() if len(v) >= 2), None)
    assert pair is not None, "no two zero-filled frames with payloads of one size"
    (n0, f0), (n1, f1) = pair[0], pair[-1]
    assert n0 < n1 and len(f0) == len(f1)
    text = jam.corpus.make("text", 3000, 12)
    head, tail = jam.jam_cli_block_write(text[:1000], MiB), jam.jam_cli_block_write(text[1000:], MiB)
    for (na, fa), (nb, fb) in (((n0, f0), (n1, f1)), ((n1, f1), (n0, f0))):
        a, b = np.concatenate([head, fa, tail]), np.concatenate([head, fb, tail])
        data = np.concatenate([text[:1000], np.zeros(na, dtype=np.uint8), text[1000:]])
        bounds = [0, 1000, 1000 + na, len(data)]
        d_a = _dev(torch, a)
        ix = ctx.jam_cli_index(d_a, len(a))
        assert (ix.frames, ix.raw_len, ix.bad_frame) == (3, len(data), -1)
        rs = [(0, len(data)), (1000, na), (999, 3), (1000 + na - 1, 2), (0, 1000), (1000 + na, 2000), (5, 17), (1000 + na + 1, 1)]
        exact(torch, ctx, ix, d_a, len(a), rs, data)
        _check_failing(torch, ctx, ix, b, data, bounds, rs, 1)


@pytest.fixture(scope="module")
def arch130(gpu, golden):
    """130 copies of the smallest golden frame: two passes of touched frames"""
    torch, jam, ctx = gpu
    z, _ = golden
    f = z[SMALL]
    one = jam.jam_cli_block_read(f, MiB)[0]
    assert len(f) == 2421 and len(one) == 200000
    return np.tile(f, 130), one


def test_two_passes(gpu, arch130):
    torch, jam, ctx = gpu
    a, one = arch130
    n = len(one)
    d_a = _dev(torch, a)
    ix = ctx.jam_cli_index(d_a, len(a))
    assert (ix.frames, ix.raw_len, ix.bad_frame, ix.kind) == (130, 130 * n, -1, CLI)
    assert ix.frame(129) == (129 * n, n, 129 * 2421 + 15, 2421 - 15)
    # every frame is touched by a range that is in it alone and by one that crosses into the next frame
    rs = [(k * n + 7 * k, 100 + k) for k in range(130)] + [((k + 1) * n - 50, 100) for k in range(129)]
    st, bad, got, at = read(torch, ctx, ix, d_a, len(a), rs)
    assert st == [0] * len(rs) and bad == -1
    want = np.full(len(got), SENT, dtype=np.uint8)
    for (off, ln), p in zip(rs, at):
        want[p: p + ln] = np.concatenate([one, one])[off % n: off % n + ln]
    assert np.array_equal(got, want)
    # frame 129 damaged: it is in the second pass, and only its ranges fail
    b = a.copy()
    b[129 * 2421 + 3] ^= 1
    d_b = _dev(torch, b)
    st2, bad2, got2, at2 = read(torch, ctx, ix, d_b, len(b), rs, check=False)
    failed = {i for i, (off, ln) in enumerate(rs) if off + ln > 129 * n}
    assert failed == {129, 258}
    assert st2 == [E_CORRUPT if i in failed else OK for i in range(len(rs))] and bad2 == 129
    keep = np.ones(len(got2), dtype=bool)
    for i in failed:
        keep[at2[i]: at2[i] + rs[i][1]] = False
    assert at2 == at and np.array_equal(got2[keep], want[keep])


def test_host_form(gpu, arch):
    torch, jam, ctx = gpu
    a, data, bounds, _, _, _ = arch
    hx = jam.jam_cli_index(a)
    rs = [(0, 1), (bounds[1] - 1, 2), (bounds[2], 17), (bounds[3] - 17, 33), (bounds[4], bounds[5] - bounds[4]), (bounds[6] + 1, 4097),
          (bounds[8] - 1, 65536), (bounds[9] - 16, 31), (bounds[9], bounds[10] - bounds[9]), (bounds[10] - 1, 1), (bounds[10], 0), (bounds[7] + 3, 0)]
    got = jam.jam_read(a, rs, index=hx)
    assert len(got) == len(rs)
    for (off, ln), g in zip(rs, got):
        assert np.array_equal(g, data[off: off + ln]), (off, ln)
    many = [r for r in edge_ranges(bounds) if r[1] <= 4097][:40]      # more than 16 ranges: one copy back, split on the host
    for (off, ln), g in zip(many, jam.jam_read(a, many, index=hx)):
        assert np.array_equal(g, data[off: off + ln]), (off, ln)
    # a plain index still reads a plain archive in the same process
    text = jam.corpus.make("text", 50000, 13)
    p = jam.jam_compress(text, MiB)
    px = jam.jam_index(p)
    assert (px.kind, hx.kind) == (PLAIN, CLI)
    assert np.array_equal(jam.jam_read(p, [(100, 40000)], index=px)[0], text[100: 40100])
    assert np.array_equal(jam.jam_read(a, [(bounds[2] - 5, 10)], index=hx)[0], data[bounds[2] - 5: bounds[2] + 5])


def test_writers_archive(gpu):
    """3.3 MiB through the stock-CLI writer with the dedupe and the filters, 1 MiB frames: index and edge ranges at every boundary"""
    torch, jam, ctx = gpu
    n = 3 * MiB + 314573
    data = np.concatenate([jam.corpus.make("text", n - MiB, 14), jam.corpus.make("samples16", MiB, 15)])
    data[2 * MiB + 5000: 2 * MiB + 45000] = data[2 * MiB - 300000: 2 * MiB - 260000]        # a long repeat for the dedupe
    a = jam.jam_cli_compress(data, MiB, dedupe=True, filters=True)
    d_a = _dev(torch, a)
    ix = ctx.jam_cli_index(d_a, len(a))
    assert (ix.frames, ix.raw_len, ix.bad_frame, ix.kind) == (4, n, -1, CLI)
    bounds = [0, MiB, 2 * MiB, 3 * MiB, n]
    assert [ix.frame(k)[:2] for k in range(4)] == [(bounds[k], bounds[k + 1] - bounds[k]) for k in range(4)]
    exact(torch, ctx, ix, d_a, len(a), edge_ranges(bounds), data)
