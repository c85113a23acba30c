"""The index and the range reads of archives with staged frames on the device (jpk_dev_blocks_lz77_sizes, jpk_dev_jam_staged_index_create,
jpk_dev_jam_staged_decompress_ix, jpk_dev_jam_read / jpk_jam_read on an index of kind 2): the size kernel answers what the serial LZ77
kernel answers without its bytes; the three sources of an index give one table; every range equals the slice of the raw bytes whatever
its edges, order and destination, and nothing outside the ranges is written; damage fails only the ranges that touch the damaged frame,
a plain or a staged one; a frame that decodes to another size than the indexed one is corrupt; the pass edge.  BlockSize is 1 MiB
throughout.  -m gpu"""
import ctypes as C
import struct

import numpy as np
import pytest

import dedupe_cases
import lz_expand_cases as lzc
from test_gpu_jam_read import SENT, edge_ranges, image
from test_gpu_jam_staged import _compress, archives, data, gpu, mixed  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

MiB = 1 << 20
STAGED_BIT = 1 << 30
OK, E_ARG, E_CAPACITY, E_CORRUPT = 0, -1, -2, -3
PLAIN, STAGED = 0, 2
FLAGS = (0, 1, 4, 5)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _u8(x):
    return np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def _table(ix):
    return [ix.frame(k) for k in range(ix.frames)]


def _kinds(ix):
    return [ix.frame_kind(k) for k in range(ix.frames)]


def _info(ix):
    return ix.kind, ix.frames, ix.raw_len, ix.archive_len, ix.bad_frame


def _headers(a):
    """[(frame start, payload size, BlockSize field)] by a walk of the headers"""
    out, o = [], 0
    while o < len(a):
        _, _, psize, field = struct.unpack("<3sIii", bytes(a[o: o + 15]))
        out.append((o, psize, field))
        o += 15 + psize
    assert o == len(a)
    return out


# ---- 1. the size kernel against the serial kernel ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def streams(gpu):
    """[(name, stream, exact out_cap)]: the crafted token streams, valid and corrupt (a corrupt one at the capacity its case names), the
    S1 streams the dedupe makes of its cases, and an input of no bytes"""
    _, jam, _ = gpu
    out = []
    for name, s, cap, _ in lzc.valid_cases() + lzc.corrupt_cases():
        out.append((name, _u8(s), len(jam.Lz77().Decompress(_u8(s), 1 << 20)) if cap is None else cap))
    for name, t in dedupe_cases.cases().items():
        out.append(("dedupe " + name, jam.Lz77().dedupe(t), len(t)))
    out.append(("no input", np.zeros(0, dtype=np.uint8), 0))
    return out


def test_size_kernel_against_the_serial_kernel(gpu, streams):
    torch, jam, ctx = gpu
    # every stream at an odd offset of one device buffer, 32 bytes apart at least
    at, pos = [], 1
    for _, s, _ in streams:
        at.append(pos)
        pos += (len(s) + 32) | 1
    img = np.full(pos + 64, SENT, dtype=np.uint8)
    for (_, s, _), p in zip(streams, at):
        img[p: p + len(s)] = s
    d_in = _dev(torch, img)
    ins, lens = [d_in.data_ptr() + p for p in at], [len(s) for _, s, _ in streams]
    outs = [torch.empty(cap + 64, dtype=torch.uint8, device="cuda") for _, _, cap in streams]
    seen = set()
    for which in ("exact", "exact - 1", "0"):
        caps = [cap if which == "exact" else max(cap - 1, 0) if which == "exact - 1" else 0 for _, _, cap in streams]
        want_len, want_st = ctx.blocks_lz77_decompress(ins, lens, outs, caps)
        got_len, got_st = ctx.blocks_lz77_sizes(ins, lens, caps)
        for i, (name, s, _) in enumerate(streams):
            assert (got_len[i], got_st[i]) == (want_len[i], want_st[i]), (name, which, caps[i])
            one_len, one_st = ctx.blocks_lz77_sizes(ins[i: i + 1], lens[i: i + 1], caps[i: i + 1])          # alone: n = 1
            assert (one_len, one_st) == ([want_len[i]], [want_st[i]]), (name, which, "alone")
            # the host form is the same rule
            n = C.c_int32(-1)
            assert jam.lib().jpk_lz77_size(s.ctypes.data if len(s) else None, len(s), caps[i], C.byref(n)) == want_st[i] and n.value == want_len[i], (name, which)
        seen |= set(want_st)
        if which == "exact":
            assert [want_len[i] for i, (name, _, _) in enumerate(streams) if name.startswith("dedupe ")] == [c for name, _, c in streams if name.startswith("dedupe ")]
    assert seen == {OK, E_CAPACITY, E_CORRUPT}
    # without a status array the call answers with the first failing block's status
    n = len(streams)
    P, I = C.c_void_p * n, C.c_int32 * n
    assert jam.lib().jpk_dev_blocks_lz77_sizes(ctx._h, n, P(*ins), I(*lens), I(*([0] * n)), I(), None) == E_CAPACITY
    assert np.array_equal(d_in.cpu().numpy(), img)                     # the inputs are as they were


# ---- 2. the index ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(gpu, data, archives, mixed):
    """name -> (archive, raw bytes, raw sizes of the frames, their kinds): the four archives of the writer and the two mixed ones"""
    frames, parts = mixed
    out = {f"flags {fl}": (archives[fl], data, [MiB, MiB, len(data) - 2 * MiB], [STAGED] * 3) for fl in FLAGS}
    out["p|s|p"] = (np.concatenate(frames), np.concatenate(parts), [len(p) for p in parts], [PLAIN, STAGED, PLAIN])
    out["s|p|s"] = (np.concatenate([frames[1], frames[0], frames[1]]), np.concatenate([parts[1], parts[0], parts[1]]),
                    [len(parts[1]), len(parts[0]), len(parts[1])], [STAGED, PLAIN, STAGED])
    return out


NAMES = [f"flags {fl}" for fl in FLAGS] + ["p|s|p", "s|p|s"]


@pytest.mark.parametrize("name", NAMES)
def test_index_from_three_sources(gpu, cases, name):
    torch, jam, ctx = gpu
    a, raw, sizes, kinds = cases[name]
    d_a = _dev(torch, a)
    offs = [0] + [int(x) for x in np.cumsum(sizes)]
    want = [(offs[k], sizes[k], o + 15, psize) for k, (o, psize, _) in enumerate(_headers(a))]
    assert [bool(f & STAGED_BIT) for _, _, f in _headers(a)] == [k == STAGED for k in kinds]
    ix0, ix1 = ctx.jam_staged_index(d_a, len(a), verify=False), ctx.jam_staged_index(d_a, len(a), verify=True)
    out = torch.full((len(raw) + 64,), SENT, dtype=torch.uint8, device="cuda")
    n, nf, bf, dx = ctx.jam_staged_decompress_ix(d_a, len(a), out, len(raw))
    assert (n, nf, bf) == (len(raw), 3, -1) and np.array_equal(out.cpu().numpy()[:n], raw) and bool((out[n:] == SENT).all())
    for ix in (ix0, ix1, dx):
        assert _info(ix) == (STAGED, 3, len(raw), len(a), -1)
        assert _table(ix) == want and _kinds(ix) == kinds
    if name in ("flags 5", "p|s|p"):                                  # the host creator: staged through the pooled context
        for verify in (False, True):
            hx = jam.jam_staged_index(a, verify=verify)
            assert _info(hx) == (STAGED, 3, len(raw), len(a), -1) and _table(hx) == want and _kinds(hx) == kinds


def test_plain_archive_indexes_to_the_plain_table(gpu, data):
    torch, jam, ctx = gpu
    a = jam.jam_compress(data[: MiB + 5001], MiB)
    d_a = _dev(torch, a)
    px = ctx.jam_index(d_a, len(a))
    for verify in (False, True):
        ix = ctx.jam_staged_index(d_a, len(a), verify=verify)
        assert _info(ix) == (STAGED, 2, MiB + 5001, len(a), -1) and _table(ix) == _table(px) and _kinds(ix) == [PLAIN, PLAIN]
    assert (px.kind, _kinds(px)) == (PLAIN, [PLAIN, PLAIN])
    # the creators of the other kinds go on refusing a staged frame
    s = jam.jam_staged_compress(data[:5000], MiB)
    d_s = _dev(torch, s)
    assert (ctx.jam_index(d_s, len(s)).bad_frame, ctx.jam_cli_index(d_s, len(s)).bad_frame) == (0, 0)


# ---- 3. reads ----------------------------------------------------------------------------------------------------------------------------
def read(torch, ctx, ix, d_a, alen, ranges, check=True):
    """the ranges into ONE sentinel-filled buffer, every range at an odd address with 64 spare bytes behind it; returns (status, bad
    frame, the whole buffer, where every range starts in it)"""
    at, pos = [], 0
    for i, (_, ln) in enumerate(ranges):
        pos = (pos + 15) // 16 * 16 + 2 * (i % 8) + 1
        at.append(pos)
        pos += ln + 64
    buf = torch.full((pos + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and all((buf.data_ptr() + p) % 2 == 1 for p in at)
    st, bad = ctx.jam_read(ix, d_a, alen, ranges, [buf.data_ptr() + p for p in at], check=check)
    return st, bad, buf.cpu().numpy(), at


def exact(torch, ctx, ix, d_a, alen, ranges, raw):
    st, bad, got, at = read(torch, ctx, ix, d_a, alen, ranges)
    assert st == [0] * len(ranges) and bad == -1
    want = image(raw, ranges, at, len(got))
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        r = max(k for k, p in enumerate(at) if p <= i) if at[0] <= i else -1
        raise AssertionError(f"byte {i} of the buffer differs (range {r}: {ranges[r]} at {at[r]})")


def _ranges_of(offs):
    """ranges for three frames at the raw offsets offs; in every archive here frame 1 or both its neighbours are staged ones"""
    raw = offs[-1]
    return [(offs[1] + 1000, 4096), (offs[1] + 5, 1), (5, 17), (offs[2] + 9, 300),           # inside one frame
            (offs[1] - 17, 40), (offs[2] - 1, 2), (offs[2] - 4000, 70000),                   # across the edges between plain and staged frames
            (offs[1], offs[2] - offs[1]), (0, offs[1]),                                      # exactly one frame: decoded in place
            (0, raw),                                                                        # the whole archive
            (0, 0), (offs[1], 0), (offs[2], 0), (raw, 0),                                    # zero length: at 0, at frame edges, at raw_len
            (offs[2] + 9, 300), (5, 17), (offs[2] + 9, 300), (offs[1] + 1000, 4096), (0, offs[2]), (offs[1] - 1, raw - offs[1] + 1)]   # unsorted, overlapping, identical


@pytest.mark.parametrize("name", ["flags 0", "flags 5", "p|s|p", "s|p|s"])
def test_reads(gpu, cases, name):
    torch, jam, ctx = gpu
    a, raw, sizes, kinds = cases[name]
    d_a = _dev(torch, a)
    offs = [0] + [int(x) for x in np.cumsum(sizes)]
    n = len(raw)
    for verify in (False, True):
        ix = ctx.jam_staged_index(d_a, len(a), verify=verify)
        exact(torch, ctx, ix, d_a, len(a), _ranges_of(offs), raw)
    exact(torch, ctx, ix, d_a, len(a), edge_ranges(offs)[:200], raw)
    # the whole archive alone is the decompress output, in place at an odd address, and stays inside its buffer
    ref = torch.full((n + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_staged_decompress(d_a, len(a), ref, n) == (n, 3, -1)
    out = torch.full((3 + n + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_read(ix, d_a, len(a), [(0, n)], [out.data_ptr() + 3]) == ([0], -1)
    assert torch.equal(out[3: 3 + n], ref[:n]) and bool((out[:3] == SENT).all()) and bool((out[3 + n:] == SENT).all())
    # a range that ends one byte behind raw_len: JPK_E_ARG, nothing written, whatever the other ranges are
    buf = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(jam.JampackError) as e:
        ctx.jam_read(ix, d_a, len(a), [(0, 100), (n - 5, 6)], [buf.data_ptr() + 1, buf.data_ptr() + 1001])
    assert e.value.status == E_ARG and bool((buf == SENT).all())
    with pytest.raises(jam.JampackError) as e:                        # another archive length than the indexed one
        ctx.jam_read(ix, d_a, len(a) - 1, [(0, 100)], [buf.data_ptr() + 1])
    assert e.value.status == E_ARG and bool((buf == SENT).all())


@pytest.mark.parametrize("name", ["flags 5", "p|s|p"])
def test_host_form(gpu, cases, name):
    _, jam, _ = gpu
    a, raw, sizes, _ = cases[name]
    offs = [0] + [int(x) for x in np.cumsum(sizes)]
    hx = jam.jam_staged_index(a)
    rs = _ranges_of(offs)
    assert len(rs) > 16                                               # one copy back, split on the host
    for some in (rs, rs[:6]):
        got = jam.jam_read(a, some, index=hx)
        assert len(got) == len(some)
        for (off, ln), g in zip(some, got):
            assert np.array_equal(g, raw[off: off + ln]), (off, ln)
    # without an index the archive is taken for a plain one, as before
    with pytest.raises(jam.JampackError):
        jam.jam_read(a, [(offs[1], 10)])


# ---- 4. / 5. damage ----------------------------------------------------------------------------------------------------------------------
def _touches(r, offs, f):
    return r[1] > 0 and r[0] < offs[f + 1] and r[0] + r[1] > offs[f]


def _check_failing(torch, ctx, ix, b, raw, offs, ranges, bad_frames):
    """reads of the archive b, whose frames bad_frames do not decode to what their crcs say: only the ranges that touch one fail"""
    d_b = _dev(torch, b)
    st, bad, got, at = read(torch, ctx, ix, d_b, len(b), ranges, check=False)
    failed = {i for i, r in enumerate(ranges) if any(_touches(r, offs, f) for f in bad_frames)}
    assert st == [E_CORRUPT if i in failed else OK for i in range(len(ranges))]
    touched_bad = [f for f in sorted(bad_frames) if any(_touches(r, offs, f) for r in ranges)]
    assert bad == (touched_bad[0] if touched_bad else -1)
    want = image(raw, ranges, at, len(got), skip=failed)
    keep = np.ones(len(got), dtype=bool)                              # the buffer of a failed range is unspecified, everything else is not
    for i in failed:
        keep[at[i]: at[i] + ranges[i][1]] = False
    assert np.array_equal(got[keep], want[keep])
    return failed


def _damage(a, frame, what):
    h = _headers(a)
    b = a.copy()
    if what == "payload":
        b[h[frame][0] + 15 + h[frame][1] // 2] ^= 0x10
    elif what == "crc":
        b[h[frame][0] + 4] ^= 1
    else:
        b[h[frame][0] + 14] &= 0xBF                                    # bit 30 of the BlockSize field
    return b


@pytest.mark.parametrize("what", ["staged payload", "staged crc", "plain payload", "two frames"])
def test_damage_after_indexing(gpu, cases, what):
    torch, jam, ctx = gpu
    a, raw, sizes, _ = cases["p|s|p"]
    offs = [0] + [int(x) for x in np.cumsum(sizes)]
    ix = ctx.jam_staged_index(_dev(torch, a), len(a))
    b, bad = {"staged payload": (_damage(a, 1, "payload"), {1}), "staged crc": (_damage(a, 1, "crc"), {1}), "plain payload": (_damage(a, 2, "payload"), {2}),
              "two frames": (_damage(_damage(a, 1, "payload"), 0, "payload"), {0, 1})}[what]
    rs = _ranges_of(offs)
    failed = _check_failing(torch, ctx, ix, b, raw, offs, rs, bad)
    assert 0 < len(failed) < len([r for r in rs if r[1] > 0])           # some ranges fail and some are delivered
    # the damaged frame is not touched at all: everything is delivered
    clean = [r for r in rs if not any(_touches(r, offs, f) for f in bad)] + [(offs[f], sizes[f]) for f in range(3) if f not in bad]
    exact(torch, ctx, ix, _dev(torch, b), len(b), clean, raw)


def test_damage_before_indexing(gpu, cases):
    torch, jam, ctx = gpu
    a, raw, sizes, kinds = cases["p|s|p"]
    offs = [0] + [int(x) for x in np.cumsum(sizes)]
    good = _table(ctx.jam_staged_index(_dev(torch, a), len(a)))
    rs = _ranges_of(offs)
    # the header crc of staged frame 1: verify = 1 ends the index in front of it, verify = 0 cannot see it -- the read does
    b = _damage(a, 1, "crc")
    d_b = _dev(torch, b)
    v1, v0 = ctx.jam_staged_index(d_b, len(b), verify=True), ctx.jam_staged_index(d_b, len(b), verify=False)
    assert _info(v1) == (STAGED, 1, offs[1], len(b), 1) and _table(v1) == good[:1]
    assert _info(v0) == (STAGED, 3, len(raw), len(b), -1) and _table(v0) == good and _kinds(v0) == kinds
    _check_failing(torch, ctx, v0, b, raw, offs, rs, {1})
    exact(torch, ctx, v1, d_b, len(b), [(0, offs[1]), (5, 17), (offs[1], 0)], raw)
    hx = jam.jam_staged_index(b, verify=True)
    assert _info(hx) == _info(v1) and _table(hx) == _table(v1)
    # a payload byte: the index without verification ends at that frame or holds it; the frames in front are indexed as they were
    b = _damage(a, 1, "payload")
    d_b = _dev(torch, b)
    v1, v0 = ctx.jam_staged_index(d_b, len(b), verify=True), ctx.jam_staged_index(d_b, len(b), verify=False)
    assert _info(v1) == (STAGED, 1, offs[1], len(b), 1)
    assert (v0.frames, v0.bad_frame) in ((1, 1), (3, -1)) and _table(v0)[:1] == good[:1]
    exact(torch, ctx, v0, d_b, len(b), [(0, offs[1]), (5, 17)], raw)
    if v0.frames == 3 and v0.frame(1)[1] > 0:
        o1 = v0.frame(1)[0]
        st, bad = ctx.jam_read(v0, d_b, len(b), [(5, 17), (o1, 1)], [torch.empty(64, dtype=torch.uint8, device="cuda").data_ptr() + 1] * 2, check=False)
        assert (st, bad) == ([OK, E_CORRUPT], 1)


@pytest.mark.parametrize("fl", [0, 4])
def test_bit_30_cleared_ends_the_index(gpu, cases, fl):
    """Without bit 30 the header is a plain frame's.  Frame 1 of these archives is a full slice without the dedupe: its payload declares
    |S2| = 1 MiB + 2 + 2 * 17 bytes, more than BlockSize, which no plain frame may -- the walk ends there, verified or not."""
    torch, jam, ctx = gpu
    a, raw, sizes, _ = cases[f"flags {fl}"]
    good = _table(ctx.jam_staged_index(_dev(torch, a), len(a)))
    b = _damage(a, 1, "bit 30")
    d_b = _dev(torch, b)
    for verify in (False, True):
        ix = ctx.jam_staged_index(d_b, len(b), verify=verify)
        assert _info(ix) == (STAGED, 1, MiB, len(b), 1) and _table(ix) == good[:1]
    exact(torch, ctx, ix, d_b, len(b), [(0, MiB), (MiB - 3, 3), (MiB, 0)], raw)
    assert _info(jam.jam_staged_index(b)) == (STAGED, 1, MiB, len(b), 1)


def test_bit_30_cleared_on_a_short_frame_fails_the_read(gpu, cases):
    """The staged frame of the mixed archive is short: without bit 30 its header is that of a VALID plain frame of |S2| bytes, which an index
    holds as it holds every plain frame, undecoded.  The read decodes it and it misses its crc (that of R): the frame is never delivered."""
    torch, jam, ctx = gpu
    a, raw, sizes, _ = cases["p|s|p"]
    b = _damage(a, 1, "bit 30")
    d_b = _dev(torch, b)
    ix = ctx.jam_staged_index(d_b, len(b))
    assert (ix.frames, ix.bad_frame, _kinds(ix)) == (3, -1, [PLAIN] * 3) and ix.frame(1)[1] > sizes[1]
    o = [ix.frame(k)[0] for k in range(3)]
    buf = torch.empty(4096, dtype=torch.uint8, device="cuda")
    st, bad = ctx.jam_read(ix, d_b, len(b), [(5, 17), (o[1] + 5, 17), (o[2] + 5, 17)], [buf.data_ptr() + 1, buf.data_ptr() + 101, buf.data_ptr() + 201], check=False)
    assert (st, bad) == ([OK, E_CORRUPT, OK], 1)
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:18], raw[5:22]) and np.array_equal(got[201:218], raw[sizes[0] + sizes[1] + 5: sizes[0] + sizes[1] + 22])
    n, nf, bf, rc, dx = ctx.jam_staged_decompress_ix(d_b, len(b), torch.empty(3 * MiB, dtype=torch.uint8, device="cuda"), 3 * MiB, check=False)
    assert (rc, n, nf, bf) == (E_CORRUPT, sizes[0], 1, 1) and (dx.frames, dx.bad_frame) == (1, 1)


# ---- 6. a changed archive ----------------------------------------------------------------------------------------------------------------
def test_same_payload_size_other_raw_size(gpu):
    """two staged frames with payloads of one size and raw sizes that differ, swapped behind the index: the last stage's capacity is the
    indexed raw size exactly, so the longer one does not fit and the shorter one does not fill it -- both are corrupt, never delivered at
    a wrong size, and neither writes outside its range"""
    torch, jam, ctx = gpu
    by_len = {}
    for n in range(4990, 5120):
        f = jam.jam_staged_block_write(np.zeros(n, dtype=np.uint8), MiB)
        by_len.setdefault(len(f), []).append((n, f))
    pair = next((v for v in by_len.values() if len(v) >= 2), None)
    assert pair is not None, "no two zero-filled staged frames with payloads of one size"
    (n0, f0), (n1, f1) = pair[0], pair[-1]
    assert n0 < n1 and len(f0) == len(f1)
    text = jam.corpus.make("text", 3000, 12)
    head, tail = jam.jam_block_write(text[:1000], MiB), jam.jam_staged_block_write(text[1000:], MiB, flags=5)
    for (na, fa), (nb, fb) in (((n0, f0), (n1, f1)), ((n1, f1), (n0, f0))):
        a, b = np.concatenate([head, fa, tail]), np.concatenate([head, fb, tail])
        raw = np.concatenate([text[:1000], np.zeros(na, dtype=np.uint8), text[1000:]])
        offs = [0, 1000, 1000 + na, len(raw)]
        d_a = _dev(torch, a)
        for verify in (False, True):
            ix = ctx.jam_staged_index(d_a, len(a), verify=verify)
            assert _info(ix) == (STAGED, 3, len(raw), len(a), -1) and _kinds(ix) == [PLAIN, STAGED, STAGED]
            rs = [(0, len(raw)), (1000, na), (999, 3), (1000 + na - 1, 2), (0, 1000), (1000 + na, 2000), (5, 17), (1000 + na + 1, 1)]
            exact(torch, ctx, ix, d_a, len(a), rs, raw)
            _check_failing(torch, ctx, ix, b, raw, offs, rs, {1})


# ---- 7. the pass edge --------------------------------------------------------------------------------------------------------------------
def test_130_frames_cross_the_pass_edge(gpu):
    """130 frames of 5000-byte texts, every third one a plain frame: a staged frame weighs its BlockSize, so a pass holds 128 frames"""
    torch, jam, ctx = gpu
    five = [jam.corpus.make("text", 5000, 200 + k) for k in range(5)]
    texts = [five[k % 5] for k in range(130)]
    kinds = [PLAIN if k % 3 == 2 else STAGED for k in range(130)]
    made = {}                                                          # five texts as plain frames and as staged ones of flags 0 and 5: 15 frames to write

    def frame(k):
        key = (k % 5, kinds[k], k % 2)
        if key not in made:
            made[key] = jam.jam_block_write(texts[k], MiB) if kinds[k] == PLAIN else jam.jam_staged_block_write(texts[k], MiB, flags=(0, 5)[k % 2])
        return made[key]
    a = np.concatenate([frame(k) for k in range(130)])
    raw = np.concatenate(texts)
    d_a = _dev(torch, a)
    want = [(5000 * k, 5000, o + 15, psize) for k, (o, psize, _) in enumerate(_headers(a))]
    for verify in (False, True):
        ix = ctx.jam_staged_index(d_a, len(a), verify=verify)
        assert _info(ix) == (STAGED, 130, 650_000, len(a), -1) and _table(ix) == want and _kinds(ix) == kinds
        exact(torch, ctx, ix, d_a, len(a), [(0, 650_000), (129 * 5000 + 77, 1000)], raw)
    # frame 129 is in the second pass: damaged, only its ranges fail
    b = _damage(a, 129, "crc")
    _check_failing(torch, ctx, ix, b, raw, [5000 * k for k in range(131)], [(0, 650_000), (129 * 5000 + 77, 1000), (128 * 5000, 5000), (0, 129 * 5000)], {129})
    v1 = ctx.jam_staged_index(_dev(torch, b), len(b), verify=True)
    assert _info(v1) == (STAGED, 129, 645_000, len(b), 129) and _table(v1) == want[:129]


# ---- 8. the _ix contract -----------------------------------------------------------------------------------------------------------------
def test_ix_contract(gpu, cases):
    torch, jam, ctx = gpu
    a, raw, sizes, kinds = cases["p|s|p"]
    lib = jam.lib()
    n = len(raw)

    def call(arch, cap, with_index):
        d_a = _dev(torch, arch)
        out = torch.full((max(cap, 0) + 64,), SENT, dtype=torch.uint8, device="cuda")
        ln, nf, bf, h = C.c_int64(-1), C.c_int32(-1), C.c_int32(-2), C.c_void_p(1)
        if with_index is None:
            rc = lib.jpk_dev_jam_staged_decompress(ctx._h, d_a.data_ptr(), len(arch), out.data_ptr(), cap, C.byref(ln), C.byref(nf), C.byref(bf))
        else:
            rc = lib.jpk_dev_jam_staged_decompress_ix(ctx._h, d_a.data_ptr(), len(arch), out.data_ptr(), cap, C.byref(ln), C.byref(nf), C.byref(bf),
                                                      C.byref(h) if with_index else None)
        return (rc, ln.value, nf.value, bf.value), out.cpu().numpy(), h

    bad1 = _damage(a, 1, "payload")
    for arch, cap in ((a, n), (a, n - 1), (a, 0), (bad1, n), (np.zeros(0, dtype=np.uint8), 0)):
        want, img, _ = call(arch, cap, None)
        res, img2, _ = call(arch, cap, False)                          # index == NULL: the plain call
        assert res == want and np.array_equal(img, img2), (cap, res, want)
        res, img3, h = call(arch, cap, True)
        assert res == want and np.array_equal(img, img3), (cap, res, want)
        if want[0] == E_CAPACITY:
            assert not h                                              # *index is NULL after JPK_E_CAPACITY
            continue
        ix = jam.JamIndex(h, want[3])
        if len(arch) == 0:
            assert _info(ix) == (STAGED, 0, 0, 0, -1)
        elif arch is a:
            assert want == (OK, n, 3, -1) and _info(ix) == (STAGED, 3, n, len(a), -1) and _kinds(ix) == kinds
        else:                                                          # a bad frame 1: the index covers frame 0
            assert want == (E_CORRUPT, sizes[0], 1, 1) and _info(ix) == (STAGED, 1, sizes[0], len(a), 1) and _kinds(ix) == [PLAIN]
            assert np.array_equal(img3[: sizes[0]], raw[: sizes[0]])
