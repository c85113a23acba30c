"""Damaged .jam archives on the device (jpk_debug_jam_scan, jpk_dev_jam_index_recover, jpk_dev_jam_read through a recovered index,
jpk_dev_jam_salvage): the scan kernels give the plausible headers a numpy search gives, whatever the alignment, the window and the
cap; the device index equals the host index, frames and gaps, on every damaged archive of the host tests, under the default limits and
under a window of 64 bytes with 4 candidates; an undamaged archive launches no scan; staged frames the stages refuse become gaps of
their own span; reads and salvage deliver every surviving frame and fail only the damaged one.  Archives sit at odd offsets of guarded
buffers, and the guard behind the archive starts with a plausible header.  BlockSize is 1 MiB throughout.  -m gpu"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import jam_resync_model as jm
import lz_expand_cases as lzc
from test_gpu_jam_staged import gpu  # noqa: F401  (fixture)
from test_jam_archive_host import hostile_cases

pytestmark = pytest.mark.gpu

MiB = 1 << 20
STAGED_BIT = 1 << 30
SENT = 0xA5
OK, E_CAPACITY, E_CORRUPT = 0, -2, -3
SIZES = [6000, 6001, 4097, 5000, 2345]
TILE = 4096                                   # k_jam_scan_*: one wave's tile (4 rows of 1 KiB)


def _place(torch, b, lead=3):
    """b at an odd offset of a device buffer; the guard behind it starts with a plausible header (payload size 0).  -> (tensor, lead)"""
    img = np.full(lead + len(b) + 64, SENT, dtype=np.uint8)
    img[lead: lead + len(b)] = b
    img[lead + len(b): lead + len(b) + 15] = jm.decoy(psize=0)
    t = torch.from_numpy(img).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, lead


def _full(ix):
    return [ix.frame(k) for k in range(ix.frames)], [ix.frame_kind(k) for k in range(ix.frames)], list(ix.gaps), ix.kind, ix.raw_len, ix.archive_len, ix.bad_frame


@pytest.fixture(scope="module")
def arch(gpu):
    """five plain frames of this library (odd sizes of a few KB), their archive and their inputs"""
    _, jam, _ = gpu
    data = jam.corpus.make("text", sum(SIZES), 91)
    parts, o = [], 0
    for n in SIZES:
        parts.append(data[o: o + n])
        o += n
    frames = [jam.jam_block_write(p, MiB) for p in parts]
    return np.concatenate(frames), parts, frames


# ---- 1. the scan kernels against a numpy search --------------------------------------------------------------------------------------
def _plausible(b, in_len, staged_ok):
    """the offsets of plausible headers in b[0..in_len) by a search of its own"""
    raw, out, x = bytes(b[:in_len]), [], -1
    while True:
        x = raw.find(b"JAM", x + 1)
        if x < 0 or x + 15 > in_len:
            return out
        psize, field = struct.unpack("<ii", raw[x + 7: x + 15])
        bs = field & ~STAGED_BIT if staged_ok and field > 0 else field
        if MiB <= bs <= 1000 * MiB and 0 <= psize <= 1000 * MiB and x + 15 + psize <= in_len:
            out.append(x)


def _scan_buffer(i, lead):
    """16 KiB + 40 of junk with headers that start i bytes behind (edge - 14) for a word edge, a row edge and two tile edges of the image,
    a run of JAMJAMJAM..., implausible headers, a staged header, one header that straddles the end and a plausible one in the guard"""
    rng = np.random.default_rng(100 + i)
    in_len = 4 * TILE + 40
    img = rng.integers(0, 256, lead + in_len + 64, dtype=np.uint8)
    img[img == ord("J")] = ord("K")                                    # the only magics are planted ones
    planted = []
    for edge in (256, 1024, TILE, 2 * TILE, 3 * TILE + 16):
        p = edge - 14 + i
        img[p: p + 15] = jm.decoy(psize=int(rng.integers(0, 200)), crc=edge)
        planted.append(p - lead)
    img[600: 600 + 48] = np.frombuffer(b"JAM" * 16, dtype=np.uint8)
    img[648: 648 + 12] = jm.decoy(psize=3)[3:]                          # the last JAM of the run is a plausible header
    img[2000: 2015] = jm.decoy(block_size=MiB - 1)
    img[2100: 2115] = jm.decoy(psize=-1)
    img[2200: 2215] = jm.decoy(psize=in_len)                           # runs past the end
    img[2300: 2315] = jm.decoy(block_size=MiB | STAGED_BIT)            # plausible with staged_ok only
    img[2400: 2415] = jm.decoy(block_size=(MiB | STAGED_BIT) - (1 << 31))              # bit 31 set: never
    end = lead + in_len
    img[end - 7: end + 8] = jm.decoy(psize=0)                           # straddles in_len
    img[end + 8: end + 23] = jm.decoy(psize=0)                          # in the guard
    return img, in_len, planted


def test_scan_offsets_equal_a_numpy_search(gpu):
    torch, jam, ctx = gpu
    calls = 0
    for i in range(15):
        lead = 3 if i % 2 == 0 else 16                                 # an odd address, and an aligned one
        img, in_len, planted = _scan_buffer(i, lead)
        t = torch.from_numpy(img).to("cuda")
        assert t.data_ptr() % 16 == 0
        d_in = t.data_ptr() + lead
        b = img[lead:]
        for staged_ok in (False, True):
            want = _plausible(b, in_len, staged_ok)
            assert all(p in want for p in planted) and (2300 - lead in want) == staged_ok and len(want) >= 6
            assert 2000 - lead not in want and 2400 - lead not in want and in_len - 7 not in want
            h = planted[2]                                             # the header at the tile edge
            variants = [(0, in_len, 4096), (0, in_len, 1), (0, in_len, 4), (0, in_len, len(want)), (0, in_len, len(want) - 1), (5, in_len - 5, 4096),
                        (planted[0] + 1, in_len, 4096), (1021, 3 * TILE, 4096), (h, 1, 4), (h + 1, 1, 4), (h - 1, 1, 4), (in_len - 1, 1, 4), (in_len, 0, 4),
                        (0, 0, 4), (in_len - 20, 20, 4)]
            variants += [(7, h - 7 + e, 4096) for e in range(16)]      # the window ends e bytes into the header at h
            if staged_ok:
                variants = variants[:6]
            for start, window, cap in variants:
                got = ctx.jam_scan(d_in, in_len, start, window, staged_ok, cap)
                assert got == [o for o in want if start <= o < start + window][:cap], (i, staged_ok, start, window, cap)
                calls += 1
        assert np.array_equal(t.cpu().numpy(), img)                    # reads only
    assert calls > 400


def test_scan_argument_checks(gpu):
    torch, jam, ctx = gpu
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    offs, n = (C.c_int64 * 4)(), C.c_int32(0)
    scan = jam.lib().jpk_debug_jam_scan
    assert scan(None, t.data_ptr(), 64, 0, 64, 0, 4, offs, C.byref(n)) == -1
    for start, window, cap in ((-1, 4, 4), (65, 4, 4), (0, -1, 4), (0, (1 << 30) + 1, 4), (0, 4, 0), (0, 4, (1 << 16) + 1)):
        assert scan(ctx._h, t.data_ptr(), 64, start, window, 0, cap, offs, C.byref(n)) == -1, (start, window, cap)
    assert scan(ctx._h, t.data_ptr(), 64, 0, 64, 0, 4, None, C.byref(n)) == -1 and scan(ctx._h, t.data_ptr(), 64, 0, 64, 0, 4, offs, None) == -1
    assert scan(ctx._h, t.data_ptr(), 64, 0, 1 << 30, 0, 4, offs, C.byref(n)) == 0 and n.value == 0


# ---- 2. the device index equals the host index -----------------------------------------------------------------------------------------
def _damaged(a):
    cases = [("undamaged", a), ("empty", a[:0]), ("deep_flip", jm.deep_flip(a))]
    cases += [(name, b) for name, b, _ in hostile_cases(a)] + jm.damage_cases(a)
    # the archive ends inside a header whose other bytes are in the guard behind it
    cases.append(("straddling_header", np.concatenate([a, jm.decoy(psize=0)[:9]])))
    return cases


def _index_all(torch, jam, ctx, a):
    for name, b in _damaged(a):
        host = jam.jam_recover_index(b)
        for lead in (3, 16):
            if name == "straddling_header":
                img = np.full(lead + len(b) + 64, SENT, dtype=np.uint8)
                img[lead: lead + len(b)] = b
                img[lead + len(b): lead + len(b) + 6] = jm.decoy(psize=0)[9:]
                t = torch.from_numpy(img).to("cuda")
            else:
                t, _ = _place(torch, b, lead)
            before = t.cpu().numpy().copy()
            dev = ctx.jam_recover_index(t.data_ptr() + lead, len(b))
            assert _full(dev) == _full(host), (name, lead)
            jm.check_tiling(dev, len(b))
            assert np.array_equal(t.cpu().numpy(), before), name
        if name in ("undamaged", "deep_flip"):
            assert dev.gaps == [] and dev.frames == 5


def test_device_index_equals_host_index(gpu, arch):
    torch, jam, ctx = gpu
    a, parts, frames = arch
    _index_all(torch, jam, ctx, a)
    # what the host tests assert of the oracle's archives holds for this library's frames
    s = jm.starts(a)
    ix = jam.jam_recover_index(dict(_damaged(a))["magic"])
    assert ix.gaps == [(s[2], s[3] - s[2], 2, 0)] and jm.table(ix)[0] == [(o + 15, len(f) - 15) for o, f in zip(s, frames)][:2] + [(s[3] + 15, len(frames[3]) - 15), (s[4] + 15, len(frames[4]) - 15)]
    for name, b in _damaged(a):
        assert jm.table(jam.jam_recover_index(b)) == jm.model(jam, b), name


def test_device_index_under_a_64_byte_window_and_4_candidates(gpu, arch):
    torch, jam, ctx = gpu
    a, parts, frames = arch
    had = os.environ.get("JPK_DEBUG_HOOKS")
    os.environ["JPK_DEBUG_HOOKS"] = "1"
    try:
        assert jam.lib().jpk_debug_jam_recover_limits(64, 4) == 0
        ctx.profile_enable(2)
        _index_all(torch, jam, ctx, a)
        scans = [r for r in ctx.profile_table() if r["name"] == "k_jam_scan_*"]
        assert scans and scans[0]["launches"] > 100                   # the windows were 64 bytes wide
    finally:
        ctx.profile_enable(0)
        assert jam.lib().jpk_debug_jam_recover_limits(0, 0) == 0
        if had is None:
            os.environ.pop("JPK_DEBUG_HOOKS", None)


# ---- 3. an undamaged archive launches no scan ------------------------------------------------------------------------------------------
def test_undamaged_archive_launches_no_scan(gpu, arch):
    torch, jam, ctx = gpu
    a, parts, frames = arch
    t, lead = _place(torch, a)
    try:
        ctx.profile_enable(2)
        ix = ctx.jam_recover_index(t.data_ptr() + lead, len(a))
        names = [r["name"] for r in ctx.profile_table()]
        assert ix.frames == 5 and "k_jam_walk/k_jam_pack" in names and "k_jam_scan_*" not in names
        ref = ctx.jam_index(t.data_ptr() + lead, len(a))
        assert _full(ix) == _full(ref)
        ctx.profile_enable(2)
        t2, _ = _place(torch, dict(_damaged(a))["magic"])
        ctx.jam_recover_index(t2.data_ptr() + lead, len(a))
        assert "k_jam_scan_*" in [r["name"] for r in ctx.profile_table()]
    finally:
        ctx.profile_enable(0)


# ---- 4. kind 2: staged frames the stages refuse ------------------------------------------------------------------------------------------
def _bad_staged_frame(jam):
    """a staged frame by hand whose S1 holds a token with an offset beyond the output: S2 = 00 00 | S1 (stored), structurally valid"""
    name, s1, _, _ = lzc.corrupt_cases()[0]
    assert name == "offset beyond the output"
    s2 = np.concatenate([np.zeros(2, dtype=np.uint8), np.frombuffer(bytes(s1), dtype=np.uint8)])
    p = jam.block_compress(s2)
    return np.concatenate([np.frombuffer(b"JAM" + struct.pack("<Iii", 0x1234, len(p), MiB | STAGED_BIT), dtype=np.uint8), p])


def test_kind_2_staged_frames_the_stages_refuse_become_gaps(gpu, arch):
    torch, jam, ctx = gpu
    a, parts, frames = arch
    s_good = jam.jam_staged_block_write(parts[1], MiB, flags=5)
    s_flip = jam.jam_staged_block_write(parts[2], MiB, flags=1).copy()
    s_flip[len(s_flip) - 8] ^= 0x10                                     # deep in its rANS data: structurally valid, fails its decode or its crc
    s_bad = _bad_staged_frame(jam)
    for verify, mid in ((True, s_flip), (False, s_bad), (True, s_bad)):
        fr = [frames[0], s_good, mid, frames[3], frames[4]]
        b = np.concatenate(fr)
        st = np.cumsum([0] + [len(f) for f in fr])
        t, lead = _place(torch, b)
        dev = ctx.jam_recover_index(t.data_ptr() + lead, len(b), jam.JAM_INDEX_STAGED, verify)
        assert dev.kind == 2 and dev.gaps == [(int(st[2]), len(mid), 2, jam.JAM_GAP_STAGE)], verify
        assert jm.table(dev)[0] == [(int(st[k]) + 15, len(fr[k]) - 15) for k in (0, 1, 3, 4)]
        assert [dev.frame_kind(k) for k in range(4)] == [0, 2, 0, 0]
        assert [dev.frame(k)[1] for k in range(4)] == [SIZES[0], SIZES[1], SIZES[3], SIZES[4]]
        jm.check_tiling(dev, len(b))
        assert _full(jam.jam_recover_index(b, jam.JAM_INDEX_STAGED, verify)) == _full(dev)      # the host form stages pass by pass
        # a header lost in front of the refused frame: two gaps, back to back, each with its reason
        c = b.copy(); c[st[1]] ^= 1
        t, lead = _place(torch, c)
        dev = ctx.jam_recover_index(t.data_ptr() + lead, len(c), jam.JAM_INDEX_STAGED, verify)
        assert dev.gaps == [(int(st[1]), len(s_good), 1, jam.JAM_GAP_NOFRAME), (int(st[2]), len(mid), 1, jam.JAM_GAP_STAGE)]
        assert _full(jam.jam_recover_index(c, jam.JAM_INDEX_STAGED, verify)) == _full(dev)
        jm.check_tiling(dev, len(c))
        # the surviving frames read back through the index
        outs = [torch.empty(dev.frame(k)[1], dtype=torch.uint8, device="cuda") for k in range(dev.frames)]
        ctx.jam_read(dev, t.data_ptr() + lead, len(c), [dev.frame(k)[:2] for k in range(dev.frames)], outs)
        for o, k in zip(outs, (0, 3, 4)):
            assert np.array_equal(o.cpu().numpy(), parts[k])
    # a plain index refuses staged frames: they are gaps without a reason of their own
    plain = jam.jam_recover_index(b)
    assert plain.frames == 3 and [g[3] for g in plain.gaps] == [0]


# ---- 5 and 6. reads and salvage through a recovered index ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wreck(arch):
    """frame 1 lost (its magic), frame 3 flipped deep in its rANS data: the index holds frames 0, 2, 3, 4 and frame 3 fails its read"""
    a, parts, frames = arch
    s = jm.starts(a)
    b = jm.deep_flip(a, 3)
    b[s[1] + 2] ^= 0x20
    return b, [parts[0], parts[2], parts[3], parts[4]]


def test_reads_through_a_recovered_index(gpu, arch, wreck):
    torch, jam, ctx = gpu
    b, src = wreck
    s = jm.starts(arch[0])
    t, lead = _place(torch, b)
    ix = ctx.jam_recover_index(t.data_ptr() + lead, len(b))
    assert ix.frames == 4 and ix.gaps == [(s[1], s[2] - s[1], 1, 0)]
    ranges = [ix.frame(k)[:2] for k in range(4)] + [(ix.frame(2)[0] - 10, 20), (ix.frame(3)[0] - 1, 1), (ix.frame(3)[0], 1)]
    outs = [torch.full((ln + 32,), SENT, dtype=torch.uint8, device="cuda") for _, ln in ranges]
    status, bad = ctx.jam_read(ix, t.data_ptr() + lead, len(b), ranges, [o.data_ptr() + 16 for o in outs], check=False)
    assert status == [OK, OK, E_CORRUPT, OK, E_CORRUPT, E_CORRUPT, OK] and bad == 2
    raw = np.concatenate(src)
    for r in (0, 1, 3, 6):
        off, ln = ranges[r]
        got = outs[r].cpu().numpy()
        assert np.array_equal(got[16: 16 + ln], raw[off: off + ln]) and (got[:16] == SENT).all() and (got[16 + ln:] == SENT).all(), r
    # the host form through the host index
    hix = jam.jam_recover_index(b)
    for k in (0, 1, 3):
        assert np.array_equal(jam.jam_read(b, [hix.frame(k)[:2]], hix)[0], src[k])
    with pytest.raises(jam.JampackError) as e:
        jam.jam_read(b, [hix.frame(2)[:2]], hix)
    assert e.value.status == E_CORRUPT


def _salvage(jam, ctx, ix, d_in, in_len, d_out, out_cap):
    st = (C.c_int32 * max(ix.frames, 1))(*([-9] * max(ix.frames, 1)))
    n, failed = C.c_int64(-9), C.c_int32(-9)
    rc = jam.lib().jpk_dev_jam_salvage(ctx._h, ix._h, d_in, in_len, d_out, out_cap, C.byref(n), st, C.byref(failed))
    return rc, n.value, list(st)[: ix.frames], failed.value


def test_salvage_delivers_everything_recoverable(gpu, arch, wreck):
    torch, jam, ctx = gpu
    b, src = wreck
    want = np.concatenate([src[0], src[1], np.zeros(len(src[2]), dtype=np.uint8), src[3]])
    t, lead = _place(torch, b)
    ix = ctx.jam_recover_index(t.data_ptr() + lead, len(b))
    assert ix.raw_len == len(want)
    out = torch.full((len(want) + 64,), SENT, dtype=torch.uint8, device="cuda")
    # one byte short: the capacity answer, nothing written
    assert _salvage(jam, ctx, ix, t.data_ptr() + lead, len(b), out.data_ptr() + 17, len(want) - 1)[:2] == (E_CAPACITY, len(want))
    assert (out.cpu().numpy() == SENT).all()
    rc, n, status, failed = _salvage(jam, ctx, ix, t.data_ptr() + lead, len(b), out.data_ptr() + 17, len(want))
    assert (rc, n, status, failed) == (OK, len(want), [OK, OK, E_CORRUPT, OK], 1)
    got = out.cpu().numpy()
    assert np.array_equal(got[17: 17 + len(want)], want) and (got[:17] == SENT).all() and (got[17 + len(want):] == SENT).all()
    assert ctx.jam_salvage(ix, t.data_ptr() + lead, len(b), out.data_ptr() + 17, len(want) + 5) == (len(want), [OK, OK, E_CORRUPT, OK])
    with pytest.raises(jam.JampackError) as e:
        ctx.jam_salvage(ix, t.data_ptr() + lead, len(b), out.data_ptr() + 17, 0)
    assert e.value.status == E_CAPACITY
    # the host form agrees, with an index of its own and with the device's
    for index in (None, ix):
        h_out, h_status = jam.jam_salvage(b, index)
        assert np.array_equal(h_out, want) and h_status == status
    # an undamaged archive: the bytes of jam_decompress, through a recovered index and through a plain one
    a, parts, frames = arch
    t, lead = _place(torch, a)
    raw = jam.jam_decompress(a)
    assert np.array_equal(raw, np.concatenate(parts))
    for ix in (ctx.jam_recover_index(t.data_ptr() + lead, len(a)), ctx.jam_index(t.data_ptr() + lead, len(a))):
        out = torch.full((len(raw) + 64,), SENT, dtype=torch.uint8, device="cuda")
        rc, n, status, failed = _salvage(jam, ctx, ix, t.data_ptr() + lead, len(a), out.data_ptr() + 1, len(raw) + 63)
        assert (rc, n, status, failed) == (OK, len(raw), [OK] * 5, 0)
        got = out.cpu().numpy()
        assert np.array_equal(got[1: 1 + len(raw)], raw) and got[0] == SENT and (got[1 + len(raw):] == SENT).all()
    assert np.array_equal(jam.jam_salvage(a)[0], raw)
    # an index that stops at a bad frame (a plain creator's) is salvaged up to there
    pix = ctx.jam_index(t.data_ptr() + lead, len(a))
    assert pix.gaps == []
