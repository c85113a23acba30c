"""Damaged stock-CLI .jam archives on the device (jpk_dev_jam_index_recover with kind JPK_JAM_INDEX_CLI, reads and salvage through the
recovered index, jpk_dev_jam_repair): an undamaged archive gives the table of jpk_dev_jam_cli_index_create and launches no scan; on a
table of damage written down from its construction the device and the host index agree with the expectation -- a lost header is a
NOFRAME gap, a frame that fails its stage chain or its crc a STAGE gap over its own span --, under the default search limits and under a
window of 64 bytes with 4 candidates; a pass ends at frame 128 with damage on both sides of the edge; reads and salvage deliver every
kept frame; a repaired archive decodes to its end, here and (where it was built) by the stock CLI.  Frames are this library's
(jam_cli_block_write, with and without dedupe and filters) and the reference CLI's golden ones.  Archives sit at odd offsets of guarded
buffers, and the guard behind the archive starts with a plausible header.  BlockSize is 1 MiB throughout.  -m gpu"""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import jam_resync_model as jm
from golden_util import GOLD
from test_gpu_jam_staged import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "jampack_ref")
MiB = 1 << 20
SENT = 0xA5
OK, E_ARG, E_CAPACITY, E_CORRUPT = 0, -1, -2, -3
NOFRAME, STAGE = 0, 1
SIZES = [6000, 6001, 4097, 5000, 2345]


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


@pytest.fixture(scope="module", params=["own", "own_dedupe_filters", "golden"])
def fx(request, gpu):
    """(frames, parts): five frames of this library's stock-CLI writer over SIZES, plain or with dedupe and filters, or the eight golden
    frames of the reference CLI with what jam_cli_block_read makes of them"""
    _, jam, _ = gpu
    if request.param == "golden":
        z, man = np.load(os.path.join(GOLD, "golden_cli.npz")), json.load(open(os.path.join(GOLD, "golden_cli_manifest.json")))
        frames = [z[c["name"]] for c in man["frames"]]
        assert len(frames) == 8 and all(c["block_size"] == MiB for c in man["frames"])
        return frames, [jam.jam_cli_block_read(f, MiB)[0] for f in frames]
    data = jam.corpus.make("text", sum(SIZES), 91)
    parts = [data[o: o + n] for o, n in zip(np.cumsum([0] + SIZES[:-1]), SIZES)]
    on = request.param == "own_dedupe_filters"
    return [jam.jam_cli_block_write(p, MiB, dedupe=on, filters=on) for p in parts], parts


def _build(segs):
    """segs: ("ok", frame, part) | ("noframe", bytes) | ("stage", bytes), in archive order -> (archive, the frames [(raw_off, raw, payload_off,
    psize)] and the gaps a stock-CLI recover must give, the kept parts).  NOFRAME bytes that touch are one gap; a STAGE gap is one frame's span."""
    at, raw_at, frames, gaps, kept, out = 0, 0, [], [], [], []
    for s in segs:
        b = s[1]
        if s[0] == "ok":
            frames.append((raw_at, len(s[2]), at + 15, len(b) - 15))
            kept.append(s[2])
            raw_at += len(s[2])
        elif s[0] == "noframe" and gaps and gaps[-1][3] == NOFRAME and gaps[-1][0] + gaps[-1][1] == at:
            gaps[-1] = (gaps[-1][0], gaps[-1][1] + len(b), gaps[-1][2], NOFRAME)
        else:
            gaps.append((at, len(b), len(frames), NOFRAME if s[0] == "noframe" else STAGE))
        at += len(b)
        out.append(b)
    return np.concatenate(out), frames, gaps, kept


def _flip(f, at, bit=1):
    g = f.copy()
    g[at] ^= bit
    return g


def _deep(f):
    """a byte flipped deep in the frame's rANS data, not in a chunk header: structurally valid, fails its decode or its crc"""
    return _flip(f, len(f) - 8, 0x10)


def _psize(f, v):
    g = f.copy()
    jm.put_i32(g, 7, v)
    return g


@pytest.fixture(scope="module")
def oversize(gpu):
    """a frame by hand whose payload is block_compress of BlockSize + 100 zero bytes: more than a plain frame may declare, within what a
    stock-CLI frame may; no stage chain makes its crc of it"""
    _, jam, _ = gpu
    p = jam.block_compress(np.zeros(MiB + 100, dtype=np.uint8))
    return np.concatenate([np.frombuffer(b"JAM" + struct.pack("<Iii", 0x1234, len(p), MiB), dtype=np.uint8), p])


def _damage_table(F, P, oversize):
    """(name, segs) for frames F with parts P: every case names what became of which frame"""
    ok = [("ok", f, p) for f, p in zip(F, P)]
    junk = np.random.default_rng(7).integers(0, 256, 137, dtype=np.uint8)
    junk[junk == ord("J")] = ord("K")
    junk[20: 35] = jm.decoy(psize=100)
    cut = F[-1][: 15 + (len(F[-1]) - 15) // 2]
    rep = lambda k, seg: ok[:k] + [seg] + ok[k + 1:]
    return [("magic_1", rep(1, ("noframe", _flip(F[1], 0)))),
            ("deep_flip_3", rep(3, ("stage", _deep(F[3])))),
            ("crc_2", rep(2, ("stage", _flip(F[2], 3)))),
            ("psize_1_too_large", rep(1, ("noframe", _psize(F[1], (1000 << 20) + 1)))),
            ("psize_1_minus_one", rep(1, ("noframe", _psize(F[1], -1)))),
            ("decoy_junk_2_3", ok[:3] + [("noframe", junk)] + ok[3:]),
            ("truncated_last", ok[:-1] + [("noframe", cut)]),
            ("magic_1_deep_2", ok[:1] + [("noframe", _flip(F[1], 0)), ("stage", _deep(F[2]))] + ok[3:]),
            ("oversize_1_2", ok[:2] + [("stage", oversize)] + ok[2:])]


def _run_table(gpu, fx, oversize):
    """every case of the damage table: the device index equals the expectation and the host index, tiles the archive, reads only -> {name: index}"""
    torch, jam, ctx = gpu
    F, P = fx
    got = {}
    for name, segs in _damage_table(F, P, oversize):
        b, frames, gaps, _ = _build(segs)
        t, lead = _place(torch, b)
        before = t.cpu().numpy().copy()
        dev = ctx.jam_recover_index(t.data_ptr() + lead, len(b), jam.JAM_INDEX_CLI)
        assert dev.kind == 1 and dev.bad_frame == -1, name
        assert [dev.frame(k) for k in range(dev.frames)] == frames, name
        assert dev.gaps == gaps, name
        jm.check_tiling(dev, len(b))
        assert np.array_equal(t.cpu().numpy(), before), name
        assert _full(jam.jam_recover_index(b, jam.JAM_INDEX_CLI)) == _full(dev), name       # the host form stages pass by pass
        if name == "oversize_1_2":
            # a plain walk refuses what it declares: the same span, without a reason of its own
            plain = ctx.jam_recover_index(t.data_ptr() + lead, len(b))
            assert plain.kind == 0 and plain.frames == len(F) and plain.gaps == [gaps[0][:3] + (NOFRAME,)]
        if name == "crc_2":
            assert ctx.jam_recover_index(t.data_ptr() + lead, len(b)).gaps == []             # a plain index keeps the frame
        got[name] = _full(dev)
    assert len(got) == 9
    return got


_DEFAULT = {}


# ---- 4. undamaged ------------------------------------------------------------------------------------------------------------------------
def test_undamaged_archive_gives_the_cli_index_and_launches_no_scan(gpu, fx):
    torch, jam, ctx = gpu
    F, P = fx
    a = np.concatenate(F)
    t, lead = _place(torch, a)
    before = t.cpu().numpy().copy()
    try:
        ctx.profile_enable(2)
        ix = ctx.jam_recover_index(t.data_ptr() + lead, len(a), jam.JAM_INDEX_CLI)
        names = [r["name"] for r in ctx.profile_table()]
    finally:
        ctx.profile_enable(0)
    assert "k_jam_walk/k_jam_pack" in names and "k_jam_scan_*" not in names
    ref = ctx.jam_cli_index(t.data_ptr() + lead, len(a))
    assert ref.bad_frame == -1 and ref.frames == len(F)
    assert _full(ix) == _full(ref) and ix.kind == 1 and ix.gaps == []
    assert [ix.frame(k)[1] for k in range(ix.frames)] == [len(p) for p in P]
    jm.check_tiling(ix, len(a))
    assert np.array_equal(t.cpu().numpy(), before)
    assert _full(jam.jam_recover_index(a, jam.JAM_INDEX_CLI)) == _full(ix)


# ---- 5. the damage table -----------------------------------------------------------------------------------------------------------------
def test_damage_table(gpu, fx, oversize, request):
    _DEFAULT[request.node.callspec.id] = _run_table(gpu, fx, oversize)


# ---- 6. tiny search windows --------------------------------------------------------------------------------------------------------------
def test_damage_table_under_a_64_byte_window_and_4_candidates(gpu, fx, oversize, request):
    torch, jam, ctx = gpu
    had = os.environ.get("JPK_DEBUG_HOOKS")
    os.environ["JPK_DEBUG_HOOKS"] = "1"
    try:
        assert jam.lib().jpk_debug_jam_recover_limits(64, 4) == 0
        ctx.profile_enable(2)
        got = _run_table(gpu, fx, oversize)
        scans = [r for r in ctx.profile_table() if r["name"] == "k_jam_scan_*"]
        assert scans and scans[0]["launches"] > 100                   # the windows were 64 bytes wide
    finally:
        ctx.profile_enable(0)
        assert jam.lib().jpk_debug_jam_recover_limits(0, 0) == 0
        if had is None:
            os.environ.pop("JPK_DEBUG_HOOKS", None)
    want = _DEFAULT.get(request.node.callspec.id) or _run_table(gpu, fx, oversize)
    assert got == want


# ---- 7. pass edges -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(gpu):
    """130 frames of 300 raw bytes: a stock-CLI pass holds 128 of them"""
    _, jam, _ = gpu
    data = jam.corpus.make("text", 130 * 300, 93)
    parts = [data[300 * k: 300 * (k + 1)] for k in range(130)]
    return [jam.jam_cli_block_write(p, MiB) for p in parts], parts


@pytest.mark.parametrize("case", ["127_noframe_128_stage", "128_stage", "60_stage", "60_noframe"])
def test_a_pass_ends_at_frame_128(gpu, many, case):
    torch, jam, ctx = gpu
    F, P = many
    segs = [("ok", f, p) for f, p in zip(F, P)]
    words = case.split("_")
    for k, how in zip(words[0::2], words[1::2]):
        segs[int(k)] = ("noframe", _flip(F[int(k)], 0)) if how == "noframe" else ("stage", _deep(F[int(k)]))
    b, frames, gaps, kept = _build(segs)
    assert len(gaps) == len(words) // 2 and len(frames) == 130 - len(gaps)
    t, lead = _place(torch, b)
    ix = ctx.jam_recover_index(t.data_ptr() + lead, len(b), jam.JAM_INDEX_CLI)
    assert [ix.frame(k) for k in range(ix.frames)] == frames and ix.gaps == gaps and ix.kind == 1
    assert [ix.frame(k)[0] for k in range(ix.frames)] == [300 * k for k in range(ix.frames)]
    jm.check_tiling(ix, len(b))
    assert _full(jam.jam_recover_index(b, jam.JAM_INDEX_CLI)) == _full(ix)
    # the frames on both sides of every gap, and the two ends
    ks = sorted({k for g in gaps for k in (g[2] - 1, g[2]) if 0 <= k < ix.frames} | {0, ix.frames - 1})
    outs = [torch.empty(300, dtype=torch.uint8, device="cuda") for _ in ks]
    ctx.jam_read(ix, t.data_ptr() + lead, len(b), [ix.frame(k)[:2] for k in ks], outs)
    for o, k in zip(outs, ks):
        assert np.array_equal(o.cpu().numpy(), kept[k]), k


# ---- 8. reads and salvage ------------------------------------------------------------------------------------------------------------------
def test_reads_and_salvage_through_a_recovered_index(gpu, fx):
    torch, jam, ctx = gpu
    F, P = fx
    n = len(F)
    segs = [("ok", f, p) for f, p in zip(F, P)]
    segs[1] = ("noframe", _flip(F[1], 0))
    segs[3] = ("stage", _deep(F[3]))
    b, frames, gaps, kept = _build(segs)
    raw = np.concatenate(kept)
    t, lead = _place(torch, b)
    d_in = t.data_ptr() + lead
    ix = ctx.jam_recover_index(d_in, len(b), jam.JAM_INDEX_CLI)
    assert ix.frames == n - 2 and [g[3] for g in ix.gaps] == [NOFRAME, STAGE] and ix.raw_len == len(raw)
    # every kept frame, and ranges over two kept frames that a gap separates in the archive
    ranges = [ix.frame(k)[:2] for k in range(ix.frames)] + [(ix.frame(1)[0] - 10, 20), (ix.frame(2)[0] - 1, 2), (0, len(raw))]
    outs = [torch.full((ln + 32,), SENT, dtype=torch.uint8, device="cuda") for _, ln in ranges]
    status, bad = ctx.jam_read(ix, d_in, len(b), ranges, [o.data_ptr() + 16 for o in outs])
    assert status == [OK] * len(ranges) and bad == -1
    for (off, ln), o in zip(ranges, outs):
        got = o.cpu().numpy()
        assert np.array_equal(got[16: 16 + ln], raw[off: off + ln]) and (got[:16] == SENT).all() and (got[16 + ln:] == SENT).all(), (off, ln)
    out = torch.full((len(raw) + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_salvage(ix, d_in, len(b), out.data_ptr() + 17, len(raw)) == (len(raw), [OK] * ix.frames)
    got = out.cpu().numpy()
    assert np.array_equal(got[17: 17 + len(raw)], raw) and (got[:17] == SENT).all() and (got[17 + len(raw):] == SENT).all()
    # the host forms: through the device's index, and through one of their own
    h_out, h_status = jam.jam_salvage(b, ix)
    assert np.array_equal(h_out, raw) and h_status == [OK] * ix.frames
    h_out, h_status = jam.jam_salvage(b, kind=jam.JAM_INDEX_CLI)
    assert np.array_equal(h_out, raw) and h_status == [OK] * ix.frames
    assert np.array_equal(jam.jam_read(b, [ranges[-3]], ix)[0], raw[ranges[-3][0]: ranges[-3][0] + 20])
    # the archive changes after indexing: kept frame 1 loses a payload byte
    po, ps = ix.frame(1)[2:]
    c = _flip(b, po + ps - 8, 0x10)
    t2, _ = _place(torch, c)
    want = raw.copy()
    want[ix.frame(1)[0]: ix.frame(1)[0] + ix.frame(1)[1]] = 0
    st_want = [OK, E_CORRUPT] + [OK] * (ix.frames - 2)
    out = torch.full((len(raw) + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_salvage(ix, t2.data_ptr() + lead, len(c), out.data_ptr() + 17, len(raw)) == (len(raw), st_want)
    assert np.array_equal(out.cpu().numpy()[17: 17 + len(raw)], want)
    h_out, h_status = jam.jam_salvage(c, ix)
    assert np.array_equal(h_out, want) and h_status == st_want
    # repair with those statuses drops it
    fixed = jam.jam_repair(c, ix, st_want)
    spans = [c[ix.frame(k)[2] - 15: ix.frame(k)[2] + ix.frame(k)[3]] for k in range(ix.frames) if k != 1]
    assert np.array_equal(fixed, np.concatenate(spans))
    d_out = torch.full((len(c) + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert ctx.jam_repair(ix, t2.data_ptr() + lead, len(c), d_out.data_ptr() + 5, len(c), st_want) == (len(fixed), ix.frames - 1)
    got = d_out.cpu().numpy()
    assert np.array_equal(got[5: 5 + len(fixed)], fixed) and (got[:5] == SENT).all() and (got[5 + len(fixed):] == SENT).all()
    assert np.array_equal(jam.jam_cli_decompress_all(fixed), np.concatenate([p for k, p in enumerate(kept) if k != 1]))


# ---- 9. repair closes the loop -------------------------------------------------------------------------------------------------------------
def _repaired(gpu, fx, which):
    """the archive with frame 1's magic flipped or frame 3 flipped deep, repaired on the device at an odd address -> (bytes, kept parts)"""
    torch, jam, ctx = gpu
    F, P = fx
    segs = [("ok", f, p) for f, p in zip(F, P)]
    segs[1 if which == "magic" else 3] = ("noframe", _flip(F[1], 0)) if which == "magic" else ("stage", _deep(F[3]))
    b, frames, gaps, kept = _build(segs)
    t, lead = _place(torch, b)
    before = t.cpu().numpy().copy()
    ix = ctx.jam_recover_index(t.data_ptr() + lead, len(b), jam.JAM_INDEX_CLI)
    assert ix.frames == len(F) - 1 and [g[3] for g in ix.gaps] == [NOFRAME if which == "magic" else STAGE]
    want = jam.jam_repair(b, ix)
    assert len(want) == len(b) - gaps[0][1]
    d_out = torch.full((len(b) + 64,), SENT, dtype=torch.uint8, device="cuda")
    for at in (7, 16):                                                 # an odd address, and an aligned one
        d_out.fill_(SENT)
        assert ctx.jam_repair(ix, t.data_ptr() + lead, len(b), d_out.data_ptr() + at, len(want)) == (len(want), len(F) - 1)
        got = d_out.cpu().numpy()
        assert np.array_equal(got[at: at + len(want)], want) and (got[:at] == SENT).all() and (got[at + len(want):] == SENT).all(), at
    assert np.array_equal(t.cpu().numpy(), before)
    return want, kept


@pytest.mark.parametrize("which", ["magic", "deep_flip"])
def test_a_repaired_archive_decodes_to_its_end(gpu, fx, which):
    torch, jam, ctx = gpu
    fixed, kept = _repaired(gpu, fx, which)
    raw = np.concatenate(kept)
    t, lead = _place(torch, fixed)
    out = torch.full((len(kept) * MiB + 64,), SENT, dtype=torch.uint8, device="cuda")
    n, nf, bf, rc = ctx.jam_cli_decompress(t.data_ptr() + lead, len(fixed), out.data_ptr() + 16, len(kept) * MiB, check=False)
    assert (n, nf, bf, rc) == (len(raw), len(kept), -1, OK)
    assert np.array_equal(out[16: 16 + n].cpu().numpy(), raw)
    got, nf, bf, rc = jam.jam_cli_decompress_all(fixed, check=False)
    assert (nf, bf, rc) == (len(kept), -1, OK) and np.array_equal(got, raw)
    # the index of the repaired archive is clean
    ix = ctx.jam_recover_index(t.data_ptr() + lead, len(fixed), jam.JAM_INDEX_CLI)
    assert ix.gaps == [] and ix.frames == len(kept) and ix.raw_len == len(raw)


@pytest.mark.parametrize("which", ["magic", "deep_flip"])
def test_the_stock_cli_decodes_a_repaired_archive(gpu, fx, which, tmp_path):
    if not os.path.exists(REF_CLI):
        pytest.skip(f"{os.path.relpath(REF_CLI, ROOT)} not built (reference tree was absent at build time)")
    fixed, kept = _repaired(gpu, fx, which)
    src, dst = tmp_path / "a.jam", tmp_path / "back.bin"
    fixed.tofile(src)
    cmd = [REF_CLI, "d", str(src), str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{' '.join(cmd)} -> {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    assert np.array_equal(np.fromfile(dst, dtype=np.uint8), np.concatenate(kept)), "the stock CLI decoded other bytes"


# ---- 10. argument checks on the device entries ---------------------------------------------------------------------------------------------
def test_device_argument_checks(gpu, fx):
    torch, jam, ctx = gpu
    F, P = fx
    lib = jam.lib()
    a = np.concatenate(F)
    t, lead = _place(torch, a)
    d_in = t.data_ptr() + lead
    h = C.c_void_p()
    assert lib.jpk_dev_jam_index_recover(None, d_in, len(a), 1, 1, C.byref(h), None) == E_ARG
    assert lib.jpk_dev_jam_index_recover(ctx._h, d_in, len(a), 1, 0, C.byref(h), None) == E_ARG and not h
    assert lib.jpk_dev_jam_index_recover(ctx._h, d_in, len(a), 1, 2, C.byref(h), None) == E_ARG
    assert lib.jpk_dev_jam_index_recover(ctx._h, None, len(a), 1, 1, C.byref(h), None) == E_ARG
    assert lib.jpk_dev_jam_index_recover(ctx._h, d_in, len(a), 1, 1, None, None) == E_ARG
    e = ctx.jam_recover_index(0, 0, jam.JAM_INDEX_CLI)
    assert (e.kind, e.frames, e.gaps) == (1, 0, [])
    ix = ctx.jam_recover_index(d_in, len(a), jam.JAM_INDEX_CLI)
    out = torch.full((len(a) + 64,), SENT, dtype=torch.uint8, device="cuda")
    n, k = C.c_int64(-7), C.c_int32(-7)
    rep = lambda ctx_h, ix_h, ln, cap: lib.jpk_dev_jam_repair(ctx_h, ix_h, d_in, ln, None, out.data_ptr() + 1, cap, C.byref(n), C.byref(k))
    assert rep(None, ix._h, len(a), len(a)) == E_ARG and rep(ctx._h, None, len(a), len(a)) == E_ARG
    assert rep(ctx._h, ix._h, len(a) - 1, len(a)) == E_ARG and rep(ctx._h, ix._h, len(a), -1) == E_ARG
    assert n.value == -7
    assert rep(ctx._h, ix._h, len(a), len(a) - 1) == E_CAPACITY and (n.value, k.value) == (len(a), len(F))
    assert (out.cpu().numpy() == SENT).all()
    with pytest.raises(jam.JampackError) as err:
        ctx.jam_repair(ix, d_in, len(a), out.data_ptr() + 1, 0)
    assert err.value.status == E_CAPACITY
    assert rep(ctx._h, ix._h, len(a), len(a)) == OK and (n.value, k.value) == (len(a), len(F))
    got = out.cpu().numpy()
    assert np.array_equal(got[1: 1 + len(a)], a) and got[0] == SENT and (got[1 + len(a):] == SENT).all()
    # an index without a kept frame: no bytes, no launch
    st = (C.c_int32 * len(F))(*([E_CORRUPT] * len(F)))
    out.fill_(SENT)
    assert lib.jpk_dev_jam_repair(ctx._h, ix._h, d_in, len(a), st, out.data_ptr() + 1, len(a), C.byref(n), C.byref(k)) == OK and (n.value, k.value) == (0, 0)
    assert (out.cpu().numpy() == SENT).all()
