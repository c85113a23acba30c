"""Updating .jam archives on the device (jpk_dev_jam_update, k_jam_splice) and through host buffers (jpk_jam_update).  The expected archive
is built from existing entries only: an untouched frame is its old bytes, a rewritten one jam_block_write / jam_staged_block_write /
jam_cli_block_write of the patched raw frame, the tail the matching jam_*compress.  Every case asserts byte equality of the whole output, 64
untouched sentinel bytes on both sides of it, the number of rewritten frames, the equality of the new index with the matching creator run
on the output, and that a whole decode of the output is the numpy-patched input.  Archives and sources sit at odd offsets; the output
starts 0, 1 and 15 bytes behind an aligned address.  Inputs are small text, BlockSize 1 MiB.  -m gpu"""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_jam_staged import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "jampack_ref")
MiB = 1 << 20
SENT = 0xA5
OK, E_ARG, E_CAPACITY, E_CORRUPT = 0, -1, -2, -3
PLAIN, CLI, STAGED = 0, 1, 2
EDGE_SIZES = [1, 119, 120, 121, 4096, 65535, 65536, 65537, 1, 300000, 16, 15]
CLI_SIZES = [6000, 6001, 4097, 5000, 2345]


def _full(ix):
    return [ix.frame(k) for k in range(ix.frames)], [ix.frame_kind(k) for k in range(ix.frames)], list(ix.gaps), ix.kind, ix.raw_len, ix.archive_len, ix.bad_frame


def _split(data, sizes):
    at = np.cumsum([0] + list(sizes))
    return [data[at[k]: at[k + 1]] for k in range(len(sizes))]


def _write(jam, kind, part, fl):
    """the single-frame writer of a frame kind"""
    if kind == PLAIN:
        return jam.jam_block_write(part, MiB)
    if kind == STAGED:
        return jam.jam_staged_block_write(part, MiB, flags=fl)
    return jam.jam_cli_block_write(part, MiB, dedupe=bool(fl & 1), filters=bool(fl & 4))


def _compress(jam, kind, t, bs, fl):
    if kind == PLAIN:
        return jam.jam_compress(t, bs)
    if kind == STAGED:
        return jam.jam_staged_compress(t, bs, flags=fl)
    return jam.jam_cli_compress(t, bs, dedupe=bool(fl & 1), filters=bool(fl & 4))


def _decode(jam, kind, a):
    if kind == PLAIN:
        return jam.jam_decompress(a)
    if kind == STAGED:
        return jam.jam_staged_decompress(a)
    return jam.jam_cli_decompress_all(a)


def _index(ctx, kind, ptr, n):
    return ctx.jam_index(ptr, n) if kind == PLAIN else ctx.jam_cli_index(ptr, n) if kind == CLI else ctx.jam_staged_index(ptr, n)


def _expected(jam, frames, parts, kinds, writes, fl=0, tail=None, tail_kind=PLAIN, bs=MiB):
    """(archive, rewritten frames, raw bytes) an update of the frames `frames` (raw parts `parts`) must give"""
    raw = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    patched = raw.copy()
    for off, src in writes:
        patched[off: off + len(src)] = src
    at = np.cumsum([0] + [len(p) for p in parts])
    out, rw = [], 0
    for k, f in enumerate(frames):
        a, b = int(at[k]), int(at[k + 1])
        if b > a and any(len(s) > 0 and o < b and o + len(s) > a for o, s in writes):
            out.append(_write(jam, kinds[k], patched[a:b], fl))
            rw += 1
        else:
            out.append(f)
    if tail is not None and len(tail):
        out.append(_compress(jam, tail_kind, tail, bs, fl))
        patched = np.concatenate([patched, tail])
    return (np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)), rw, patched


def _dev(torch, b, lead):
    """b `lead` bytes behind an aligned device address, sentinels around it -> (tensor, pointer)"""
    img = np.full(lead + len(b) + 64, SENT, dtype=np.uint8)
    img[lead: lead + len(b)] = b
    t = torch.from_numpy(img).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + lead


def _update(gpu, a, kind, writes, fl=0, tail=None, bs=MiB, out_lead=0, ix=None, cap=None):
    """jpk_dev_jam_update of the archive a (index kind `kind`, or the index ix) -> (status, output, new index, rewritten, bad frame); the
    sentinels around the output are checked here"""
    torch, jam, ctx = gpu
    t_in, d_in = _dev(torch, a, 3)
    before = t_in.cpu().numpy().copy()
    ix = ix if ix is not None else _index(ctx, kind, d_in, len(a))
    keep, dw = [], []
    for i, (off, src) in enumerate(writes):
        t, p = _dev(torch, np.asarray(src, dtype=np.uint8), i % 17)
        keep.append(t)
        dw.append((off, len(src), p))
    t_tail, d_tail = _dev(torch, tail if tail is not None else np.zeros(0, dtype=np.uint8), 5)
    tail_len = len(tail) if tail is not None else 0
    if cap is None:
        cap = jam.jam_update_bound(ix, [(o, n) for o, n, _ in dw], tail_len, bs)
    out = torch.full((64 + out_lead + cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    n, nix, rw, bad, rc = ctx.jam_update(ix, d_in, len(a), dw, out.data_ptr() + 64 + out_lead, cap, d_tail if tail_len else None, tail_len, bs, flags=fl, check=False)
    got = out.cpu().numpy()
    assert np.array_equal(t_in.cpu().numpy(), before)
    lo = 64 + out_lead
    if rc == OK:
        assert (got[:lo] == SENT).all() and (got[lo + n: lo + n + 64] == SENT).all() and n <= cap
    return rc, got[lo: lo + max(n, 0)] if rc == OK else None, nix, rw, bad


def _check(gpu, kind, frames, parts, kinds, writes, fl=0, tail=None, bs=MiB, out_lead=0, host=False):
    """one update against its expectation, on the device and (host) through host buffers"""
    torch, jam, ctx = gpu
    a = np.concatenate(frames) if frames else np.zeros(0, dtype=np.uint8)
    want, want_rw, raw = _expected(jam, frames, parts, kinds, writes, fl, tail, kind, bs)
    rc, got, nix, rw, bad = _update(gpu, a, kind, writes, fl, tail, bs, out_lead)
    assert (rc, rw, bad) == (OK, want_rw, -1)
    assert len(got) == len(want) and np.array_equal(got, want)
    t, p = _dev(torch, got, 7)
    assert _full(nix) == _full(_index(ctx, kind, p, len(got))) and nix.kind == kind and nix.gaps == [] and nix.bad_frame == -1
    assert np.array_equal(_decode(jam, kind, got), raw)
    if host:
        hix = jam.jam_index(a) if kind == PLAIN else jam.jam_cli_index(a) if kind == CLI else jam.jam_staged_index(a)
        h_got, h_nix = jam.jam_update(a, writes, hix, tail=tail, block_size=bs, flags=fl)
        assert np.array_equal(h_got, got) and _full(h_nix) == _full(nix)
    return got, nix


# ---- plain frames, edge sizes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge(gpu):
    _, jam, _ = gpu
    parts = _split(jam.corpus.make("text", sum(EDGE_SIZES), 31), EDGE_SIZES)
    return [jam.jam_block_write(p, MiB) for p in parts], parts


def _edge_sets():
    """writes at every frame edge, offsets -17, -16, -1, 0, +1, lengths 0, 1, 15, 16, 17, 33, 4097 and to the end of the frame the write
    starts in, dealt into sets of pairwise disjoint writes (a write of 0 bytes goes anywhere), each set in shuffled order"""
    at = [int(x) for x in np.cumsum([0] + EDGE_SIZES)]
    raw_len = at[-1]
    rng = np.random.default_rng(5)
    cand = []
    for e in at:
        for d in (-17, -16, -1, 0, 1):
            o = e + d
            if o < 0 or o > raw_len:
                continue
            end = min(x for x in at if x > o) if o < raw_len else raw_len
            for ln in (0, 1, 15, 16, 17, 33, 4097, end - o):
                if o + ln <= raw_len and (o, ln) not in cand:
                    cand.append((o, ln))
    cand = [cand[i] for i in rng.permutation(len(cand))]
    sets = []
    for o, ln in cand:
        for s in sets:
            if ln == 0 or all(m == 0 or o + ln <= p or p + m <= o for p, m in s):
                s.append((o, ln))
                break
        else:
            sets.append([(o, ln)])
    return sets


EDGE_SETS = _edge_sets()


def test_edge_sets_cover_what_they_should():
    flat = [w for s in EDGE_SETS for w in s]
    assert len(flat) > 300
    assert {ln for _, ln in flat} >= {0, 1, 15, 16, 17, 33, 4097}
    for s in EDGE_SETS:
        live = sorted(w for w in s if w[1])
        assert all(a[0] + a[1] <= b[0] for a, b in zip(live, live[1:]))


@pytest.mark.parametrize("third", [0, 1, 2])
def test_plain_frames_at_every_edge(gpu, edge, third):
    torch, jam, ctx = gpu
    frames, parts = edge
    rng = np.random.default_rng(17 + third)
    for i, s in enumerate(EDGE_SETS):
        if i % 3 != third:
            continue
        writes = [(o, rng.integers(0, 256, ln, dtype=np.uint8)) for o, ln in s]
        _check(gpu, PLAIN, frames, parts, [PLAIN] * len(frames), writes, out_lead=(0, 1, 15)[(i // 3) % 3], host=(i == third))


# ---- a changed size moves every later frame --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five(gpu):
    """five plain frames of CLI_SIZES raw bytes"""
    _, jam, _ = gpu
    parts = _split(jam.corpus.make("text", sum(CLI_SIZES), 33), CLI_SIZES)
    return [jam.jam_block_write(p, MiB) for p in parts], parts


def test_a_changed_size_moves_the_later_frames(gpu, five):
    frames, parts = five
    rng = np.random.default_rng(3)
    moved = set()
    for ln in (6001, 3000):
        got, nix = _check(gpu, PLAIN, frames, parts, [PLAIN] * 5, [(6000, rng.integers(0, 256, ln, dtype=np.uint8))], out_lead=1)
        old = np.cumsum([0] + [len(f) for f in frames])
        assert nix.frame(1)[3] != len(frames[1]) - 15
        moved |= {(nix.frame(k)[2] - 15 - int(old[k])) % 16 for k in (2, 3, 4)}
    assert moved - {0}                                                 # the kept frames behind it landed at another alignment


def test_every_frame_wholly_covered_decodes_nothing(gpu, five):
    """the same call on an archive whose frames all have broken crcs: a decode would have failed them"""
    torch, jam, ctx = gpu
    frames, parts = five
    rng = np.random.default_rng(4)
    at = np.cumsum([0] + CLI_SIZES)
    # one write over frames 0-1, frame 2 tiled by three, frames 3-4 by one that ends at raw_len; shuffled
    writes = [(int(at[3]), rng.integers(0, 256, CLI_SIZES[3] + CLI_SIZES[4], dtype=np.uint8)), (int(at[2]) + 1000, rng.integers(0, 256, 97, dtype=np.uint8)),
              (0, rng.integers(0, 256, int(at[2]), dtype=np.uint8)), (int(at[2]), rng.integers(0, 256, 1000, dtype=np.uint8)),
              (int(at[2]) + 1097, rng.integers(0, 256, 3000, dtype=np.uint8))]
    got, nix = _check(gpu, PLAIN, frames, parts, [PLAIN] * 5, writes, out_lead=15)
    broken = [f.copy() for f in frames]
    for f in broken:
        f[3] ^= 0x40
    rc, got2, nix2, rw, bad = _update(gpu, np.concatenate(broken), PLAIN, writes, out_lead=15)
    assert (rc, rw, bad) == (OK, 5, -1) and np.array_equal(got2, got) and _full(nix2) == _full(nix)


def test_no_frame_touched(gpu, five):
    frames, parts = five
    e = np.zeros(0, dtype=np.uint8)
    got, nix = _check(gpu, PLAIN, frames, parts, [PLAIN] * 5, [(0, e), (6000, e), (sum(CLI_SIZES), e)], out_lead=1, host=True)
    assert np.array_equal(got, np.concatenate(frames))
    got, nix = _check(gpu, PLAIN, frames, parts, [PLAIN] * 5, [], out_lead=15)
    assert np.array_equal(got, np.concatenate(frames))


# ---- pass edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(gpu):
    """300 plain frames of 2 000 raw bytes"""
    _, jam, _ = gpu
    parts = _split(jam.corpus.make("text", 300 * 2000, 35), [2000] * 300)
    return [jam.jam_block_write(p, MiB) for p in parts], parts


def test_129_rewritten_frames_of_130(gpu, many):
    frames, parts = many[0][:130], many[1][:130]
    rng = np.random.default_rng(6)
    writes = [(2000 * k + int(rng.integers(0, 1990)), rng.integers(0, 256, 7, dtype=np.uint8)) for k in range(130) if k != 77]
    writes = [writes[i] for i in rng.permutation(len(writes))]
    _check(gpu, PLAIN, frames, parts, [PLAIN] * 130, writes, out_lead=1)


def test_a_kept_run_longer_than_a_pass(gpu, many):
    frames, parts = many
    s = np.arange(40, dtype=np.uint8)
    got, nix = _check(gpu, PLAIN, frames, parts, [PLAIN] * 300, [(299 * 2000 + 1960, s), (0, s)], out_lead=15)
    assert nix.frames == 300


# ---- kind 2: plain and staged frames -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(gpu):
    """plain and staged frames in turn, the staged ones written with flags 0, 1, 4, 5; frame 3 is a dedupe frame of 300-byte repeats"""
    _, jam, _ = gpu
    sizes = [5000, 6000, 1, 6000, 4097, 3000, 2345, 5000]
    parts = _split(jam.corpus.make("text", sum(sizes), 37), sizes)
    tile = np.random.default_rng(8).integers(0, 256, 300, dtype=np.uint8)
    parts[3] = np.tile(tile, 20)
    kinds = [PLAIN, STAGED, PLAIN, STAGED, STAGED, PLAIN, STAGED, STAGED]
    fls = [0, 0, 0, 1, 4, 0, 5, 1]
    return [_write(jam, k, p, f) for k, p, f in zip(kinds, parts, fls)], parts, kinds


@pytest.mark.parametrize("fl", [0, 1, 4, 5])
def test_kind_2_keeps_the_kind_of_every_frame(gpu, mixed, fl):
    torch, jam, ctx = gpu
    frames, parts, kinds = mixed
    at = [int(x) for x in np.cumsum([0] + [len(p) for p in parts])]
    rng = np.random.default_rng(9 + fl)
    rep = np.tile(rng.integers(0, 256, 256, dtype=np.uint8), 12)
    # a plain frame partly, the dedupe frame partly with repeats, a staged frame wholly, the edge of a staged and a plain frame
    writes = [(at[5] - 10, rng.integers(0, 256, 20, dtype=np.uint8)), (at[3] + 100, rep), (at[6], rng.integers(0, 256, 2345, dtype=np.uint8)), (17, rng.integers(0, 256, 33, dtype=np.uint8))]
    got, nix = _check(gpu, STAGED, frames, parts, kinds, writes, fl=fl, out_lead=1, host=True)
    assert [nix.frame_kind(k) for k in range(nix.frames)] == kinds                       # plain frames stay plain, staged ones staged
    for k in range(nix.frames):                                                          # BlockSize and the staged bit as before
        po = nix.frame(k)[2]
        assert int(np.frombuffer(got[po - 4: po].tobytes(), dtype="<i4")[0]) == (MiB | (1 << 30) if kinds[k] == STAGED else MiB)


# ---- kind 1: frames of the stock CLI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(gpu):
    _, jam, _ = gpu
    parts = _split(jam.corpus.make("text", sum(CLI_SIZES), 91), CLI_SIZES)
    return [jam.jam_cli_block_write(p, MiB) for p in parts], parts


def _cli_writes(seed):
    rng = np.random.default_rng(seed)
    return [(12001 + 4097 - 5, rng.integers(0, 256, 30, dtype=np.uint8)), (6000, rng.integers(0, 256, 6001, dtype=np.uint8)), (3, rng.integers(0, 256, 1, dtype=np.uint8))]


@pytest.mark.parametrize("fl", [0, 5])
def test_kind_1(gpu, cli, fl):
    frames, parts = cli
    got, nix = _check(gpu, CLI, frames, parts, [CLI] * 5, _cli_writes(11 + fl), fl=fl, out_lead=15, host=True)
    assert nix.kind == 1 and [nix.frame(k)[1] for k in range(5)] == CLI_SIZES


@pytest.mark.parametrize("fl", [0, 5])
def test_the_stock_cli_decodes_an_updated_archive(gpu, cli, fl, tmp_path):
    if not os.path.exists(REF_CLI):
        pytest.skip(f"{os.path.relpath(REF_CLI, ROOT)} not built (reference tree was absent at build time)")
    torch, jam, ctx = gpu
    frames, parts = cli
    writes = _cli_writes(11 + fl)
    tail = jam.corpus.make("text", 7000, 92)
    rc, got, nix, rw, bad = _update(gpu, np.concatenate(frames), CLI, writes, fl=fl, tail=tail)
    assert (rc, rw) == (OK, 4)
    src, dst = tmp_path / "a.jam", tmp_path / "back.bin"
    got.tofile(src)
    cmd = [REF_CLI, "d", str(src), str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{' '.join(cmd)} -> {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    assert np.array_equal(np.fromfile(dst, dtype=np.uint8), _expected(jam, frames, parts, [CLI] * 5, writes, fl, tail, CLI)[2]), "the stock CLI decoded other bytes"


# ---- damaged frames ------------------------------------------------------------------------------------------------------------------------------
def test_a_damaged_frame_is_replaced_whole_and_refused_in_part(gpu, five):
    torch, jam, ctx = gpu
    frames, parts = five
    bad_frames = [f.copy() for f in frames]
    bad_frames[2][3] ^= 1                                               # its crc: a plain index keeps the frame
    a = np.concatenate(bad_frames)
    rng = np.random.default_rng(12)
    new = rng.integers(0, 256, CLI_SIZES[2], dtype=np.uint8)
    # wholly covered (by two writes, with a neighbour partly covered): replaced, and the result decodes cleanly
    writes = [(12001 + 2000, new[2000:]), (12001 - 9, np.concatenate([rng.integers(0, 256, 9, dtype=np.uint8), new[:2000]]))]
    want, want_rw, raw = _expected(jam, frames, parts, [PLAIN] * 5, writes)
    rc, got, nix, rw, bad = _update(gpu, a, PLAIN, writes, out_lead=1)
    assert (rc, rw, bad) == (OK, 2, -1) and np.array_equal(got, want) and np.array_equal(jam.jam_decompress(got), raw)
    # partly covered, behind a sound frame that is partly covered too: the lowest failing frame, no index
    for writes in ([(12001 - 9, new[:2009])], [(12001 + 1, new[1:])], [(100, new[:5]), (12001 + 4096, new[:1]), (12001 + 4097 + 5, new[:1])]):
        rc, got, nix, rw, bad = _update(gpu, a, PLAIN, writes)
        assert (rc, bad, nix) == (E_CORRUPT, 2, None), writes
    # the host form answers the same
    with pytest.raises(jam.JampackError) as err:
        jam.jam_update(a, [(12001 + 1, new[1:])])
    assert err.value.status == E_CORRUPT and "frame 2" in str(err.value)


def test_a_recovered_index_with_two_gaps(gpu, five):
    torch, jam, ctx = gpu
    frames, parts = five
    segs = [f.copy() for f in frames]
    segs[1][0] ^= 1                                                     # two lost headers: the index keeps frames 0, 2, 4
    segs[3][0] ^= 1
    a = np.concatenate(segs)
    t_in, d_in = _dev(torch, a, 3)
    ix = ctx.jam_recover_index(d_in, len(a))
    assert ix.frames == 3 and len(ix.gaps) == 2
    kept, kparts = [frames[0], frames[2], frames[4]], [parts[0], parts[2], parts[4]]
    s = np.arange(50, dtype=np.uint8)
    writes = [(6000 + 4097 - 25, s), (5, s[:3])]                       # raw coordinates of the index: frames 1-2 of it, and frame 0
    want, want_rw, raw = _expected(jam, kept, kparts, [PLAIN] * 3, writes)
    rc, got, nix, rw, bad = _update(gpu, a, PLAIN, writes, ix=ix, out_lead=15)
    assert (rc, rw, bad) == (OK, 3, -1) and np.array_equal(got, want)
    fixed = jam.jam_repair(a, ix)
    rix = jam.jam_index(fixed)
    assert nix.gaps == [] and nix.frames == rix.frames == 3                             # the gaps are gone; frames and raw offsets as in repair
    assert [nix.frame(k)[:2] for k in range(3)] == [rix.frame(k)[:2] for k in range(3)]
    assert _full(nix) == _full(jam.jam_index(got)) and np.array_equal(jam.jam_decompress(got), raw)
    h_got, h_nix = jam.jam_update(a, writes, ix)
    assert np.array_equal(h_got, got) and _full(h_nix) == _full(nix)


# ---- the tail --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_text(gpu):
    _, jam, _ = gpu
    return jam.corpus.make("text", 5 * MiB // 2, 39)


@pytest.mark.parametrize("tail_len", [0, 1, MiB - 1, MiB, 5 * MiB // 2])
def test_tail(gpu, five, tail_text, tail_len):
    frames, parts = five
    s = np.arange(9, dtype=np.uint8)
    got, nix = _check(gpu, PLAIN, frames, parts, [PLAIN] * 5, [(sum(CLI_SIZES) - 9, s)], tail=tail_text[:tail_len], out_lead=1, host=tail_len in (0, 1))
    assert nix.frames == 5 + (tail_len + MiB - 1) // MiB


@pytest.mark.parametrize("kind", [PLAIN, CLI, STAGED])
def test_an_empty_index_with_a_tail_is_a_writer(gpu, tail_text, kind):
    torch, jam, ctx = gpu
    tail = tail_text[: MiB + 4097]
    got, nix = _check(gpu, kind, [], [], [], [], fl=5 if kind != PLAIN else 0, tail=tail, out_lead=15, host=(kind == STAGED))
    assert nix.frames == 2 and nix.raw_len == len(tail)
    got, nix = _check(gpu, kind, [], [], [], [])                        # and without one: nothing
    assert len(got) == 0 and nix.frames == 0


def test_kind_2_tail_is_staged_frames(gpu, mixed):
    torch, jam, ctx = gpu
    frames, parts, kinds = mixed
    tail = jam.corpus.make("text", 9000, 41)
    got, nix = _check(gpu, STAGED, frames, parts, kinds, [(1, np.arange(5, dtype=np.uint8))], fl=1, tail=tail, out_lead=1)
    assert nix.frame_kind(nix.frames - 1) == STAGED and nix.frames == len(frames) + 1


# ---- capacity --------------------------------------------------------------------------------------------------------------------------------------
def test_a_capacity_between_the_least_and_the_need_reports_the_bound(gpu, five):
    torch, jam, ctx = gpu
    frames, parts = five
    a = np.concatenate(frames)
    writes = [(6000, np.random.default_rng(13).integers(0, 256, 6001, dtype=np.uint8))]          # random bytes: the new frame is larger than the old one
    want, _, _ = _expected(jam, frames, parts, [PLAIN] * 5, writes)
    assert len(want) > len(a)
    t_in, d_in = _dev(torch, a, 3)
    ix = ctx.jam_index(d_in, len(a))
    bound = jam.jam_update_bound(ix, [(6000, 6001)])
    rc, got, nix, rw, bad = _update(gpu, a, PLAIN, writes, cap=len(want) - 1)
    assert (rc, nix) == (E_CAPACITY, None)
    tw, pw = _dev(torch, writes[0][1], 2)
    out = torch.full((len(want) + 128,), SENT, dtype=torch.uint8, device="cuda")
    n, nix, rw, bad, rc = ctx.jam_update(ix, d_in, len(a), [(6000, 6001, pw)], out.data_ptr() + 64, len(want) - 1, check=False)
    assert (rc, n, nix) == (E_CAPACITY, bound, None)
    img = out.cpu().numpy()
    assert (img[:64] == SENT).all() and (img[64 + len(want) - 1:] == SENT).all()                  # nothing outside the capacity it was given
    n, nix, rw = ctx.jam_update(ix, d_in, len(a), [(6000, 6001, pw)], out.data_ptr() + 64, len(want))       # exactly enough
    assert n == len(want) and np.array_equal(out.cpu().numpy()[64: 64 + n], want)
