"""rank_window_model on the CPU: the window scheme of k_enc_mtf (ans_enc_front.hip) -- by its definition (one stable sort of a tile's heads
by symbol) and the way the kernel computes it (64-byte groups) -- gives the ranks and frequencies of a plain one-list MTF on every
crafted input of test_gpu_rank_window.py and on a few hundred random short texts over alphabets of 1, 2, 3, 64, 65, 255 and 256 values;
nothing is written outside the chunk's n bytes.  The inputs are shown to reach what they are named for: windows of exactly 1 and of 255
heads, windows across tile edges, a tile of 4096 heads, first heads ranked from the stamps."""
import functools

import numpy as np
import pytest

import rank_window_model as M

N_RANDOM = 210


@functools.lru_cache(maxsize=None)
def _plain(name):
    return M.plain_rank_encode(M.case(name))


def _check(t, want, how, what):
    r, f = M.rank_window(t, how)
    n = len(t)
    assert np.array_equal(f, want[1]), what
    bad = np.flatnonzero(r[:n] != want[0])
    assert len(bad) == 0, f"{what}: {len(bad)} ranks differ, first at {bad[0]}: {r[bad[0]]} != {want[0][bad[0]]}"
    assert (r[n:] == M.STALE_RANK).all(), f"{what}: wrote outside the chunk"


@pytest.mark.parametrize("how", ["sort", "groups"])
@pytest.mark.parametrize("name", M.CASES)
def test_crafted(name, how):
    _check(M.case(name), _plain(name), how, f"{name} ({how})")


def test_two_chunks():
    """1 MiB + 4097 bytes: each chunk on its own (the stamps restart), by the definition"""
    t = M.case(M.TWO_CHUNKS)
    assert len(t) == M.F.CHUNK + M.ATILE + 1
    for i, ch in enumerate(M.F.chunks(t)):
        _check(ch, M.plain_rank_encode(ch), "sort", f"two-chunks, chunk {i}")
    tail = M.F.chunks(t)[1]
    _check(tail, M.plain_rank_encode(tail), "groups", "two-chunks, chunk 1 (groups)")


@pytest.mark.parametrize("part", range(7))
def test_random_short(part):
    for i in range(part, N_RANDOM, 7):                                         # one alphabet per part
        t = M.random_short(i)
        want = M.plain_rank_encode(t)
        for how in ("sort", "groups"):
            _check(t, want, how, f"random short text {i} ({len(t)} B, alphabet {M.ALPHABETS[i % 7]}, {how})")


def _tiles(t):
    return [t[a: a + M.ATILE] for a in range(0, len(t), M.ATILE)]


def test_inputs_reach_what_they_are_named_for():
    nostamp = np.full(256, -1)
    # every byte a head, every window 1
    hp, hs, run, rank, before, win = M.tile_by_sort(_tiles(M.case("alternating"))[0], nostamp)
    assert len(hp) == M.ATILE and (win == 1).all() and (rank[2:] == 1).all()
    # every rank 255, every window 255: four steps of 64 behind the RW_CAP positions of the own lane
    t = M.case("cycle-256")
    assert len(t) == 5 * M.ATILE
    hp, hs, run, rank, before, win = M.tile_by_sort(_tiles(t)[1], nostamp)
    assert (win == 255).all() and len(win) == M.ATILE - 256
    log = []
    M.rank_window(t, "groups", log)
    assert set(log) == {(M.RW_CAP, 4)}
    r, f = _plain("cycle-256")
    assert sorted(r.tolist())[256:] == [255] * (len(t) - 256)
    # a tile of 4096 heads and no repeats
    hp, hs, run, rank, before, win = M.tile_by_sort(_tiles(M.case("lds-worst"))[0], nostamp)
    assert len(hp) == M.ATILE and (run == 1).all()
    # a symbol seen once in tile 0 and again at the last byte of tile 3: a first head of tile 3, ranked from the stamps
    t = M.case("window-three-tiles")
    assert np.flatnonzero(t == 200).tolist() == [1000, 4 * M.ATILE - 1]
    # tile 2 of carried-ties opens with 256 first heads
    t = M.case("carried-ties")
    tilebase, prevlast, freq, bstart = M.F.prep(*M.F.hist(t))
    hp, hs, run = M.heads(_tiles(t)[2])
    P, N, before = M.sort_by_symbol(hs, run)
    assert (P[:256] < 0).all() and (prevlast[2] >= 0).all()
    assert len(set(M.carried(hs, P, prevlast[2])[:256].tolist())) > 50          # the stamps decide, not the counter alone
    # a tile's first byte continues a run (rank 0 from the stamps), at the edge 3|4
    t = M.case("runs-at-edges")
    assert t[4 * M.ATILE] == t[4 * M.ATILE - 1]
    # the lengths: a chunk of one byte, partial last groups of 1 and 63, a tile of one byte
    assert [len(M.case(f"len-{n}")) for n in M.LENGTHS] == list(M.LENGTHS)


def test_window_lengths_of_a_bwt_image():
    """what the lane assignment rests on: most windows of a BWT image end within RW_CAP heads"""
    win = []
    M.rank_window(M.case("bwt-text"), "sort", win)
    win = np.concatenate(win)
    assert np.median(win) <= M.RW_CAP
