"""The crafted texts of r0_tile_model put heads, singletons and short suffixes on every edge round 0's finish (bwt_fwd_r0.hip) cuts its sorted
list at, and runs on every edge the run-length kernels cut the text at (CPU only).

The kinds are conditions on the INPUTS of test_gpu_r0_finish.py, not measurements of the code under test.  The model is held against brute
force (Python's own sort of the suffixes) and against the oracle's suffix array; the "rule dropped" twins show that the text crafted for a
kind tells a kernel that forgot the rule from one that kept it -- by the survivor count, the ranks or the run lengths, which is what the GPU
test compares.  If a seed misses a kind, another seed is chosen -- the assertions stay."""
import numpy as np
import pytest

import r0_tile_model as M


def _brute(t):
    """suffixes in Python's own order of their bytes, grouped by 7-byte prefix; a suffix shorter than 7 bytes is a group of its own.
    Returns (sa, rank per suffix = first slot of its group, survivors, run members) -- the last two as sets of suffixes"""
    n = len(t)
    b = bytes(t)
    sa = sorted(range(n), key=lambda s: b[s:])
    rank, surv, runs = [0] * n, set(), set()
    j = 0
    while j < n:
        e = j + 1
        if sa[j] + M.DEPTH <= n:
            pre = b[sa[j]: sa[j] + M.DEPTH]
            while e < n and sa[e] + M.DEPTH <= n and b[sa[e]: sa[e] + M.DEPTH] == pre:
                e += 1
        for k in range(j, e):
            rank[sa[k]] = j
        if e - j > 1:
            surv.update(sa[j:e])
            if len(set(b[sa[j]: sa[j] + M.DEPTH])) == 1:
                runs.update(sa[j:e])
        j = e
    return sa, rank, surv, runs


def _small_texts():
    rng = np.random.default_rng(99)
    for values in ((7,), (0,), (0, 1), (5, 9), (0, 1, 2), (1, 2, 3), tuple(range(256))):
        for n in (1, 2, 6, 7, 8, 13, 14, 63, 64, 65, 150, 300):
            yield rng.choice(np.array(values, dtype=np.uint8), n)
    for n in (40, 200, 300):                    # texts that end inside a run, of zeros and of another byte
        for byte in (0, 3):
            t = rng.choice(np.array((0, 1, 2, 3), dtype=np.uint8), n)
            t[n - 11:] = byte
            yield t


def test_the_model_against_brute_force():
    """heads, ranks, survivors and run members of small texts over 1, 2, 3 and 256 values, zeros and closing runs included"""
    count = 0
    for t in _small_texts():
        f = M.finish(t)
        sa, rank, surv, runs = _brute(t)
        n = len(t)
        assert sorted(f.sa.tolist()) == list(range(n))
        model_rank = np.empty(n, dtype=np.int64)
        model_rank[f.sa] = f.rank
        assert model_rank.tolist() == rank, t.tolist()
        assert f.starts.tolist() == sorted(set(rank)), t.tolist()                       # the heads
        assert set(f.sa[f.survivor].tolist()) == surv and f.survivors == len(surv) == M.survivors(t), t.tolist()
        assert set(f.sa[f.run].tolist()) == runs, t.tolist()
        single = ~f.survivor
        assert f.sa[single].tolist() == [sa[k] for k in np.flatnonzero(single)]          # a singleton's slot is final
        assert M.ends_after_round_0(t) == (not surv)
        rl = [next(k for k in range(i, n + 1) if k == n or t[k] != t[i]) - i for i in range(n)]
        assert M.run_lengths(t).tolist() == rl
        count += 1
    assert count == 7 * 12 + 6


def test_lists_made_by_hand():
    """the definitions on texts small enough to check by eye"""
    f = M.finish(np.array([5, 5, 5, 5, 5, 5, 5, 5, 5], dtype=np.uint8))                 # 5^9: six short suffixes, then 5^7 at positions 2, 1, 0
    assert f.sa.tolist() == [8, 7, 6, 5, 4, 3, 2, 1, 0] and f.head.tolist() == [True] * 7 + [False] * 2
    assert f.survivor.tolist() == [False] * 6 + [True] * 3 and f.run.tolist() == f.survivor.tolist() and f.rank.tolist() == [0, 1, 2, 3, 4, 5, 6, 6, 6]
    f = M.finish(np.array([9, 0, 0, 0, 0, 0, 0, 1, 9], dtype=np.uint8))                 # the short "9" ties with "9000000" on padding only
    assert f.sa[-2:].tolist() == [8, 0] and f.head[-2:].tolist() == [True, True] and f.survivors == 0
    assert M.finish(np.array([9, 0, 0, 0, 0, 0, 0, 1, 9], dtype=np.uint8), drop="short-shift").survivors == 2
    assert M.run_lengths(np.array([4, 4, 4, 7, 7, 4], dtype=np.uint8)).tolist() == [3, 2, 1, 2, 1, 1]
    assert M.large_members(M.period_2(1028)) == 2 * 1025 and M.large_members(M.period_2(1027)) == 0 and M.survivors(M.period_2(1027)) == 2 * 1024


def test_every_kind_is_shown_by_a_crafted_text():
    """the table of text x kind counts; every name of KINDS and RUN_KINDS at least once, the placed ones where they were placed"""
    total = {}
    for name in M.TEXTS:
        t, f = M.crafted(name), M.crafted_finish(name)
        c, r = M.kind_counts(t, f), M.run_kind_counts(t, f)
        assert set(c) <= set(M.KINDS) and set(r) <= set(M.RUN_KINDS)
        print(f"{name}: {len(t)} bytes, {f.survivors} survivors, {M.large_members(t)} in groups above 1024; {dict(c)}; {dict(r)}")
        assert len(t) <= 1_200_000 and (len(t) <= 1 << 20 or name == "tiles-257")
        for k, v in (c + r).items():
            total[k] = total.get(k, 0) + v
    for kind in M.KINDS + M.RUN_KINDS:
        assert total.get(kind, 0) > 0, kind
    for name, kind in (("n-50", "n-below-one-row"), ("abc-4095", "n-one-short-of-a-tile"), ("zab-4097", "n-one-past-a-tile"),
                       ("rand256-8192", "n-multiple-of-4096"), ("rand256-8192", "no-survivors"), ("short-row", "short-on-row-last-lane"),
                       ("short-wave", "short-on-wave-last-slot"), ("short-tile", "short-on-tile-last-slot"), ("short-tile-first", "short-on-tile-first-slot"),
                       ("zeros-tail", "short-between-two-equal-keys"), ("pair-row", "pair-straddles-row-edge"), ("pair-wave", "pair-straddles-wave-edge"),
                       ("pair-tile", "pair-straddles-tile-edge"), ("group-row", "group-straddles-row-edge"), ("group-wave", "group-straddles-wave-edge"),
                       ("group-tile", "group-straddles-tile-edge"), ("survivors-4096", "survivors-multiple-of-4096"), ("long-run", "tile-without-head"),
                       ("long-run", "head-65-or-more-tiles-in-front"), ("short-tile", "last-slot-survives")):
        assert M.kind_counts(M.crafted(name), M.crafted_finish(name))[kind] > 0, (name, kind)
    for name, kind in (("runs-3tiles", "run-crosses-tile-edge"), ("runs-3tiles", "run-ends-on-tile-last-byte"), ("runs-3tiles", "run-ends-text"),
                       ("runs-3tiles", "thread-segment-without-boundary"), ("long-run", "tiles-without-boundary-in-a-row"),
                       ("tiles-257", "more-than-256-tiles"), ("tiles-257", "tiles-without-boundary-in-a-row")):
        assert M.run_kind_counts(M.crafted(name), M.crafted_finish(name))[kind] > 0, (name, kind)


def test_the_placed_slots():
    """a placed short suffix ties with the slots behind it on padding only; a placed pair lies across its edge"""
    for name, slot in (("short-row", M.ROW - 1), ("short-wave", M.WAVE - 1), ("short-tile", M.CT - 1), ("short-tile-first", M.CT)):
        f = M.crafted_finish(name)
        assert f.sa[slot] == f.n - 1 and f.short[slot] and not f.short[slot + 1]
        assert f.key[slot] == f.key[slot + 1] == f.key[slot + 2] and f.rank[slot: slot + 3].tolist() == [slot, slot + 1, slot + 1]
    for name, slot in (("pair-row", M.ROW - 1), ("pair-wave", M.WAVE - 1), ("pair-tile", M.CT - 1)):
        f = M.crafted_finish(name)
        assert f.head[slot: slot + 3].tolist() == [True, False, True] and f.survivors == 2
    f = M.crafted_finish("long-run")
    assert f.head[1000] and f.sizes[np.searchsorted(f.starts, 1000)] == 67 * M.CT - 6 and f.run.sum() == 67 * M.CT - 6


def test_a_dropped_rule_shows_on_the_text_crafted_for_it():
    """every twin differs from the rule in the survivor count or the ranks (what the GPU test compares through sa_round_active[1] and the suffix
    array) on the text of its kind, and is the rule itself on a text without that kind"""
    assert set(M.DROPS) == {"row-short-carry", "row-key-handoff", "wave-load", "wave-short-carry", "tile-short-carry", "short-shift", "he64-as-1",
                            "he64-as-0", "carry-nearest-tile", "carry-one-batch", "lhl-word-only"}
    for drop, (kind, name) in M.DROPS.items():
        t, f = M.crafted(name), M.crafted_finish(name)
        assert M.kind_counts(t, f)[kind] > 0, (drop, kind, name)
        g = M.finish(t, drop=drop)
        count, ranks = g.survivors != f.survivors, int((g.rank != f.rank).sum())
        print(f"{drop} on {name} ({kind}): survivors {f.survivors} -> {g.survivors}, {ranks} ranks differ")
        assert count or ranks, drop
        plain = M.crafted("n-50")                                      # one row: no edge of any kind
        h = M.finish(plain, drop=drop)
        assert h.survivors == M.survivors(plain) and np.array_equal(h.rank, M.finish(plain).rank), drop
    for drop, (kind, name) in M.RUN_DROPS.items():
        t = M.crafted(name)
        assert M.run_kind_counts(t, M.crafted_finish(name))[kind] > 0, (drop, kind, name)
        wrong = int((M.run_lengths(t, drop=drop) != M.run_lengths(t)).sum())
        print(f"{drop} on {name} ({kind}): {wrong} run lengths differ")
        assert wrong, drop
        plain = M.crafted("short-row")                                 # one tile, no run of sixteen
        assert np.array_equal(M.run_lengths(plain, drop=drop), M.run_lengths(plain)), drop


@pytest.mark.parametrize("name", M.TEXTS)
def test_the_model_agrees_with_the_suffix_array(oracle, name):
    """what round 0 finishes is final: a singleton's slot holds its suffix in the oracle's suffix array, and every survivor's final slot lies
    inside its group"""
    t, f = M.crafted(name), M.crafted_finish(name)
    sa = oracle.suffix_array(np.array(t)).astype(np.int64)
    single = ~f.survivor
    assert np.array_equal(sa[single], f.sa[single])
    final = np.empty(f.n, dtype=np.int64)
    final[sa] = np.arange(f.n)
    where = final[f.sa]                                                 # the final slot of the suffix on slot j of round 0's list
    size = np.repeat(f.sizes, f.sizes)
    assert ((where >= f.rank) & (where < f.rank + size)).all()
