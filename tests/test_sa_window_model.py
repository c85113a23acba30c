"""The crafted texts of sa_window_model reach every route the doubling rounds of the suffix sort take at the edges of their 1024-slot
windows (CPU only).

The geometry kinds are conditions on the INPUTS of test_gpu_sa_windows.py, not measurements of the code under test: a text that
misses a kind would let a comparison of win_geometry / k_win_pieces / k_seg_round / k_lg_* go unexercised there.  If a seed misses a
kind, another seed is chosen -- the assertions stay."""
import numpy as np
import pytest

import sa_window_model as M

ROUND1_KINDS = (
    "small-inside", "small-straddle", "1024-aligned", "1024-straddle",
    "large-1025", "large-2-windows", "large-3-windows", "large-4-or-more-windows", "large-starts-at-slot-0", "large-starts-at-last-slot",
    "large-ends-on-edge", "large-ends-list",
    "window-inside-large", "A+B", "A+small+B", "small-tail+B",
    "last-window-ragged", "list-multiple-of-1024", "last-window-single-slot",
)
ROUND2_KINDS = ("large-2-windows", "large-3-windows", "large-4-or-more-windows", "A+B", "window-inside-large", "small-straddle", "last-window-ragged")


def _oracle_sizes(oracle, t, h):
    """the definition, from the suffix array: runs of neighbours that agree over h bytes (a suffix shorter than h is padded with a byte
    the text does not have)"""
    sa = oracle.suffix_array(t).astype(np.int64)
    pad = np.concatenate((t, np.zeros(h, dtype=np.uint8)))
    same = np.ones(len(t) - 1, dtype=bool)
    for k in range(h):
        col = pad[sa + k]
        same &= col[1:] == col[:-1]
    sizes = np.diff(np.flatnonzero(np.concatenate(([True], ~same, [True]))))
    return sizes[sizes > 1]


def test_kinds_of_lists_made_by_hand():
    """the model's own definitions on lists small enough to check by eye (W = 1024)"""
    assert M.kinds([1024]) == {"small-inside", "1024-aligned", "list-multiple-of-1024"}
    assert M.kinds([1, 1024]) == {"small-inside", "small-straddle", "1024-straddle", "last-window-single-slot", "last-window-ragged"}
    assert M.kinds([1025]) == {"large-1025", "large-2-windows", "large-starts-at-slot-0", "large-ends-list", "window-inside-large",
                               "last-window-single-slot", "last-window-ragged"}                   # window 1: one slot, no head
    # a large group on the last slot of window 0 that ends with window 1 (and the list): window 1 has no head
    assert M.kinds([1023, 1025]) == {"small-inside", "large-1025", "large-2-windows", "large-starts-at-last-slot", "large-ends-on-edge",
                                     "large-ends-list", "window-inside-large", "list-multiple-of-1024"}
    # window 1 = [1024, 2048): the tail of the first large group (ends at 1100), then the head of the next
    assert M.kind_counts([1100, 2000])["A+B"] == 1 and M.kind_counts([1100, 5, 2000])["A+small+B"] == 1
    assert "A+B" not in M.kinds([1100, 5, 2000]) and "A+B" not in M.kinds([2048, 2000])            # the second starts with its window: no tail
    assert M.kind_counts([1000, 100, 1500])["small-tail+B"] == 1                                   # 100 straddles slot 1024, 1500 starts at 1100
    assert M.kind_counts([4096])["window-inside-large"] == 3 and "large-4-or-more-windows" in M.kinds([4096])
    assert "large-3-windows" in M.kinds([1, 2048]) and "large-2-windows" in M.kinds([2048])
    assert M.large_members([1024, 1025, 3, 2000]) == 3025


def test_digit_widths_of_the_large_group_radix():
    """lg_digit_bits: kbits = bits(3 n), ceil(kbits / 8) passes of ceil(kbits / passes) bits, at least 4"""
    assert [M.lg_digit_bits(n) for n in (1, 5, 85, 10922, 10923, 21845, 21846, 87381, 87382, 699050, 699051, 5592405, 5592406)] == \
           [(1, 4), (1, 4), (1, 8), (2, 8), (2, 8), (2, 8), (3, 6), (3, 6), (3, 7), (3, 7), (3, 8), (3, 8), (4, 7)]


def test_text_lengths_cover_the_four_digit_classes_a_large_group_can_meet():
    """A block with a group above 1024 members has more than 1024 bytes, so kbits = bits(3 n) >= 12: one pass never suffices, and two
    passes of ceil(kbits / 2) >= 6 bits or three of >= 6 -- the DB = 4 and DB = 5 instantiations of k_lg_hist / k_lg_scatter cannot be
    reached by a large group (they are reached by no piece at all; the code stays).  What remains for blocks below 2^24 / 3 bytes:
      3 n in [2^15, 2^16)  2 passes of 8 bits     3 n in [2^16, 2^18)  3 passes of 6 bits
      3 n in [2^18, 2^21)  3 passes of 7 bits     3 n in [2^21, 2^24)  3 passes of 8 bits  (from n = 699 051)
    Below that, 3 n in [2^12, 2^15), it is 2 passes of 6, 7, 7 or 8 bits -- the same instantiations; the period-2 text is there (2 passes
    of 7 bits).  Every text holds a large group."""
    classes = {}
    for name in M.TEXTS:
        n = len(M.crafted(name))
        assert n <= 1_500_000 and n % M.UNIT == 0, name            # (a multiple of 120: the forward BWT sorts all of it)
        assert M.large_members(M.crafted_layout(name, M.DEPTH)) > M.WIN, name
        classes.setdefault(M.lg_digit_bits(n), []).append((name, n))
    print(classes)
    for n3_lo, n3_hi, want in ((1 << 15, 1 << 16, (2, 8)), (1 << 16, 1 << 18, (3, 6)), (1 << 18, 1 << 21, (3, 7)), (1 << 21, 1 << 24, (3, 8))):
        assert want in classes and all(n3_lo <= 3 * n < n3_hi for _, n in classes[want]), (want, classes.get(want))
    assert (2, 7) in classes


def test_the_texts_together_reach_every_kind_in_round_1():
    assert ROUND1_KINDS == M.KINDS
    total = {}
    for name in M.TEXTS:
        s = M.crafted_layout(name, M.DEPTH)
        c = M.kind_counts(s)
        print(f"{name}: {len(M.crafted(name))} bytes, round 1: {int(s.sum())} active in {len(s)} groups, {M.large_members(s)} in large groups; {dict(c)}")
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    for kind in ROUND1_KINDS:
        assert total.get(kind, 0) > 0, kind


def test_chance_alone_reaches_the_common_kinds():
    """the random-placement text: everything but what chance places once in 1024 tries"""
    got = M.kinds(M.crafted_layout("scatter-650k", M.DEPTH))
    for kind in ("small-inside", "small-straddle", "1024-straddle", "large-1025", "large-2-windows", "large-3-windows", "large-4-or-more-windows",
                 "window-inside-large", "A+B", "A+small+B", "small-tail+B", "last-window-ragged"):
        assert kind in got, kind


def test_prescribed_groups_open_and_close_the_list():
    """the stems of a prescribed text are the first groups of the round-1 list, in order, at the slots EDGE_SIZES was written for; 0xFF +
    stem closes the list with the same sizes"""
    s = M.crafted_layout("edges-213k", M.DEPTH)
    k = len(M.EDGE_SIZES)
    assert tuple(s[:k]) == M.EDGE_SIZES and tuple(s[-k:]) == M.EDGE_SIZES
    assert np.cumsum(s[:k]).tolist() == [1024, 2047, 3072, 5120, 6145, 7169, 10169, 15169, 15179, 17179, 18179, 19379]
    head = M.kind_counts(s[:k])
    for kind in ("1024-aligned", "1024-straddle", "large-starts-at-last-slot", "large-starts-at-slot-0", "large-ends-on-edge", "large-1025",
                 "large-2-windows", "large-3-windows", "large-4-or-more-windows", "window-inside-large", "A+B", "A+small+B", "small-tail+B", "small-straddle"):
        assert head[kind] > 0, kind
    assert int(s.sum()) % M.WIN == 0 and s[-1] > M.WIN                      # the list ends on a window edge, inside a large group
    one = M.crafted_layout("one-large", M.DEPTH)
    assert tuple(one[:2]) == (600, 1025) and int(one.sum()) % M.WIN == 1 and one[-1] == 1025    # the last window holds one slot: a piece of one
    mid = M.crafted_layout("edges-56k", M.DEPTH)
    assert tuple(mid[:4]) == (1023, 1025, 1024, 2047)
    assert {"large-starts-at-last-slot", "large-ends-on-edge", "1024-aligned", "large-starts-at-slot-0"} <= M.kinds(mid[:4])


def test_the_deep_stems_carry_large_groups_into_round_2():
    for name in M.DEEP:
        s = M.crafted_layout(name, 2 * M.DEPTH)
        c = M.kind_counts(s)
        print(f"{name}: round 2: {int(s.sum())} active in {len(s)} groups, {M.large_members(s)} in large groups; {dict(c)}")
        assert M.large_members(s) > 0
        for kind in ROUND2_KINDS:
            assert c[kind] > 0, (name, kind)


@pytest.mark.parametrize("name", M.TEXTS)
def test_the_model_states_the_definition(oracle, name):
    """layout() never sorts a suffix: the oracle's suffix array, neighbours compared over h bytes, gives the same groups"""
    t = M.crafted(name)
    for h in (M.DEPTH, 2 * M.DEPTH):
        assert np.array_equal(M.crafted_layout(name, h), _oracle_sizes(oracle, t, h)), (name, h)


def test_layout_refuses_texts_outside_its_premises():
    t = np.array(M.crafted("one-large"))
    for spoil in (lambda a: a.__setitem__(100, 0), lambda a: a.__setitem__(slice(200, 207), 77), lambda a: a.__setitem__(len(a) - 1, a[5])):
        bad = t.copy()
        spoil(bad)
        with pytest.raises(AssertionError):
            M.layout(bad, M.DEPTH)
