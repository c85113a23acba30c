"""The crafted streams of adapt_segment_model reach every route of the adaptive-model kernels (CPU only).

The segment kinds are conditions on the INPUTS of test_gpu_adapt_merge.py, not measurements of the code under test: a stream that
misses a kind would let a route of k_adapt_a / k_adapt_tab / k_adapt_c go unexercised there.  If a seed misses a kind, another seed
is chosen -- the assertions stay."""
import functools

import adapt_segment_model as M

SEED = 3


@functools.lru_cache(maxsize=None)
def _segments(which, seed):
    return M.classify_chunk({1: M.stream1, 2: M.stream2}[which](seed))


def _all(segs):
    return [(name, k, s) for name, lst in segs.items() for k, s in enumerate(lst)]


def test_stream_lengths():
    assert len(M.stream1(SEED)) == 32613 and len(M.stream2(SEED)) == 24289


def test_the_two_streams_reach_all_six_kinds():
    kinds = {s["kind"] for w in (1, 2) for _, _, s in _all(_segments(w, SEED))}
    assert kinds == set(M.KINDS), f"missing {set(M.KINDS) - kinds}"


def test_stream1_reaches_merge_plateau_identity_and_resolved():
    count = {k: 0 for k in M.KINDS}
    for _, _, s in _all(_segments(1, SEED)):
        count[s["kind"]] += 1
    print(count)
    for kind in ("first", "resolved", "identity", "merge", "plateau-merge"):
        assert count[kind] > 0, kind


def test_merge_steps_cover_every_residue_mod_16():
    res = {s["merge"] % 16 for w in (1, 2) for _, _, s in _all(_segments(w, SEED)) if "merge" in s}
    assert res == set(range(16)), f"missing residues {set(range(16)) - res}"


def test_stream2_has_exactly_one_table_segment_the_quiet_mantissa_run():
    """A run of zero bits behind an all-zero warm-up: the low end stalls 31 under the top, the high end sits on it, and nothing in
    the segment moves either -- but a mantissa model has no identity route, so this is what k_adapt_tab is left with."""
    for seed in (1, 2, 3):
        tab = [(name, k) for name, k, s in _all(_segments(2, seed)) if s["kind"] == "table"]
        assert tab == [("mant0", 2)], (seed, tab)
        assert sum(s["kind"] == "plateau-merge" for _, _, s in _all(_segments(2, seed))) > 0, seed


def test_a_plateau_lane_does_not_move_in_front_of_its_first_reaching_symbol():
    """what k_adapt_c's constant fill rests on: every state of [smax - 31, smax] is a fixed point of a step whose symbol does not
    reach the entry, and no lane merges before that symbol"""
    for w in (1, 2):
        sym = {1: M.stream1, 2: M.stream2}[w](SEED)
        for name, i, A, items in M.recurrences(sym):
            exact = None
            for k, s in enumerate(_segments(w, SEED)[name]):
                if s["kind"] != "plateau-merge":
                    continue
                exact = exact or M.exact_states(i, A, items)
                t0 = k * M.SEG
                assert s["reach"] < s["merge"]
                assert len(set(exact[t0:t0 + s["reach"] + 1])) == 1
                assert i + 65536 - A - 31 <= exact[t0] <= i + 65536 - A


def test_outputs_after_the_merge_step_do_not_depend_on_the_start_state():
    """walk a merged segment from both extreme candidates: from the merge step on the two trajectories are the exact one"""
    sym = M.stream1(SEED)
    for name, i, A, items in M.recurrences(sym):
        exact = M.exact_states(i, A, items)
        for k, s in enumerate(_segments(1, SEED)[name]):
            if "merge" not in s:
                continue
            t0 = k * M.SEG
            lo, hi = i, i + 65536 - A
            for t in range(t0 - M.WARM, t0 + s["merge"]):
                lo, hi = M.step(lo, i, items[t], A), M.step(hi, i, items[t], A)
            assert lo == hi == exact[t0 + s["merge"]] if t0 + s["merge"] < len(items) else lo == hi
