"""enc_quasi_model on the CPU: the restated index scheme of the rANS encoder's middle (k_cls_count, k_cls_prefix, k_cls_ord, k_quasi_build
and the QuasiModel half of k_pairs) gives the oracle's pair words on every crafted stream and on its decoy, the streams reach every named
edge of the scheme (REACH, pinned by name), every one-token change of the scheme changes a word of the cases named in CAUGHT or is shown to
change none (enc_quasi_model.EQUIVALENT), and qbound / qinterval are the sequential rebuild schedule in closed form.

The events are conditions on the INPUTS of test_gpu_enc_quasi.py, not measurements of the kernels: an input builder that loses an edge
fails here.  A case is run AFTER its decoy on the same model arena, as the GPU test runs it on the same context: every table the skip rule
leaves out and every bin a short clear leaves behind then holds the decoy's mirrored values.

Seven of the mutants the scheme invites change no word of any input, and the tests say so instead of naming a case (the reasons are in
EQUIVALENT): the branch of qbound switched at 12 or 14, the skip rule with <=, q0 taken from clsbase + 1, the lg loop with >=, match_any
without `valid`, and k_cls_count's mask of the ragged tile dropped.  The edges they sit on are held by their neighbours: qbound-lo+1 /
qbound-hi+1, skip+2 and skip-next-bound (one-class-r-d at -1, 0, +1), flush-q0+1, the ragged cases.

REACH's entries are (deepest interval that codes a symbol: table-0 .. table-r are all reached; deepest lg: lg-0 .. lg-k are; the other
events).  For a case the list is complete; for a chunk of an image or a block of the group it is what that input is there for."""
import functools

import numpy as np
import pytest

import enc_quasi_model as M

TOPS = tuple(f"mantissa-top-coded-{e}" for e in range(2, 8))

_DEEP = ("q-13-to-14", "tile-starts-at-bound-1", "tile-in-one-interval", "tile-spans-9-intervals", "wave-of-one-class")
_DEEP7 = _DEEP + ("mantissa-top-coded-7", "sym-256", "one-bin-interval")
# case, image/chunk or group block -> (deepest table, deepest lg, events)
REACH = {
    "one-class-1--1": (0, -1, ("total-at-bound-1@r<=3", "tile-in-one-interval")),
    "one-class-1-0": (0, -1, ("total-at-bound@r<=3", "tile-in-one-interval", "rlen-odd-last-quasi")),
    "one-class-1-1": (1, 0, ("total-at-bound+1@r<=3",)),
    "one-class-2--1": (1, 0, ("total-at-bound-1@r<=3", "rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "one-class-2-0": (1, 0, ("total-at-bound@r<=3", "mantissa-top-coded-2")),
    "one-class-2-1": (2, 0, ("total-at-bound+1@r<=3", "tile-spans-3-intervals", "rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "one-class-3--1": (2, 0, ("total-at-bound-1@r<=3", "tile-spans-3-intervals", "mantissa-top-coded-2")),
    "one-class-3-0": (2, 0, ("total-at-bound@r<=3", "tile-spans-3-intervals", "rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "one-class-3-1": (3, 0, ("total-at-bound+1@r<=3", "mantissa-top-coded-2")),
    "one-class-10--1": (9, 0, ("tile-starts-at-bound-1", "tile-spans-9-intervals", "class-only-at-0", "wave-of-one-class",
                               "last-tile-of-1", "rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "one-class-10-0": (9, 0, _DEEP[1:] + ("mantissa-top-coded-2",)),
    "one-class-10-1": (10, 1, ("tile-starts-at-bound-1", "tile-spans-9-intervals", "wave-of-one-class", "rlen-odd-last-quasi",
                               "mantissa-top-coded-2")),
    "one-class-13--1": (12, 3, _DEEP[1:] + ("mantissa-top-coded-2",)),
    "one-class-13-0": (12, 3, _DEEP[1:] + ("rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "one-class-13-1": (13, 4, _DEEP[1:] + ("mantissa-top-coded-2",)),
    "one-class-14--1": (13, 4, ("total-at-bound-1@r=14",) + _DEEP[1:] + ("rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "one-class-14-0": (13, 4, ("total-at-bound@r=14",) + _DEEP[1:] + ("mantissa-top-coded-2",)),
    "one-class-14-1": (14, 5, ("q-13-to-14", "total-at-bound+1@r=14") + _DEEP[1:] + ("rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "class7-full": (27, 5, ("q-13-to-14", "q-27") + _DEEP[1:] + ("mantissa-top-coded-7", "sym-256", "remainder-ge-64")),
    "all-256": (15, 5, _DEEP7 + ("remainder-ge-64",)),
    "skew-128": (15, 5, _DEEP7 + ("remainder-ge-64",)),
    "skew-128-gap": (15, 5, _DEEP7 + ("freq-1-coded", "remainder-ge-64")),
    "uniform-300k": (14, 5, ("q-13-to-14", "tile-starts-at-bound-1", "tile-in-one-interval", "tile-spans-9-intervals") + TOPS +
                     ("sym-256", "remainder-ge-64")),
    "tile-bounds": (5, 0, ("total-at-bound-1@r<=3", "tile-starts-at-bound-1", "tile-starts-at-bound", "tile-starts-at-bound+1",
                           "tile-in-one-interval", "tile-spans-3-intervals", "class-absent-from-tile", "class-only-at-4095", "class-only-at-0",
                           "class-skips-a-wave", "wave-of-one-class", "wave-of-eight-classes", "mantissa-top-coded-3", "mantissa-top-coded-5")),
    "ragged-1": (8, 0, ("total-at-bound+1@r<=3", "tile-spans-9-intervals", "class-absent-from-tile", "class-only-at-0", "last-tile-of-1",
                        "rlen-odd-last-quasi") + TOPS + ("sym-256", "remainder-ge-64")),
    "ragged-4095": (8, 0, ("tile-starts-at-bound+1", "tile-in-one-interval", "tile-spans-9-intervals", "wave-of-eight-classes",
                           "last-tile-of-4095", "rlen-odd-last-quasi") + TOPS + ("sym-256", "remainder-ge-64")),
    "odd-last-quasi": (9, 0, ("tile-in-one-interval", "tile-spans-9-intervals", "class-absent-from-tile", "class-only-at-0",
                              "wave-of-eight-classes", "last-tile-of-1", "rlen-odd-last-quasi") + TOPS + ("sym-256", "remainder-ge-64")),
    "tops": (6, 0, TOPS + ("sym-256", "remainder-ge-64")),
    "three-chunks/0": (20, 5, ("q-13-to-14", "tile-starts-at-bound+1", "tile-in-one-interval", "tile-spans-3-intervals",
                               "wave-of-eight-classes", "rlen-odd-last-quasi", "sym-256", "remainder-ge-64") + TOPS),
    "three-chunks/1": (21, 5, ("q-13-to-14", "tile-in-one-interval", "tile-spans-9-intervals", "rlen-odd-last-quasi", "mantissa-top-coded-2")),
    "three-chunks/2": (11, 2, ("tile-in-one-interval", "tile-spans-3-intervals", "class-absent-from-tile", "wave-of-eight-classes",
                               "rlen-odd-last-quasi", "sym-256", "remainder-ge-64") + TOPS),
    "sixteen-chunks/0": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/1": (18, 5, ("q-13-to-14",)),
    "sixteen-chunks/2": (20, 5, ("q-13-to-14", "wave-of-eight-classes", "sym-256", "remainder-ge-64")),
    "sixteen-chunks/3": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/4": (19, 5, ("q-13-to-14", "wave-of-eight-classes", "remainder-ge-64")),
    "sixteen-chunks/5": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/6": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/7": (20, 5, ("q-13-to-14", "wave-of-eight-classes", "sym-256", "remainder-ge-64")),
    "sixteen-chunks/8": (18, 5, ("q-13-to-14",)),
    "sixteen-chunks/9": (19, 5, ("q-13-to-14", "wave-of-eight-classes", "remainder-ge-64")),
    "sixteen-chunks/10": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/11": (-1, -1, ()),                                   # one byte: twenty run bits, no QuasiModel symbol at all
    "sixteen-chunks/12": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/13": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/14": (19, 5, ("q-13-to-14",)),
    "sixteen-chunks/15": (7, 0, ("wave-of-eight-classes", "last-tile-of-1", "sym-256", "remainder-ge-64")),
    "group-0": (10, 1, ("tile-spans-9-intervals", "freq-1-coded")),
    "group-1": (10, 1, ("freq-1-coded",)),
    "group-2": (10, 1, ("class-skips-a-wave", "freq-1-coded")),
    "group-3": (10, 1, ("class-skips-a-wave", "freq-1-coded")),
    "group-4": (11, 2, ("freq-1-coded", "remainder-ge-64")),
    "group-5": (11, 2, ("freq-1-coded", "remainder-ge-64")),
    "group-6": (11, 2, ("sym-256", "remainder-ge-64")),
    "group-7": (11, 2, ("freq-1-coded",)),
}

# case -> the mutants that change a word of it, all of them (the cases above 100 000 symbols: of the mutants in M.BIG_MUTANTS)
_COMMON = {"qbound-lo+1", "qinterval-<", "hist-of-r", "flush-q0+1", "wave-prefix-inclusive", "below-le", "plus1-dropped", "remainder-to-last",
           "cdf-end-unwritten", "m-without-base"}
_NEXT, _PLUS2, _STUCK, _CARRY = {"skip-next-bound"}, {"skip+2"}, {"wave-count-stuck"}, {"carry-dropped"}
CAUGHT = {
    "one-class-1--1": {"wave-prefix-inclusive", "m-without-base"},       # table 0 alone: only an ordinal pushed past 8 shows
    "one-class-1-0": {"below-le", "m-without-base"},
    "one-class-1-1": (_COMMON - {"cdf-end-unwritten"}) | _PLUS2 | _NEXT,
    "one-class-2--1": _COMMON | _NEXT,
    "one-class-2-0": _COMMON,
    "one-class-2-1": _COMMON | _PLUS2 | _NEXT,
    "one-class-3--1": _COMMON | _NEXT,
    "one-class-3-0": _COMMON,
    "one-class-3-1": _COMMON | _PLUS2 | _NEXT,
    "one-class-10--1": _COMMON | _NEXT | _STUCK,
    "one-class-10-0": _COMMON | _STUCK,
    "one-class-10-1": _COMMON | _PLUS2 | _NEXT | _STUCK,
    "one-class-13--1": _COMMON | _NEXT | _STUCK,
    "one-class-13-0": _COMMON | _STUCK,
    "one-class-13-1": _COMMON | _PLUS2 | _NEXT | _STUCK,
    "one-class-14--1": set(),
    "one-class-14-0": set(),
    "one-class-14-1": {"qbound-hi+1", "skip+2"},
    "class7-full": {"qbound-hi+1", "qhist-clear-short"},
    "all-256": set(),                                                    # one bin: the tables 13, 14 and 15 are the same table
    "skew-128": set(),
    "skew-128-gap": {"qbound-hi+1"},
    "uniform-300k": {"qbound-hi+1"},
    "tile-bounds": _COMMON | _NEXT | _STUCK,
    "ragged-1": _COMMON | _PLUS2 | _NEXT | _STUCK | _CARRY,
    "ragged-4095": _COMMON | _NEXT | _STUCK | _CARRY,
    "odd-last-quasi": _COMMON | _NEXT | _STUCK | _CARRY,
    "tops": _COMMON | _NEXT | _STUCK | _CARRY,
}
# mutants only an image of several chunks can show: image -> those that change a word of it
IMAGE_MUTANTS = ("table-offset-c8", "qhist-clear-short")
IMAGE_CAUGHT = {"three-chunks": ("table-offset-c8",)}


def _events(ev):
    """reach()'s dict in REACH's form"""
    got = [e for e in M.EVENTS if ev[e]]
    tabs = [e for e in got if e.startswith("table-")]
    lgs = [e for e in got if e.startswith("lg-")]
    assert tabs == [f"table-{r}" for r in range(len(tabs))] and lgs == [f"lg-{k}" for k in range(len(lgs))], got
    return len(tabs) - 1, len(lgs) - 1, tuple(e for e in got if not e.startswith(("table-", "lg-")))


def _expanded(entry):
    deepest, lg, rest = entry
    return {f"table-{r}" for r in range(deepest + 1)} | {f"lg-{k}" for k in range(lg + 1)} | set(rest)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def _image_symbols(name):
    """the RLE0 symbols of every chunk of an image, from the oracle's stages: computed once, shared, left unchanged"""
    out = []
    for c in M.chunks(M.image(name)):
        s = M.chunk_symbols(_oracle(), c)
        s.setflags(write=False)
        out.append(s)
    return tuple(out)


def _mirror(s):
    s = np.asarray(s, dtype=np.int64)
    e = M.sym_class(s)
    return (M._BASE[e] + M._ALPHA[e] - 1 - (s - M._BASE[e])).astype(np.uint16)


def _sweep(decoys, streams, muts):
    """the mutants of `muts` that change a word of `streams` when the call runs after the one on `decoys`, on the same arena"""
    def words(mut):
        pre = [M.ordinals(s, mut) for s in streams]                      # the classes alone: the decoy's are the same
        a = M.Arena(len(streams))
        M.run(decoys, a, mut, pre=pre)
        return [r["words"] for r in M.run(streams, a, mut, pre=pre)], [r["ord"] for r in pre]
    base, base_ord = words(None)
    caught, moved = [], []
    for m in muts:
        w, o = words(m)
        if any(not np.array_equal(x, y) for x, y in zip(w, base)):
            caught.append(m)
        if any(not np.array_equal(x, y) for x, y in zip(o, base_ord)):
            moved.append(m)
    return tuple(caught), tuple(moved)


def test_the_case_list_is_the_one_the_stage_needs():
    assert set(REACH) == set(M.CASES) | {f"{i}/{k}" for i in M.IMAGES for k in range(len(M.chunks(M.image(i))))} | set(M.GROUP)
    assert set(CAUGHT) == set(M.CASES) and len(set(M.CASES)) == len(M.CASES)
    for r, d in M.ONE_CLASS:
        s = M.case(f"one-class-{r}-{d}")
        assert len(s) == M.qbound(r) + d and set(M.sym_class(s).tolist()) == {2}
    assert (1, -1) in M.ONE_CLASS and (14, 1) in M.ONE_CLASS and len(M.ONE_CLASS) == 18
    assert len(M.case("class7-full")) == M.CHUNK and int(M.case("class7-full").min()) >= 128
    assert len(M.case("all-256")) == len(M.case("skew-128")) == M.qbound(15) + 5
    assert set(M.case("all-256").tolist()) == {256}
    sk = M.case("skew-128")
    assert np.array_equal(np.flatnonzero(sk == 256), np.arange(4096, len(sk), 4097)) and set(sk.tolist()) == {128, 256}
    assert [len(M.case(n)) for n in ("ragged-1", "ragged-4095", "odd-last-quasi")] == [4097, 8191, 12289]
    assert M.sym_class(M.case("odd-last-quasi")[-1]) == 5
    assert len(M.image("three-chunks")) == (2 << 20) + 70_001 and len(M.image("sixteen-chunks")) == (15 << 20) + 4097
    assert len(M.group()) == 8 and all(30_000 <= len(t) <= 70_000 for t in M.group())
    for name in M.CASES:                                                 # the decoy: same classes, no mantissa kept
        s, d = M.case(name).astype(np.int64), M.decoy(name).astype(np.int64)
        e = M.sym_class(s)
        assert np.array_equal(M.sym_class(d), e) and np.array_equal((s - M._BASE[e]) + (d - M._BASE[e]), M._ALPHA[e] - 1)


@pytest.mark.parametrize("name", M.CASES)
def test_model_equals_oracle_and_reach(oracle, name):
    s, d = M.case(name), M.decoy(name)
    a = M.Arena(1)
    rd = M.run([d], a)[0]
    want_d = oracle.model_pairs(d)
    assert np.array_equal(M.splice(want_d, rd), want_d), "the decoy, on a fresh arena"
    rs = M.run([s], a)[0]
    want = oracle.model_pairs(s)
    assert np.array_equal(M.splice(want, rs), want), "the case, behind its decoy"
    assert np.array_equal(rs["ord"], rd["ord"])
    ev = M.reach(s)
    deepest, lg, rest = _events(ev)
    assert (deepest, lg, set(rest)) == (REACH[name][0], REACH[name][1], set(REACH[name][2])), (deepest, lg, rest)
    print(name, len(s), {e: int(ev[e]) for e in M.EVENTS if ev[e] and not e.startswith("table-")})


def test_every_event_is_reached():
    by = {e: [n for n in M.CASES if e in _expanded(REACH[n])] for e in M.EVENTS}
    assert not [e for e, names in by.items() if not names], by
    # what each case is there for, by name
    for r, d in M.ONE_CLASS:
        ev = _expanded(REACH[f"one-class-{r}-{d}"])
        if r <= 3 or r == 14:
            assert f"total-at-bound{ {-1: '-1', 0: '', 1: '+1'}[d] }@r{'<=3' if r <= 3 else '=14'}" in ev
        assert (f"table-{r}" in ev) == (d == 1), "a class of qbound(r) + 1 symbols is the first to read table r"
        if r >= 10:
            assert {"tile-spans-9-intervals", "tile-starts-at-bound-1"} <= ev                # tile 1 starts at 4096 = qbound(9) - 1
    full = _expanded(REACH["class7-full"])
    assert {"q-27", "q-13-to-14", "lg-5", "sym-256", "remainder-ge-64", "mantissa-top-coded-7"} <= full and "table-28" not in full
    assert M.reach(M.case("class7-full"))["lg-5"] == 14
    assert "one-bin-interval" in _expanded(REACH["all-256"]) and "freq-1-coded" in _expanded(REACH["skew-128-gap"])
    tb = _expanded(REACH["tile-bounds"])
    assert {"tile-starts-at-bound-1", "tile-starts-at-bound", "tile-starts-at-bound+1", "class-only-at-0", "class-only-at-4095",
            "class-skips-a-wave", "wave-of-one-class", "wave-of-eight-classes", "class-absent-from-tile", "tile-in-one-interval",
            "tile-spans-3-intervals"} <= tb
    r = M.run([M.case("tile-bounds")])[0]
    assert r["clsbase"][1:10, 3].tolist() == [M.qbound(q) + d for q in (1, 2, 5) for d in (-1, 0, 1)]
    assert "last-tile-of-1" in _expanded(REACH["ragged-1"]) and "last-tile-of-4095" in _expanded(REACH["ragged-4095"])
    assert "rlen-odd-last-quasi" in _expanded(REACH["odd-last-quasi"])
    assert set(TOPS) <= _expanded(REACH["tops"]) and REACH["tops"][0] >= 3
    assert set(f"lg-{k}" for k in range(6)) <= _expanded(REACH["uniform-300k"]) and set(TOPS) <= _expanded(REACH["uniform-300k"])


@pytest.mark.parametrize("name", M.CASES)
def test_mutants_are_caught_by_the_named_cases(name):
    s = M.case(name)
    muts = M.MUTANTS if len(s) <= M.BIG else M.BIG_MUTANTS
    caught, moved = _sweep([M.decoy(name)], [s], muts)
    assert set(caught) == CAUGHT[name], caught
    assert not [m for m in moved if m in M.EQUIVALENT], "an equivalent mutant leaves every ordinal where it was, those of the classes 0/1 too"
    print(name, "exposes", caught)


def test_images_expose_what_only_several_chunks_can():
    for name, want in IMAGE_CAUGHT.items():
        syms = list(_image_symbols(name))
        caught, _ = _sweep([_mirror(s) for s in syms], syms, IMAGE_MUTANTS)
        assert caught == want
        print(name, "exposes", caught)


def test_every_mutant_is_caught_or_equivalent():
    assert set(M.EQUIVALENT) < set(M.MUTANTS) and set(M.BIG_MUTANTS) <= set(M.MUTANTS)
    for m in M.MUTANTS:
        names = [n for n in M.CASES if m in CAUGHT[n]] + [n for n in IMAGE_CAUGHT if m in IMAGE_CAUGHT[n]]
        assert bool(names) != (m in M.EQUIVALENT), (m, names)
        print(m, "->", names if names else "equivalent: " + M.EQUIVALENT[m])
    # what each edge is for, by name
    one = {(r, d): CAUGHT[f"one-class-{r}-{d}"] for r, d in M.ONE_CLASS}
    for (r, d), c in one.items():
        assert ("skip+2" in c) == (d == 1), "qbound(r) + 1 symbols: one ordinal reads the table that clstotal < qbound(r) + 2 leaves out"
        if r < 14:
            assert ("skip-next-bound" in c) == (d == 1 or (d == -1 and r > 1)), (r, d)          # the deepest table read is built a bound late
    assert "qbound-hi+1" in one[(14, 1)] and "qbound-hi+1" not in one[(14, 0)] and "qbound-lo+1" in one[(13, 1)]
    assert [n for n in M.CASES if "qhist-clear-short" in CAUGHT[n]] == ["class7-full"]          # the only histogram in the last 6 intervals
    assert "wave-count-stuck" not in one[(3, 1)] and "wave-count-stuck" in one[(10, -1)]       # needs a second iteration of a wave
    assert [n for n in M.CASES if "carry-dropped" in CAUGHT[n]] == ["ragged-1", "ragged-4095", "odd-last-quasi", "tops"]      # alphabets > 64
    # the equivalent ones ran on the inputs that could have told them apart
    assert "total-at-bound@r<=3" in _expanded(REACH["one-class-2-0"]) and "total-at-bound@r=14" in _expanded(REACH["one-class-14-0"])
    assert "tile-starts-at-bound-1" in _expanded(REACH["tile-bounds"]) and "last-tile-of-1" in _expanded(REACH["ragged-1"])
    assert "q-13-to-14" in _expanded(REACH["one-class-14-1"])


def test_schedule_is_the_sequential_one():
    """qbound / qinterval against the reference's count: rebuild after EXP + 1 symbols, EXP = 8, 16, ..., 65 536, 65 536, ..."""
    seq = np.array(M.sequential_intervals(M.CHUNK), dtype=np.int64)
    assert np.array_equal(M.qinterval(np.arange(M.CHUNK)), seq)
    starts = np.flatnonzero(np.diff(seq)) + 1
    assert starts.tolist() == [M.qbound(q) for q in range(1, 28)] and M.qbound(0) == 0
    assert int(seq[-1]) == 27 and M.qbound(27) < M.CHUNK <= M.qbound(28)
    assert M.qbound(13) == 65_541 and M.qbound(14) - M.qbound(13) == 65_537 == M.qbound(15) - M.qbound(14) and M.qbound(13) - M.qbound(12) == 32_769
    assert M.qbound(M.NQ) == 1_310_744 > M.CHUNK                         # the clamp of qinterval is out of a chunk's reach
    assert M.qinterval(np.array([M.qbound(M.NQ - 1), M.qbound(M.NQ), 1 << 31])).tolist() == [M.NQ - 1] * 3
    for e in range(8):
        A = M.class_alpha(e)
        cdf = [M.uniform_cdf(A, i) for i in range(A + 1)]
        assert cdf[0] == 0 and cdf[A] == 65536 and all(b > a for a, b in zip(cdf, cdf[1:])) and A + 1 <= M.QSTRIDE
    assert [M.class_base(e) for e in range(8)] == [0, 2, 4, 8, 16, 32, 64, 128] and M.class_alpha(7) == 129
    assert M.sym_class(np.array([0, 1, 2, 3, 4, 7, 8, 127, 128, 256])).tolist() == [0, 0, 1, 1, 2, 2, 3, 6, 7, 7]


@pytest.mark.parametrize("name", M.IMAGES)
def test_images_chunk_by_chunk(oracle, name):
    img = M.image(name)
    cs = M.chunks(img)
    syms = _image_symbols(name)
    res = M.run(list(syms))                                              # one call, every chunk's tables side by side in the arena
    for k, s in enumerate(syms):
        want = oracle.model_pairs(s)
        assert np.array_equal(M.splice(want, res[k]), want), (name, k)
        deepest, lg, rest = _events(M.reach(s, res[k]))
        assert (deepest, lg) == REACH[f"{name}/{k}"][:2] and set(REACH[f"{name}/{k}"][2]) <= set(rest), (name, k, deepest, lg, rest)
    dens = [M.density(c) for c in cs]
    order = M.launch_order(dens)
    if name == "three-chunks":
        tot = [res[k]["clstotal"] for k in range(3)]
        assert int(np.argmax(tot[0])) == 7 and int(np.argmax(tot[1][2:])) == 0 and (tot[2] > 0).all() and len(cs[2]) == 70_001
        assert int(tot[1][0]) > 50_000, "zero runs"
    else:
        assert len(cs) == 16 and len(cs[15]) == 4097
        assert np.array_equal(cs[3], cs[14]) and len(set(cs[11].tolist())) == 1
        assert order != list(range(16)) and order.index(3) + 1 == order.index(14) and dens[3] == dens[14]      # the tie: by chunk number
        assert order[0] == 2 and order[-1] == 11
        al = [len(set(c[:65536].tolist())) for c in cs[:15]]
        assert set(al) == {1, 5, 9, 17, 33, 65, 129, 256}
        d14 = [dens[k] for k in range(15)]
        assert d14 != sorted(d14) and d14 != sorted(d14, reverse=True)


def test_group_blocks_are_deep_and_differ(oracle):
    blocks = M.group()
    dominant = []
    for i, t in enumerate(blocks):
        img = oracle.bwt_forward(t)
        assert len(img) < M.CHUNK
        s = M.chunk_symbols(oracle, img)
        r = M.run([s])[0]
        want = oracle.model_pairs(s)
        assert np.array_equal(M.splice(want, r), want), i
        deepest, lg, rest = _events(M.reach(s, r))
        assert deepest >= 9 and (deepest, lg) == REACH[f"group-{i}"][:2] and set(REACH[f"group-{i}"][2]) <= set(rest), (i, deepest, lg, rest)
        dominant.append(int(np.argmax(r["clstotal"][2:])) + 2)
    assert len(set(dominant)) >= 6, dominant
