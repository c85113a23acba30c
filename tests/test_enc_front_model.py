"""enc_front_model on the CPU: the restated scheme of ans_enc_front.hip (k_enc_hist, k_enc_prep, k_enc_mtf; k_rle_lz, k_rle_ext, k_rle_tiles,
k_tile_prefix) gives the oracle's ranks, frequencies and RLE0 symbols on every crafted input, the inputs reach every named arm of the
scheme (REACH, pinned by name), and every one-token change of the scheme changes the output of the input named in DETECTS or is shown to
change none (enc_front_model.EQUIVALENT).  test_oracle_vs_ref.py pins the oracle to the reference build.

The events are conditions on the INPUTS of test_gpu_enc_front.py, not measurements of the kernels: an input builder that loses an arm
fails here, before a GPU test relies on it.

One mutant changes nothing: `prevc = readlane(b, 63)`.  prevc feeds only pb of lane 0, whose head bit `b != pb || l == 0` is true
whatever pb holds; and lane 63 differs from lane nvalid - 1 only in a tile's partial last group, after which the loop ends.  It ran on
every text, with tiles that end in partial groups of 1, 17, 63 bytes among them.

`runs-at-edges` is two texts (the seven runs the stage needs are longer than six tiles together): the second holds the run of 3 * 4096."""
import functools

import numpy as np
import pytest

import enc_front_model as M

RUN_LENS = tuple(f"run-len-2^{k}{d}" for k in range(1, 17) for d in ("-1", "", "+1"))
_FIRSTS = ("first-at-63", "first-at-64", "first-at-128", "first-at-192", "first-at-255")
_LADDER = ("run-over-segment", "run-starts-at-seg-last", "run-over-tile", "tile-first-zero-prev-zero", "ext-chain-1", "ext-chain-3") + RUN_LENS
_ZEROS = ("run-to-chunk-end", "chunk-all-zero")
_LONG_ZEROS = ("run-over-segment", "run-over-tile", "tile-first-zero-prev-zero") + _ZEROS
_EDGES = ("rank-reg0", "rank-reg1", "rank-q0-reg1", "rank-q63-reg0", "first-at-63", "first-at-64", "first-in-later-tile", "lane0-repeat",
          "tile-start-repeat", "wave-edge-run", "block-edge-run", "partial-last-group", "freq-tie")
_REGS = ("rank-reg0", "rank-reg1", "rank-reg2", "rank-reg3")
_Q_ALL = ("rank-q0-reg1", "rank-q0-reg2", "rank-q0-reg3", "rank-q63-reg0", "rank-q63-reg1", "rank-q63-reg2", "rank-q63-reg3")
_Q_SHORT = ("rank-q0-reg1", "rank-q0-reg2", "rank-q0-reg3", "rank-q63-reg0", "rank-q63-reg1", "rank-q63-reg2")

# input -> the events it reaches, all of them, in the order of M.EVENTS (rank_events of the text / rle_events of the byte array)
REACH = {
    "rr-64": ("rank-reg0", "rank-q63-reg0", "first-at-63", "partial-last-group", "freq-tie"),
    "rr-65": ("rank-reg1", "rank-q0-reg1") + _FIRSTS[:2] + ("partial-last-group", "freq-tie"),
    "rr-128": ("rank-reg1", "rank-q63-reg1") + _FIRSTS[:2] + ("partial-last-group", "freq-tie"),
    "rr-129": ("rank-reg2", "rank-q0-reg2") + _FIRSTS[:3] + ("partial-last-group", "freq-tie"),
    "rr-192": ("rank-reg2", "rank-q63-reg2") + _FIRSTS[:3] + ("partial-last-group", "freq-tie"),
    "rr-193": ("rank-reg3", "rank-q0-reg3") + _FIRSTS[:4] + ("rebuild-deep", "partial-last-group", "freq-tie"),
    "rr-256": ("rank-reg3", "rank-q63-reg3") + _FIRSTS + ("rebuild-deep", "partial-last-group", "freq-tie"),
    "rr-256-exact": ("rank-reg3", "rank-q63-reg3") + _FIRSTS + ("rebuild-deep", "freq-tie", "all-freq-equal"),
    "staircase": _REGS + ("rank-q0-reg2", "rank-q63-reg1", "rank-q63-reg2", "rank-q63-reg3") + _FIRSTS +
                 ("first-in-later-tile", "rebuild-deep", "lane0-repeat", "partial-last-group", "freq-tie"),
    "runs-at-edges": _EDGES,
    "runs-at-edges-long": _EDGES,
    "shuffled-256": _REGS + _Q_ALL + _FIRSTS + ("first-in-later-tile", "lane0-repeat", "tile-start-repeat", "wave-edge-run", "partial-last-group",
                                                "freq-tie"),
    "shuffled-256-4095": _REGS + _Q_SHORT + _FIRSTS[:4] + ("lane0-repeat", "partial-last-group", "freq-tie"),
    "shuffled-256-4096": _REGS + _Q_SHORT + _FIRSTS[:4] + ("lane0-repeat", "freq-tie"),
    "shuffled-256-4097": _REGS + ("rank-q0-reg1", "rank-q0-reg3", "rank-q63-reg0", "rank-q63-reg1", "rank-q63-reg2") + _FIRSTS[:4] +
                         ("rebuild-deep", "lane0-repeat", "partial-last-group", "tile-of-one-byte", "freq-tie"),
    "shuffled-256-16384": _REGS + _Q_ALL + _FIRSTS + ("first-in-later-tile", "lane0-repeat", "tile-start-repeat", "wave-edge-run", "freq-tie"),
    "shuffled-256-16385": _REGS + _Q_ALL + _FIRSTS + ("first-in-later-tile", "lane0-repeat", "tile-start-repeat", "wave-edge-run", "block-edge-run",
                                                      "partial-last-group", "tile-of-one-byte", "freq-tie"),
    "shuffled-256-20543": _REGS + _Q_ALL + _FIRSTS + ("first-in-later-tile", "rebuild-deep", "lane0-repeat", "tile-start-repeat", "wave-edge-run",
                                                      "block-edge-run", "partial-last-group", "freq-tie"),
    "ladder": _LADDER + ("last-tile-partial",),
    "ladder+1": _LADDER + ("last-tile-partial",),
    "ladder+15": _LADDER + ("last-tile-partial",),
    "ladder+4095": _LADDER + ("sym-256", "last-tile-partial"),
    "whole-tiles": ("run-over-segment", "run-starts-at-seg-last", "run-over-tile", "run-starts-at-tile-first-prev-nonzero",
                    "tile-first-zero-prev-zero", "ext-chain-1", "ext-chain-3", "run-len-2^12-1", "run-len-2^12", "run-len-2^12+1", "sym-256"),
    "all-zero-1": _ZEROS + ("run-len-2^1-1", "last-tile-partial"),
    "all-zero-15": _ZEROS + ("run-len-2^4-1", "last-tile-partial"),
    "all-zero-16": _ZEROS + ("run-len-2^4", "last-tile-partial"),
    "all-zero-17": ("run-over-segment",) + _ZEROS + ("run-len-2^4+1", "last-tile-partial"),
    "all-zero-4096": ("run-over-segment",) + _ZEROS + ("run-len-2^12",),
    "all-zero-4097": ("run-over-segment", "run-over-tile", "tile-first-zero-prev-zero", "ext-chain-1") + _ZEROS + ("run-len-2^12+1", "last-tile-partial"),
    "all-zero-12288": _LONG_ZEROS,
    "all-zero-1048576": _LONG_ZEROS,
    "all-zero-1048577": _LONG_ZEROS + ("last-tile-partial",),
    "zero-at-last-byte": ("run-starts-at-tile-first-prev-nonzero", "run-to-chunk-end", "run-len-2^1-1", "sym-256", "last-tile-partial"),
    "only-255": ("sym-256", "last-tile-partial"),
}

# mutant -> one input whose output it changes: the input made for the arm the mutant sits in
DETECTS = {
    "prep-tie-larger-first": "rr-256-exact",         # every frequency equal: the bucket order is the tie rule alone
    "prep-ge": "rr-64",
    "lastpos-first-lane": "shuffled-256",            # two symbols interleaved in a tile's last groups: the stamps' order flips
    "hist-valid-ignored": "shuffled-256-4095",       # one clamped lane
    "place-ge": "rr-65",
    "nseen-from-zero": "staircase",                  # first occurrences in tiles 1, 2 and 3
    "carry1-dropped": "rr-65", "carry2-dropped": "rr-129", "carry3-dropped": "rr-193",       # the rank right behind the carry
    "part-lt": "rr-128",
    "reg0-shift-lt": "rr-64",
    "lane0-not-walked": "runs-at-edges",
    "runlen-short": "shuffled-256-4096",
    "pos-plus-one": "runs-at-edges-long",
    "tilebase-inclusive": "shuffled-256-4097",       # the second tile is one byte
    "ext-no-chain": "all-zero-12288",                # two whole tiles behind the first
    "ext-over-full-only": "whole-tiles",             # a run that ends inside the tile behind the whole ones
    "after-without-ext": "all-zero-4097",
    "prev-at-tile-start-one": "all-zero-4097",       # the second tile's only byte would start a run of its own
    "prev-at-chunk-start-src": "all-zero-1",
    "digits-one-more": "all-zero-15",
    "digits-one-less": "all-zero-16",
    "digits-lsb-first": "all-zero-17",               # L = 18: 0010, not a palindrome
    "L-without-plus-one": "zero-at-last-byte",
    "sym-plus-zero": "only-255",
    "toff-inclusive": "ladder+4095",
}
# mutant -> an input that must NOT show it: what the input in DETECTS has and this one lacks is the arm
BLIND = {
    "carry1-dropped": "rr-64", "carry2-dropped": "rr-128", "carry3-dropped": "rr-192",       # ranks stay inside the registers in front
    "part-lt": "rr-64",
    "nseen-from-zero": "rr-256",                     # all symbols are seen in tile 0
    "lane0-not-walked": "rr-193",                    # no two equal neighbours
    "pos-plus-one": "rr-129",
    "hist-valid-ignored": "shuffled-256-4096",       # no partial group
    "ext-no-chain": "all-zero-4097",                 # one tile behind the first: nothing to chain
    "ext-over-full-only": "all-zero-12288",          # whole tiles only
    "prev-at-tile-start-one": "zero-at-last-byte",   # the byte before the tile is not zero
    "prev-at-chunk-start-src": "ladder+1",           # the chunk starts with a non-zero byte
    "digits-lsb-first": "all-zero-15",               # L = 16: 000 either way
    "sym-plus-zero": "all-zero-4096",
}


@functools.lru_cache(maxsize=None)
def _rank(name):
    """the model's (R, freq, events) of a text: computed once, shared, left unchanged"""
    R, f, ev = M.rank_front(M.case(name))
    R.setflags(write=False)
    return R, f, ev


@functools.lru_cache(maxsize=None)
def _rle(name):
    s, rlen, tabs = M.rle_front(M.ranks(name))
    s.setflags(write=False)
    return s, rlen, tabs


def test_the_input_lists_are_the_ones_the_stage_needs():
    assert set(REACH) == set(M.CASES) | set(M.RANKS) and len(set(M.CASES + M.RANKS)) == len(M.CASES) + len(M.RANKS)
    assert max(len(M.case(n)) for n in M.CASES) <= 6 * M.ATILE
    for d in (64, 65, 128, 129, 192, 193, 256):
        t = M.case(f"rr-{d}")
        assert len(t) == 3 * M.ATILE + 17 and len(set(t.tolist())) == d and len(set(t[:d].tolist())) == d and np.array_equal(t[d:], t[:-d])
    assert len(M.case("rr-256-exact")) == 2 * M.ATILE
    assert {len(M.case(n)) for n in M.CASES if n.startswith("shuffled-256-")} == {4095, 4096, 4097, 4 * 4096, 4 * 4096 + 1, 5 * 4096 + 63}
    assert len(set(M.case("shuffled-256").tolist())) == 256
    # the runs of runs-at-edges: (length, offset in the tile) read back from the two texts
    got = set()
    for name in ("runs-at-edges", "runs-at-edges-long"):
        t = M.case(name)
        edge = np.flatnonzero(np.concatenate(([True], t[1:] != t[:-1], [True])))
        got |= {(int(b - a), int(a % M.ATILE)) for a, b in zip(edge[:-1], edge[1:]) if b - a > 1}
    assert {ln for ln, _ in got} == {63, 64, 65, 4095, 4096, 4097, 3 * 4096} and {at for _, at in got} == {1, 63, 4095}
    assert {len(M.ranks(f"all-zero-{n}")) for n in M.ALL_ZERO} == {1, 15, 16, 17, 4096, 4097, 3 * 4096, 1 << 20, (1 << 20) + 1}
    assert set(M.LADDER) >= set(range(1, 41)) | {(1 << k) + d for k in range(6, 17) for d in (-1, 0, 1)}
    assert max(len(M.ranks(n)) for n in M.RANKS) == (1 << 20) + 1 and max(len(M.image(n)) for n in M.IMAGES) == (1 << 20) + 4097
    lad = M.ranks("ladder")
    assert set(lad[lad != 0].tolist()) <= set(range(1, 256)) and M.ranks("zero-at-last-byte")[-1] == 0 and M.ranks("zero-at-last-byte")[:-1].all()
    for k in (1, 15, 4095):
        s = M.ranks(f"ladder+{k}")
        assert np.array_equal(s[k:], lad) and s[:k].all()


@pytest.mark.parametrize("name", M.CASES)
def test_rank_model_equals_oracle_and_reach(oracle, name):
    t = M.case(name)
    R, f, ev = _rank(name)
    r, of = oracle.rank_encode(t)
    assert np.array_equal(f, of), name
    assert np.array_equal(R[:len(t)], r), f"{name}: first difference at {np.flatnonzero(R[:len(t)] != r)[:4].tolist()}"
    assert (R[len(t):] == M.STALE_RANK).all(), "nothing lands outside the chunk"
    assert np.array_equal(oracle.rank_decode(r, of), t)
    assert tuple(e for e in M.RANK_EVENTS if ev[e]) == REACH[name]
    print(name, {e: int(ev[e]) for e in REACH[name]})


@pytest.mark.parametrize("name", M.RANKS)
def test_rle_model_equals_oracle_and_reach(oracle, name):
    r = M.ranks(name)
    s, rlen, (lz, ext, tcount, toff) = _rle(name)
    want = oracle.rle_encode(r)
    assert rlen == len(want) and np.array_equal(s, want), f"{name}: {rlen} vs {len(want)} symbols"
    assert np.array_equal(oracle.rle_decode(want, len(r)), r)
    assert int(tcount.sum()) == rlen <= len(r) and (ext <= len(r)).all()
    ev = M.rle_events(r)
    assert tuple(e for e in M.RLE_EVENTS if ev[e]) == REACH[name]
    print(name, rlen, {e: int(ev[e]) for e in REACH[name] if not e.startswith("run-len")})


def test_every_event_is_reached():
    by = {e: [n for n in REACH if e in REACH[n]] for e in M.EVENTS}
    assert not [e for e, names in by.items() if not names], by
    assert set(e for v in REACH.values() for e in v) == set(M.EVENTS) and len(M.EVENTS) == len(set(M.EVENTS))
    for e, names in by.items():
        print(f"{e}: {', '.join(names)}")
    # the arms the inputs were made for, by name
    for d, e in ((64, "rank-q63-reg0"), (65, "rank-q0-reg1"), (128, "rank-q63-reg1"), (129, "rank-q0-reg2"), (192, "rank-q63-reg2"),
                 (193, "rank-q0-reg3"), (256, "rank-q63-reg3")):
        assert e in REACH[f"rr-{d}"]
    for d, e in ((64, "first-at-63"), (65, "first-at-64"), (129, "first-at-128"), (193, "first-at-192"), (256, "first-at-255")):
        assert e in REACH[f"rr-{d}"]
    assert "all-freq-equal" in REACH["rr-256-exact"]
    for e in ("tile-start-repeat", "wave-edge-run", "block-edge-run", "lane0-repeat"):
        assert e in REACH["runs-at-edges"] and e in REACH["runs-at-edges-long"]
    assert "tile-of-one-byte" in REACH["shuffled-256-4097"] and "tile-of-one-byte" in REACH["shuffled-256-16385"]
    assert "ext-chain-1" in REACH["whole-tiles"] and "ext-chain-3" in REACH["whole-tiles"] and set(RUN_LENS) <= set(REACH["ladder"])


def test_staircase_first_occurrences(oracle):
    """first occurrences at nseen 63 and 64 in tile 0, 128 in tile 1, 192 in tile 2 and 255 in tile 3; tiles 3 and 4 start, with 220 and 256 symbols seen, 64 deep or deeper"""
    t = M.case("staircase")
    first = {}
    for i, b in enumerate(t.tolist()):
        first.setdefault(b, i)
    order = sorted(first.values())
    assert len(order) == 256 and [order[k] // M.ATILE for k in (63, 64, 128, 192, 255)] == [0, 0, 1, 2, 3]
    assert len(t) == 5 * M.ATILE + 63 and len(set(t[3 * M.ATILE: 4 * M.ATILE].tolist())) >= 64 and t[4 * M.ATILE] not in t[3 * M.ATILE: 4 * M.ATILE]
    R, f, ev = _rank("staircase")
    assert ev["rebuild-deep"] == 2 and ev["first-in-later-tile"] == 256 - 100


@pytest.mark.parametrize("mut", [m for m in M.MUTANTS if m not in M.EQUIVALENT])
def test_every_mutant_changes_the_named_input(mut):
    assert set(DETECTS) == set(M.MUTANTS) - set(M.EQUIVALENT)

    def changed(name):
        if mut in M.RANK_MUTANTS:
            R, f, _ = _rank(name)
            R2, f2, _ = M.rank_front(M.case(name), mut)
            return not (np.array_equal(R, R2) and np.array_equal(f, f2))
        s, rlen, _ = _rle(name)
        s2, rlen2, _ = M.rle_front(M.ranks(name), mut)
        return not (rlen == rlen2 and np.array_equal(s, s2))

    assert changed(DETECTS[mut]), f"{mut} changes nothing on {DETECTS[mut]}"
    if mut in BLIND:
        assert not changed(BLIND[mut]), f"{mut} shows on {BLIND[mut]}, which lacks its arm"


@pytest.mark.parametrize("mut", sorted(M.EQUIVALENT))
def test_equivalent_mutants_change_nothing(mut):
    assert mut in M.MUTANTS and len(M.EQUIVALENT[mut]) > 40, "every entry carries its reason"
    assert mut in M.RANK_MUTANTS
    partial = set()
    for name in M.CASES:
        t = M.case(name)
        R, f, _ = _rank(name)
        R2, f2, _ = M.rank_front(t, mut)
        assert np.array_equal(R, R2) and np.array_equal(f, f2), name
        partial.add(len(t) % M.WAVE)
    assert {1, 17, 63} <= partial                  # it ran where lane 63 is past the tile's end


@pytest.mark.parametrize("name", M.IMAGES)
def test_images_chunk_by_chunk(oracle, name):
    img = M.image(name)
    cs = M.chunks(img)
    assert len(cs) == 2 and len(cs[0]) == M.CHUNK and len(M.IMAGE_REACH[name]) == 2
    for k, c in enumerate(cs):
        R, f, ev = M.rank_front(c)
        r, of = oracle.rank_encode(c)
        assert np.array_equal(f, of) and np.array_equal(R[:len(c)], r) and (R[len(c):] == M.STALE_RANK).all(), (name, k)
        s, rlen, _ = M.rle_front(r)
        assert np.array_equal(s, oracle.rle_encode(r)), (name, k)
        ev2 = M.rle_events(r)
        missing = [e for e in M.IMAGE_REACH[name][k][0] if not ev[e]] + [e for e in M.IMAGE_REACH[name][k][1] if not ev2[e]]
        assert not missing, (name, k, missing)
        print(name, "chunk", k, len(c), {e: int(ev[e]) for e in M.IMAGE_REACH[name][k][0]}, {e: int(ev2[e]) for e in M.IMAGE_REACH[name][k][1]})
    if name == "edge-zeros":
        # chunk one's rank array ends in the bucket of its least frequent symbol: one head at offset 4094 of a tile, then zeros to the
        # chunk's end -- three whole tiles behind the one the run starts in; chunk two begins with the same byte, as a first occurrence
        r, f = oracle.rank_encode(cs[0])
        tail = 3 * M.ATILE + 2
        assert (cs[0][-tail:] == 200).all() and cs[0][-tail - 1] != 200 and cs[1][0] == 200 and f[200] == tail == min(f[f > 0])
        assert r[-tail] != 0 and not r[-tail + 1:].any() and (M.CHUNK - tail + 1) % M.ATILE == M.ATILE - 1
        assert M.rle_front(r)[2][1][-4] == 3 * M.ATILE                     # ext[] of the tile the run starts in: it stops at the chunk's end
        assert oracle.rank_encode(cs[1])[0][0] == 0
    if name == "ragged-1":
        assert len(cs[1]) == 1
    if name == "ragged-4097":
        assert len(cs[1]) == 4097
    if name == "rr-193-split":
        a = M.CHUNK - 2 * M.ATILE - 100
        assert np.array_equal(img[a + 193:], img[a: -193]) and len(set(img[a:].tolist())) == 193


def test_group_blocks(oracle):
    blocks = M.group()
    assert len(blocks) == 12 and [len(b) + M.TRAILER for b in blocks[::2]] == [4095, 4096, 4097, 8192, 3 * 4096 + 1, 70_001]
    for i, b in enumerate(blocks):
        assert len(b) == len(blocks[i - i % 2]) and (len(set(b.tolist())) == (1, 193)[i % 2])
        img = oracle.bwt_forward(b)
        assert len(img) == len(b) + M.TRAILER
        R, f, ev = M.rank_front(img)
        r, of = oracle.rank_encode(img)
        assert np.array_equal(f, of) and np.array_equal(R[:len(img)], r), i
        assert np.array_equal(M.rle_front(r)[0], oracle.rle_encode(r)), i
