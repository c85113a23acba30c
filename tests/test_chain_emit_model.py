"""chain_emit_model on the CPU: the restated index scheme of the rANS encoder's back half (k_pairs' padding, k_rans_lanes' leftovers,
k_emit_count -> k_emit_prefix -> k_put_payload) gives the oracle's bytes on every crafted input, the inputs reach every named edge of the
scheme (REACH, pinned by name), every one-token change of the scheme changes the bytes of the cases named in CAUGHT or is shown to change
none (chain_emit_model.EQUIVALENT), and rans_record's 32-bit reciprocal is exact for every frequency.

The events are conditions on the INPUTS of test_gpu_chain_emit.py, not measurements of the kernels: an input builder that loses an edge
fails here.

Three of the mutants the scheme invites change no byte of any input, and the tests say so instead of naming a case:
  * the two halves of a mask word swapped: the readers add the two bits of a step (k_put_payload) or count all 32 (k_emit_count);
  * `tile * ETILE > np` in either emit kernel: the one more tile that runs when np is a multiple of 4096 counts and places nothing.
    The edge itself is held by "tile-test-late" (`(tile + 1) * ETILE >= np`), which every case catches.

The reciprocal: for fr = 1 the record's form is q = x - 1 with 65535 added to the bias, exact for x >= 1; at x = 0 it gives 65535 too
much.  No step divides a state below fr << 7 (the state is >= 2^23 before renormalisation and >= x_max >> 8 after it), so the test pins
that one value instead of asking for equality there; every other (fr, x) it checks is exact."""
import functools

import numpy as np
import pytest

import chain_emit_model as M

# case -> the events it reaches (chain_emit_model.reach on the oracle's pairs of the case), all of them
REACH = {
    "norep-1": ('pad-255', 'pad-256', 'chains-unequal', 'one-batch', 'last-batch-partial', 'tile-without-emits', 'freq-pow2>=4'),
    "norep-2": ('pad-255', 'one-batch', 'last-batch-partial', 'tile-without-emits', 'freq-pow2>=4'),
    "norep-3": ('chains-unequal', 'one-batch', 'last-batch-partial', 'tile-without-emits', 'freq-pow2>=4'),
    "norep-31": ('chains-unequal', 'one-batch', 'freq-pow2>=4'),
    "norep-32": ('one-batch', 'one@tile-first', 'emit@pair0', 'freq-pow2>=4'),
    "norep-33": ('chains-unequal', 'last-batch-partial', 'freq-pow2>=4'),
    "norep-511": ('chains-unequal', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'freq-1', 'freq-2', 'freq-pow2>=4',
                  'freq>32768'),
    "norep-512": ('pad-0', 'two@bit0', 'two@bit15', 'two@thread-last', 'one@tile-first', 'emit@pair0', 'all-16-residues-two', 'freq-1',
                  'freq-pow2>=4', 'freq>32768'),
    "norep-513": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'two@bit0', 'two@bit15', 'two@thread-last',
                  'emit@last-pair', 'freq-1', 'freq-pow2>=4', 'freq>32768'),
    "norep-1023": ('chains-unequal', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'one@tile-first', 'emit@pair0',
                   'emit@last-pair', 'all-16-residues-two', 'freq-1', 'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "norep-1024": ('pad-0', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'emit@last-pair', 'all-16-residues-two',
                   'freq-1', 'freq-2', 'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "norep-1025": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'two@bit0', 'two@bit15', 'two@thread-last',
                   'emit@last-pair', 'all-16-residues-two', 'freq-1', 'freq-pow2>=4', 'freq>32768'),
    "norep-2047": ('chains-unequal', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'emit@last-pair',
                   'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4', 'freq>32768'),
    "norep-2048": ('pad-0', 'tile-exact', 'two@bit0', 'two@bit15', 'two@thread-last', 'one@tile-first', 'emit@pair0',
                   'all-16-residues-two', 'freq-1', 'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "norep-2049": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'tile+1pair', 'tile-without-emits', 'two@bit0',
                   'two@bit15', 'two@thread-last', 'one@tile-last', 'all-16-residues-two', 'freq-1', 'freq-pow2>=4', 'freq>32768'),
    "norep-4095": ('chains-unequal', 'two@bit0', 'two@bit15', 'two@thread-last', 'one@tile-last', 'all-16-residues-two', 'freq-1',
                   'freq-2', 'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "norep-4096": ('pad-0', 'tile-exact', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'one@tile-first',
                   'one@tile-last', 'emit@pair0', 'emit@last-pair', 'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4',
                   'freq-pow2+1', 'freq>32768'),
    "norep-4097": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'tile+1pair', 'tile-without-emits', 'two@bit0',
                   'two@bit15', 'two@thread-first', 'two@thread-last', 'one@tile-last', 'all-16-residues-two', 'freq-1', 'freq-2',
                   'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "quiet-2047": ('chains-unequal', 'one@tile-first', 'emit@pair0', 'emit@last-pair', 'freq-pow2>=4', 'freq>32768'),
    "quiet-2048": ('pad-0', 'tile-exact', 'two@bit15', 'two@thread-first', 'one@tile-last', 'emit@last-pair', 'freq-1', 'freq-pow2>=4',
                   'freq>32768'),
    "quiet-2049": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'tile+1pair', 'one@tile-first', 'emit@pair0',
                   'emit@last-pair', 'freq-pow2>=4', 'freq>32768'),
    "quiet-first": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'tile+1pair', 'tile-without-emits', 'two@bit0',
                    'two@bit15', 'two@thread-first', 'two@tile-first', 'one@tile-first', 'emit@pair0', 'freq-1', 'freq-pow2>=4',
                    'freq>32768'),
    "quiet-last": ('chains-unequal', 'two@bit0', 'two@thread-last', 'two@tile-last', 'one@tile-first', 'emit@pair0', 'freq-1',
                   'freq-pow2>=4', 'freq>32768'),
    "quiet-still": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'tile+1pair', 'tile-without-emits', 'freq-pow2>=4',
                    'freq>32768'),
    "norep-131071": ('chains-unequal', 'window-exact', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'one@tile-first',
                     'one@tile-last', 'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "norep-131072": ('pad-0', 'tile-exact', 'window-exact', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last',
                     'one@tile-first', 'one@tile-last', 'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4', 'freq-pow2+1',
                     'freq>32768'),
    "norep-131073": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'tile+1pair', 'tile-without-emits', 'window+1',
                     'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'one@tile-first', 'one@tile-last',
                     'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "norep-262145": ('pad-255', 'pad-256', 'chains-unequal', 'last-batch-partial', 'tile+1pair', 'tile-without-emits', 'window+1',
                     'three-windows', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last', 'one@tile-first', 'one@tile-last',
                     'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4', 'freq-pow2+1', 'freq>32768'),
    "full-chunk": ('pad-0', 'tile-exact', 'window-exact', 'eight-windows', 'two@bit0', 'two@bit15', 'two@thread-first',
                   'two@thread-last', 'one@tile-first', 'one@tile-last', 'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4',
                   'freq-pow2+1', 'freq>32768'),
    "full-chunk-1": ('chains-unequal', 'window-exact', 'eight-windows', 'two@bit0', 'two@bit15', 'two@thread-first', 'two@thread-last',
                     'two@tile-first', 'one@tile-first', 'one@tile-last', 'all-16-residues-two', 'freq-1', 'freq-2', 'freq-pow2>=4',
                     'freq-pow2+1', 'freq>32768'),
}

# case -> the mutants that change its bytes, all of them (the cases above 140 000 symbols: of the mutants in BIG_MUTANTS)
BIG_MUTANTS = ("carry-dropped", "suffix-inclusive", "tile-test-late", "count-tile-test->", "put-tile-test->", "halves-swapped")
CAUGHT = {
    "norep-1": ('tile-test-late', 'steps-pad-down', 'pad-bits-kept'),
    "norep-2": ('tile-test-late', 'steps-pad-down', 'pad-bits-kept'),
    "norep-3": ('tile-test-late', 'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-31": ('bit-order', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive', 'first-without-chain',
                 'steps-pad-down', 'pad-bits-kept'),
    "norep-32": ('bit-order', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive', 'steps-pad-down'),
    "norep-33": ('bit-order', 'tile-test-late', 'suffix-inclusive', 'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-511": ('bit-order', 'bytes-swapped', 'count-live+1', 'count-live-1', 'put-live+1', 'put-live-1', 'tile-test-late',
                  'suffix-inclusive', 'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-512": ('bit-order', 'bytes-swapped', 'count-live+1', 'count-live-1', 'put-live+1', 'put-live-1', 'tile-test-late',
                  'suffix-inclusive'),
    "norep-513": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive',
                  'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-1023": ('bit-order', 'bytes-swapped', 'count-live+1', 'count-live-1', 'put-live+1', 'put-live-1', 'tile-test-late',
                   'suffix-inclusive', 'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-1024": ('bit-order', 'bytes-swapped', 'count-live+1', 'count-live-1', 'put-live+1', 'put-live-1', 'tile-test-late',
                   'suffix-inclusive'),
    "norep-1025": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive',
                   'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-2047": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive',
                   'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-2048": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive'),
    "norep-2049": ('bit-order', 'bytes-swapped', 'tile-test-late', 'suffix-inclusive', 'first-without-chain', 'steps-pad-down',
                   'pad-bits-kept'),
    "norep-4095": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive',
                   'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-4096": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive'),
    "norep-4097": ('bit-order', 'bytes-swapped', 'tile-test-late', 'suffix-inclusive', 'first-without-chain', 'steps-pad-down',
                   'pad-bits-kept'),
    "quiet-2047": ('bit-order', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive', 'first-without-chain',
                   'steps-pad-down', 'pad-bits-kept'),
    "quiet-2048": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive'),
    "quiet-2049": ('bit-order', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive', 'first-without-chain',
                   'steps-pad-down', 'pad-bits-kept'),
    "quiet-first": ('bit-order', 'bytes-swapped', 'tile-test-late', 'suffix-inclusive', 'first-without-chain', 'steps-pad-down',
                    'pad-bits-kept'),
    "quiet-last": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive',
                   'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "quiet-still": ('bit-order', 'tile-test-late', 'suffix-inclusive', 'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-131071": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive',
                     'first-without-chain', 'steps-pad-down', 'pad-bits-kept'),
    "norep-131072": ('bit-order', 'bytes-swapped', 'count-live-1', 'put-live-1', 'tile-test-late', 'suffix-inclusive'),
    "norep-131073": ('bit-order', 'bytes-swapped', 'tile-test-late', 'carry-dropped', 'suffix-inclusive', 'first-without-chain',
                     'steps-pad-down', 'pad-bits-kept'),
    "norep-262145": ('carry-dropped', 'suffix-inclusive', 'tile-test-late'),
    "full-chunk": ('carry-dropped', 'suffix-inclusive', 'tile-test-late'),
    "full-chunk-1": ('carry-dropped', 'suffix-inclusive', 'tile-test-late'),
}


@functools.lru_cache(maxsize=None)
def _pairs(name):
    """(symbols, pairs, emits) of a named case: computed once, shared, left unchanged"""
    from oracle.pyoracle import Oracle
    _, s, pairs = M.chunk_pairs(Oracle(), M.case(name))
    pairs.setflags(write=False)
    return s, pairs, M.emits(pairs)


def _rlen_of(name):
    return {"full-chunk": M.CHUNK, "full-chunk-1": M.CHUNK - 1}.get(name) or (M.QUIET[name][0] if name in M.QUIET else int(name.split("-")[1]))


def test_the_case_list_is_the_one_the_stage_needs():
    assert set(REACH) == set(CAUGHT) == set(M.CASES) and len(set(M.CASES)) == len(M.CASES)
    rl = {_rlen_of(n) for n in M.CASES if n.startswith("norep")}
    assert rl >= {1, 2, 3, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 131071, 131072, 131073, 262145}
    assert _rlen_of("full-chunk") == 1 << 20


@pytest.mark.parametrize("name", M.CASES)
def test_model_equals_oracle_and_reach(oracle, name):
    t = M.case(name)
    s, pairs, em = _pairs(name)
    assert len(t) == len(s) == _rlen_of(name), "the construction pins rlen"
    assert M.payload(pairs, em=em) == oracle.rans_encode_pairs(pairs).tobytes()
    _, f = oracle.rank_encode(t)
    pay = M.payload(pairs, em=em)
    whole = b"".join(M.leb(int(v)) for v in f) + M.leb(len(t)) + M.leb(len(pay)) + M.leb(len(s)) + pay
    assert whole == oracle.ans_encode(t).tobytes()
    ev = M.reach(pairs, em)
    assert tuple(e for e in M.EVENTS if ev[e]) == REACH[name]
    print(name, {e: int(ev[e]) for e in REACH[name]})


def test_every_event_is_reached():
    by = {e: [n for n in M.CASES if e in REACH[n]] for e in M.EVENTS}
    assert not [e for e, names in by.items() if not names], by
    # the searched ones, by name
    assert "two@tile-first" in REACH["quiet-first"] and "two@tile-last" in REACH["quiet-last"]
    assert "tile-without-emits" in REACH["quiet-still"] and "eight-windows" in REACH["full-chunk"] and "three-windows" in REACH["norep-262145"]
    s, pairs, em = _pairs("quiet-first")
    assert em[0][M.ETILE] == 2                                                  # pair 4096: the first of tile 1
    s, pairs, em = _pairs("quiet-last")
    assert em[0][M.ETILE - 1] == 2 and s[M.ETILE // 2 - 1] == 3                 # pair 4095: the mantissa of the rank-2 symbol
    s, pairs, em = _pairs("quiet-still")
    assert M.reach(pairs, em)["tile-without-emits"] == 8


@pytest.mark.parametrize("name", M.CASES)
def test_mutants_are_caught_by_the_named_cases(name):
    s, pairs, em = _pairs(name)
    base = M.place(pairs, em=em)[:2]
    muts = M.MUTANTS if len(s) <= 140_000 else BIG_MUTANTS
    assert tuple(m for m in muts if M.place(pairs, m, em=em)[:2] != base) == CAUGHT[name]


def test_every_mutant_is_caught_or_equivalent():
    assert set(M.EQUIVALENT) < set(M.MUTANTS)
    for m in M.MUTANTS:
        names = [n for n in M.CASES if m in CAUGHT[n]]
        assert bool(names) != (m in M.EQUIVALENT), (m, names)
    # what each edge is for, by name
    want = {
        "count-live+1": {"norep-511", "norep-512", "norep-1023", "norep-1024"},      # the word behind the last batch is the first STALE one
        "put-live+1": {"norep-511", "norep-512", "norep-1023", "norep-1024"},        #   only where the chain's batches end a ring round
        "carry-dropped": {"norep-131073", "norep-262145", "full-chunk", "full-chunk-1"},     # a second window
    }
    for m, names in want.items():
        assert {n for n in M.CASES if m in CAUGHT[n]} == names, m
    for m in ("first-without-chain", "pad-bits-kept", "steps-pad-down"):
        assert m in CAUGHT["norep-513"] and m in CAUGHT["norep-3"]
    assert "first-without-chain" not in CAUGHT["norep-512"] and "first-without-chain" not in CAUGHT["norep-2"]     # even rlen: equal chains
    assert "pad-bits-kept" not in CAUGHT["norep-512"]                                                            # no pad step at all
    for m in ("bit-order", "bytes-swapped"):
        assert m in CAUGHT["quiet-first"] and m in CAUGHT["quiet-last"] and m in CAUGHT["norep-512"]
    # the equivalent ones ran on the inputs that could have told them apart: np a multiple of 4096, two-byte emits in both halves
    for n in ("norep-2048", "norep-4096", "norep-131072", "full-chunk"):
        assert "tile-exact" in REACH[n]


@pytest.mark.parametrize("name", M.IMAGES)
def test_images_chunk_by_chunk(oracle, name):
    img = M.image(name)
    _, _, r1, r2 = M.IMAGE_SPECS[name]
    cs = M.chunks(img)
    assert len(cs) == 2 and len(cs[0]) == M.CHUNK and len(cs[1]) == r2
    whole = b""
    for k, c in enumerate(cs):
        _, s, pairs = M.chunk_pairs(oracle, c)
        assert len(s) == (r1, r2)[k]
        em = M.emits(pairs)
        assert M.payload(pairs, em=em) == oracle.rans_encode_pairs(pairs).tobytes()
        ev = M.reach(pairs, em)
        assert not [e for e in M.IMAGE_REACH[name][k] if not ev[e]], (name, k)
        whole += M.chunk_stream(oracle, c)
    assert whole == oracle.ans_encode(img).tobytes()


def test_group_blocks_have_the_searched_rlens(oracle):
    blocks = M.group()
    assert len(blocks) >= 8 and [len(b) for b in blocks] == list(M.GROUP_LENS)
    got = {}
    for b in blocks:
        cs = M.chunks(oracle.bwt_forward(b))
        assert len(cs) == 1
        _, s, pairs = M.chunk_pairs(oracle, cs[0])
        got[len(b)] = len(s)
        assert M.payload(pairs) == oracle.rans_encode_pairs(pairs).tobytes()
    assert {n: got[n] for n in M.GROUP_RLENS} == M.GROUP_RLENS
    rl = set(got.values())
    assert {511, 512, 513} <= rl and {1535, 1536, 1537} <= rl and 2048 in rl      # a multiple of 512 and that +-1, twice; a multiple of 2048


def test_layout_against_the_kernels_formulas():
    """layout() against the expressions of k_pairs / k_rans_lanes / the emit kernels, and the bounds k_pairs' pad writes rest on"""
    for rl in list(range(0, 1100)) + [2047, 2048, 2049, 131071, 131072, 131073, 262145, (1 << 20) - 1, 1 << 20]:
        np_ = 2 * rl
        lay = M.layout(np_)
        if np_:
            assert lay["steps_pad"] == 16 * lay["nbatch"] == ((((np_ - 1) // 4) // 16 + 1) + 15 & ~15) * 16
            assert sum(lay["steps"]) == np_ and lay["steps"][0] == (np_ + 3) // 4
            for ch in range(4):
                a, b = lay["identity_written"][ch]
                assert a == lay["steps"][ch] and b == lay["steps_pad"] and 0 <= lay["identity"][ch] == b - a <= 256 < M.PAD_SPAN
            assert lay["batches"] <= lay["nbatch"] and lay["tiles"] * 64 >= lay["batches"] > (lay["tiles"] - 1) * 64
            assert (lay["identity"][0] == 0) == (rl % 512 in (0, 511)) and (max(lay["identity"]) == 0) == (rl % 512 == 0)
            assert (lay["identity"][3] == 256) == (rl % 512 == 1)
        assert lay["windows"] == (lay["tiles"] + 63) // 64


def test_reciprocal_records_are_exact_for_every_frequency():
    rng = np.random.default_rng(4)
    fr = np.arange(1, 65536, dtype=np.uint64)
    lo = rng.integers(0, 65537 - fr)                                            # low + freq <= 65536
    rec = M.record(lo, fr)
    xmax, rcp, bias, w = rec
    assert xmax.dtype == rcp.dtype == bias.dtype == w.dtype == np.uint32
    # the reciprocal against the 64-bit division it replaces
    big = fr >= 2
    sh = np.array([int(f - 1).bit_length() for f in fr.tolist()], dtype=np.uint64)
    exact = ((np.uint64(1) << (sh + np.uint64(31))) + fr - np.uint64(1)) // fr
    assert np.array_equal(rcp[big].astype(np.uint64), exact[big]) and int(rcp[0]) == 0xFFFFFFFF
    assert np.array_equal((w >> np.uint32(24)).astype(np.uint64)[big], sh[big] - np.uint64(1)) and int(w[0]) >> 24 == 0
    assert np.array_equal(xmax.astype(np.uint64), fr << np.uint64(15))
    # the step's form against the division, on renormalised states (x < fr << 15 <= 2^31)
    top = fr << np.uint64(15)
    xs = [np.zeros_like(fr), np.ones_like(fr), fr - np.uint64(1), fr, top - np.uint64(1), np.minimum(top - np.uint64(1), np.uint64(2 ** 31 - 1))]
    xs += [rng.integers(0, top) for _ in range(64)]
    for x in xs:
        x = x.astype(np.uint64)
        assert (x < top).all() and (x < 2 ** 31).all()
        want = ((x // fr) << np.uint64(16)) + x % fr + lo.astype(np.uint64)
        got = M.record_step(x, rec)
        bad = np.flatnonzero(got != want)
        # fr = 1, x = 0: the one pair outside the form's domain (the module's docstring)
        assert bad.size == 0 or (bad.tolist() == [0] and int(x[0]) == 0 and int(got[0]) == int(want[0]) + 65535), (bad[:4], x[bad[:4]])
    assert (M.record_step(np.ones(1, np.uint64), M.record(np.array([7]), np.array([1]))) == 65536 + 7).all()
