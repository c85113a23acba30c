"""dec_front_model on the CPU: the restated scheme of the rANS decoder's front (ans_dec*.hip: k_dec_headers, ByteQueue and k_dec_rans, k_dec_rle, the batch
plumbing with k_dec_order) gives the oracle's chunk table, RLE0 symbols, rank arrays and bytes on every crafted stream, every named arm is
reached by the input made for it (REACH, pinned by name and lead), and every one-token change of the scheme changes the output of the input
named in DETECTS or is shown to change none (dec_front_model.EQUIVALENT).  test_oracle_vs_ref.py pins the oracle to the reference build.

The events are conditions on the INPUTS of test_gpu_dec_front.py, not measurements of the kernels: an input builder that loses an arm
fails here, before a GPU test relies on it.  Every chain is decoded by the oracle first: that a concatenation of streams is a stream is
checked, not assumed.

One event is out of reach of any stream the encoder makes and stands in dec_front_model.UNREACHABLE with the argument: a chunk without a
single zero rank (the chunk's first byte always codes as rank 0).  `zeros-512KiB` breaks the 300 000-byte bound the other inputs keep: a
group of 19 digits needs a run of 2^19 - 1 zeros or more, so no shorter chunk has one.

A stream `lead` bytes behind an aligned address has a = (lead + in_off) & 3, so leads 3 and 15 are one case to the model and two
addresses to the GPU module.

The refusal side (the tests at the end; test_gpu_dec_refusals.py is its GPU module): every stream of dec_front_model.REFUSED is refused
by the model for the acceptance test it is named for and for no other (REASON; where the format ties two tests together, both, and the
stream that parts them stands beside it), the C oracle refuses it too, and every neighbour in STILL_ACCEPTED decodes to the oracle's
bytes.  Each acceptance test dropped or moved by one is a mutant of DETECTS like the others -- a mutant under which the model's own
bounds assertion fires counts as detected -- and the EQUIVALENT ones are run on the malformed streams as well.  Three acceptance tests
are out of reach of any stream (nch >= max_chunks, ip > len, sy > 256: UNREACHABLE).  One case could not be had as the issue words it: a
rank that lands at run == olen makes the count olen + 1 as well, so `rle-store-at-olen` names both tests and `rle-count-wraps` is the
stream on which the store guard refuses alone."""
import functools

import numpy as np
import pytest

import dec_front_model as M

NAMES = M.CASES + tuple(M.CHAINS)

# event -> (input, lead) made for the arm
REACH = {
    "hdr-freq-since1": ("freq-straddle", 0), "hdr-freq-since2": ("freq-straddle", 0),
    "hdr-olen-since1": ("hdr-olen-since1", 0), "hdr-olen-since2": ("hdr-olen-since2", 0),
    "hdr-clen-since1": ("hdr-clen-since1", 0), "hdr-clen-since2": ("hdr-clen-since2", 0),
    "hdr-rlen-since1": ("hdr-rlen-since1", 0), "hdr-rlen-since2": ("hdr-rlen-since2", 0),
    "hdr-end-lane63": ("hdr-end-lane63", 0), "hdr-end-lane0": ("hdr-rlen-since2", 0),
    "hdr-surplus-terminators": ("hdr-rlen-since2", 0),          # the header ends on lane 0: every other terminator of the window is payload
    "hdr-5-windows": ("rlen-1", 0), "hdr-more-than-5-windows": ("hdr-olen-since2", 0), "hdr-window-past-len": ("rlen-1", 0),
    "hdr-start-mod4-0": ("rlen-1", 0), "hdr-start-mod4-1": ("chain-digits", 0), "hdr-start-mod4-2": ("chain-digits", 0),
    "hdr-start-mod4-3": ("chain-63", 0),
    "hdr-start-mod64-0": ("rlen-1", 0), "hdr-start-mod64-1": ("chain-70", 0), "hdr-start-mod64-63": ("chain-63", 0),
    "hdr-freq-3-bytes": ("freq-straddle", 0), "hdr-chunk-of-one-byte-275": ("rlen-1", 0), "hdr-chain-over-64": ("chain-70", 0),
    "queue-a0": ("rlen-1", 1), "queue-a1": ("rlen-1", 2), "queue-a2": ("rlen-1", 3), "queue-a3": ("rlen-1", 0),
    "queue-roll-1": ("dense-5000", 0), "queue-roll-2": ("dense-5000", 0),
    "queue-roll-after-4-byte-symbol": ("roll-after-22", 3),
    "queue-tail-partial-dword": ("rlen-1", 0), "queue-dword-past-end": ("rlen-1", 1),
    "queue-payload-ends-at-in-len": ("rlen-1", 0), "queue-taken-equals-clen": ("rlen-1", 0),
    "rlen-1": ("rlen-1", 0), "rlen-2": ("rlen-2", 0), "rlen-3": ("rlen-3", 0), "rlen-63": ("rlen-63", 0), "rlen-64": ("rlen-64", 0),
    "rlen-65": ("rlen-65", 0), "rlen-128": ("rlen-128", 0),
    "rlen-above-64-mod4-1": ("rlen-129", 0), "rlen-above-64-mod4-2": ("rlen-130", 0), "rlen-above-64-mod4-3": ("rlen-131", 0),
    "class-0": ("classes", 0), "class-1": ("classes", 0), "class-2": ("classes", 0), "class-3": ("classes", 0), "class-4": ("classes", 0),
    "class-5": ("classes", 0), "class-6": ("classes", 0), "class-7": ("class7", 0),
    "bytes-01": ("class7", 0), "bytes-10": ("class7", 0), "bytes-11": ("class7", 0), "bytes-02": ("class7", 0), "bytes-20": ("class7", 0),
    "bytes-12": ("class7", 0), "bytes-21": ("class7", 0), "bytes-22": ("class7", 0),
    # rlen-63 and rlen-128 have no symbol of class 6 or 7: every visit with an event due is a rebuild of class 2 or 3
    "slow-due-only": ("rlen-63", 0), "slow-bytes-only": ("rlen-63", 0), "slow-due-and-bytes": ("rlen-128", 0),
    "rebuild-class-2": ("classes", 0), "rebuild-class-3": ("classes", 0), "rebuild-class-4": ("classes", 0), "rebuild-class-5": ("classes", 0),
    "rebuild-class-6": ("classes", 0), "rebuild-class-7": ("class7", 0),
    "lg-0": ("class7", 0), "lg-1": ("class7", 0), "lg-ge-2": ("class7", 0), "lg-5": ("cap", 0),
    "expn-cap": ("cap", 0), "expn-cap-twice": ("cap", 0),
    "class7-reg0": ("class7", 0), "class7-reg1": ("class7", 0), "class7-sym129": ("class7", 0),
    "pair0-high": ("pairs", 0), "pair0-low": ("pairs", 0), "pair1-high": ("pairs", 0), "pair1-low": ("pairs", 0),
    "exp-floor-used": ("cap", 0), "tail-odd": ("rlen-3", 0),
    "rle-group-over-thread-edge": ("digit-groups", 0), "rle-group-over-pass-edge": ("pass-edge", 0),
    "rle-lookahead-over-pass-edge": ("pass-edge", 0), "rle-group-at-chunk-start": ("zero-heavy-6000", 0),
    "rle-group-at-chunk-end": ("digit-groups", 0), "rle-digits-end-then-digits-start": ("chain-digits", 0),
    "rle-group-1-digits": ("rlen-1", 0), "rle-group-2-digits": ("chain-digits", 0), "rle-group-19-digits": ("zeros-512KiB", 0),
    "rle-group-20-digits": ("zeros-1MiB", 0), "rle-store-at-olen-1": ("rlen-2", 0), "rle-pass-with-carry": ("pass-edge", 0),
    "rle-one-zero": ("rlen-65", 0), "rle-only-zeros": ("zeros-1MiB", 0),
}
BATCH_REACH = ("batch-block-offsets-nonzero", "batch-zero-over-dense", "batch-order-not-identity")       # reached by the tests named for them below

# mutant -> (input, lead) whose output it changes: the input made for the arm the mutant sits in
DETECTS = {
    "since-not-carried": ("hdr-clen-since2", 0),
    "leb-off-nlead": ("rlen-128", 0),                       # a count of 128: the first two-byte value
    "end-from-last-terminator": ("rlen-1", 0),              # payload bytes with bit 7 set behind the header, in its last window
    "before-counts-own-lane": ("rlen-1", 0),
    "fsum-vidx-le-256": ("rlen-1", 0),
    "rp-plus-olen": ("chain-digits", 0),                    # a second chunk, and a first one with fewer symbols than bytes
    "skip-not-dropped": ("rlen-1", 0),                      # a = 3
    "roll-at-63": ("dense-5000", 0),
    "no-prefetch": ("dense-5000", 0),
    "tail-dword-zero": ("rlen-1", 0),
    "tail-no-swap": ("rlen-2", 0),
    "renorm-x-single-byte": ("class7", 0), "renorm-x2-single-byte": ("class7", 0),
    "renorm-mantissa-first": ("rlen-63", 0),
    "rem-starts-8": ("rlen-63", 0), "rem-ex1": ("rlen-63", 0),
    "cap-32768": ("cap", 0),
    "remainder-lane0": ("rlen-63", 0),
    "reg2-wrong-lane": ("class7", 0),
    "tgt-swapped": ("rlen-3", 0),
    "gate-x-only": ("rlen-63", 0),
    "rem6-not-reset": ("classes", 0),
    "exp-mix-le": ("rlen-2", 0),
    "seen7-ge": ("class7", 0),
    "gather-stops-at-b0": ("pass-edge", 0),
    "gather-past-chunk-start": ("chain-digits", 0),
    "lookahead-unguarded": ("chain-digits", 0),
    "nb-limit-lower": ("zeros-1MiB", 0),
    "carry-not-added": ("pass-edge", 0),
    # an acceptance test dropped or moved by one: the refused stream it alone refuses, or the accepted neighbour it would refuse
    "no-nlead-limit": ("nlead-6-bytes-in-window@1", 0),
    "no-freq-limit": ("freq-two-of-2^31@1", 0),             # the counts' 32-bit sum is olen again: only the limit refuses
    "no-olen-limit": ("olen-chunk-plus-1@1", 0),
    "olen-ge-chunk": ("freq-equals-chunk", 0),              # a full chunk of 2^20 bytes is valid
    "no-rlen-limit": ("rlen-olen-plus-1@1", 0),
    "no-clen-fit": ("clen-past-len@1", 0),
    "no-clen-min": ("clen-15@1", 0), "clen-lt-15": ("clen-15@1", 0),
    "no-total-check": ("total-olen-minus-1@1", 0),
    "no-states-check": ("rans-last-byte-flipped", 0),
    "no-taken-check": ("rans-taken-over-clen", 0),
    "taken-ge-clen": ("valid-base", 0),                     # a valid chunk takes exactly clen bytes
    "no-nb-limit": ("rle-21-digits-in-the-middle", 0), "nb-limit-21": ("rle-21-digits-in-the-middle", 0),
    "no-store-flag": ("rle-count-wraps", 0),                # the count wraps onto olen: only the refused stores tell
    "run-le-olen": ("rle-store-at-olen", 0),                # the model's bounds assertion fires: dst[olen]
    "no-carry-check": ("rle-short", 0),
}
# mutant -> an (input, lead) that must NOT show it: what the input in DETECTS has and this one lacks is the arm
BLIND = {
    "since-not-carried": ("rlen-1", 0),                     # no value over a window's edge
    "leb-off-nlead": ("rlen-65", 0),                        # one-byte values only
    "rp-plus-olen": ("rlen-65", 0),                         # one chunk
    "skip-not-dropped": ("rlen-1", 1),                      # a = 0
    "roll-at-63": ("rlen-131", 0), "no-prefetch": ("rlen-131", 0),         # a payload inside the first window
    "tail-dword-zero": ("rlen-1", 1),                       # the input ends on a dword's edge
    "tail-no-swap": ("rlen-64", 0), "cap-32768": ("class7", 0), "reg2-wrong-lane": ("pairs", 0), "rem6-not-reset": ("pairs", 0),
    "seen7-ge": ("pairs", 0),
    "gather-stops-at-b0": ("digit-groups", 0),              # more than one pass, but no group over the edge
    "gather-past-chunk-start": ("rlen-65", 0), "lookahead-unguarded": ("rlen-65", 0),
    "nb-limit-lower": ("zeros-512KiB", 0),                  # 19 digits
    "carry-not-added": ("rlen-131", 0),                     # one pass
    "no-nlead-limit": ("since-5-at-window-edge@1", 0),      # the same six bytes over a window's edge: `since` refuses first
    "no-freq-limit": ("freq-chunk-plus-1@1", 0),            # no wrap: total != olen refuses as well
    "no-olen-limit": ("freq-equals-chunk", 0), "no-rlen-limit": ("valid-base", 0), "no-clen-fit": ("valid-base", 0),
    "no-clen-min": ("empty-chunk-alone", 0), "clen-lt-15": ("empty-chunk-alone", 0),           # clen = 16, the least there is
    "olen-ge-chunk": ("olen-chunk-plus-1@1", 0),
    "no-total-check": ("freq-two-moved", 0),                # the sum is right
    "no-states-check": ("rans-taken-over-clen", 0), "no-taken-check": ("rans-last-byte-flipped", 0),
    "taken-ge-clen": ("surplus-payload-1", 0),              # one byte of the payload is never taken
    "no-nb-limit": ("rle-short", 0), "nb-limit-21": ("rle-25-digits", 0),
    "no-store-flag": ("rle-store-at-olen", 0),              # no wrap: the count is olen + 1 and refuses as well
    "run-le-olen": ("rle-short", 0),
    "no-carry-check": ("rle-21-digits-at-end", 0),
}
CRAFTED = tuple(M.REFUSED) + tuple(M.STILL_ACCEPTED)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def _stream(name):
    """(stream, text) of a valid case or chain; (stream, out_cap) of a REFUSED or STILL_ACCEPTED name"""
    return M.crafted(_oracle(), name) if name in CRAFTED else M.stream(_oracle(), name)


@functools.lru_cache(maxsize=None)
def _front(name, lead=0):
    """the model's (result, events) of a stream: computed once, shared, left unchanged"""
    ev = {}
    return M.front(_stream(name)[0], lead, None, ev), ev


def _oracle_walk(o, s):
    """orc_ans_decode's walk over the chunk headers, one LEB value at a time -> ([ChunkInfo], [freq])"""
    b = s.tobytes()
    ip = op = rp = 0
    infos, freqs = [], []
    while ip < len(b):
        v = []
        for _ in range(259):
            x, n = o.leb_decode(b[ip: ip + 5])
            v.append(x)
            ip += n
        olen, clen, rlen = v[256:]
        infos.append(M.ChunkInfo(ip, clen, olen, rlen, 0, op, rp))
        freqs.append(v[:256])
        ip += clen
        op += olen
        rp += rlen
    assert ip == len(b)
    return infos, freqs


def test_the_input_lists_are_the_ones_the_stage_needs(oracle):
    assert len(set(NAMES)) == len(NAMES) and set(n for n, _ in REACH.values()) <= set(NAMES) and set(M.BATCH) <= set(NAMES)
    assert set(REACH) | set(BATCH_REACH) | set(M.UNREACHABLE) == set(M.EVENTS) and len(M.EVENTS) == len(set(M.EVENTS))
    assert not (set(REACH) | set(BATCH_REACH)) & set(M.UNREACHABLE)
    # what small valid streams are known to reach may never be declared out of reach
    kept = [e for e in M.UNREACHABLE if e.startswith(("bytes-", "expn-cap", "lg-", "class7-", "rle-group-20"))]
    assert not kept and all(len(why) > 40 for why in M.UNREACHABLE.values())
    sizes = {n: len(M.case(n)) for n in M.CASES}
    assert sizes["zeros-1MiB"] == M.CHUNK and sizes["zeros-512KiB"] == M.CHUNK // 2
    assert max(v for n, v in sizes.items() if not n.startswith("zeros-")) <= 300_000 and sizes["class7"] == sizes["classes"] == 20_000
    assert sizes["cap"] == 282_011 and all(sizes[f"hdr-{v}"] == 20_000 for v in M.HDR_EDGE.values())
    for b, what in M.HDR_EDGE.items():
        # the histogram fixes the header: 256 + b frequency bytes, three 3-byte length fields
        f = np.bincount(M.case(f"hdr-{what}"), minlength=256)
        assert int((f >= 127).sum()) == b and f.max() < 16510 and sum(len(oracle.leb_encode(int(x))) for x in f) == 256 + b
    assert len(M.CHAINS["chain-70"]) == 70 and len(M.BIG_CHAIN) == 1100 and len(_stream("chain-63")[0]) - 275 == 319 and 319 % 64 == 63
    r, _ = oracle.rank_encode(M.part("@ends-in-digits"))
    assert r[-1] == 0 and oracle.rank_encode(M.part("@starts-with-digits"))[0][0] == 0
    r, _ = oracle.rank_encode(M.case("zeros-1MiB"))
    assert not r.any() and oracle.rle_encode(r).tolist() == [0] * 19 + [1]
    assert oracle.rle_encode(oracle.rank_encode(M.case("zeros-512KiB"))[0]).tolist() == [0] * 18 + [1]


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle(oracle, name):
    s, t = _stream(name)
    assert np.array_equal(oracle.ans_decode(s, len(t)), t), f"{name}: not a valid stream of its text"
    (status, infos, freqs, totals, syms, ranks, bits), ev = _front(name)
    want_infos, want_freqs = _oracle_walk(oracle, s)
    assert status == M.OK and bits == 0 and infos == want_infos and freqs == want_freqs, name
    assert totals == (len(t), sum(ci.rlen for ci in infos))
    assert len(infos) == (len(M.CHAINS[name]) if name in M.CHAINS else 1)
    for ci, f, r in zip(infos, freqs, ranks):
        want = oracle.rans_decode_chunk(s[ci.in_off: ci.in_off + ci.clen], ci.rlen)
        got = np.array(syms[ci.rle_off: ci.rle_off + ci.rlen], dtype=np.uint16)
        assert np.array_equal(got, want), f"{name} chunk at {ci.in_off}: first difference at symbol {np.flatnonzero(got != want)[:4].tolist()}"
        want_r = oracle.rle_decode(want, ci.olen)
        assert r == want_r.tobytes(), f"{name} chunk at {ci.in_off}: rank arrays differ"
        assert oracle.rank_decode(want_r, np.array(f, dtype=np.int32)).tobytes() == t[ci.out_off: ci.out_off + ci.olen].tobytes()
    assert not [e for e in M.UNREACHABLE if ev.get(e)], "an event declared out of reach was logged"
    print(name, len(t), "->", len(s), "bytes,", len(infos), "chunks,", {e: v for e, v in ev.items() if REACH.get(e, ("",))[0] == name})


@pytest.mark.parametrize("name", NAMES)
def test_decode_equals_oracle_at_exact_capacity(oracle, name):
    s, t = _stream(name)
    assert M.decode(oracle, [s], [len(t)]) == [(M.OK, t.tobytes())]
    assert M.decode(oracle, [s], [len(t) - 1]) == [(M.E_CAPACITY, b"")]


@pytest.mark.parametrize("event", sorted(REACH))
def test_every_event_is_reached_by_the_input_made_for_it(event):
    name, lead = REACH[event]
    ev = _front(name, lead)[1]
    assert ev.get(event), f"{event} is not reached by {name} at lead {lead}"
    assert not [e for e in M.UNREACHABLE if ev.get(e)]
    print(event, name, lead, ev[event])


def test_leads_reach_every_alignment_and_both_tail_arms():
    """leads 0..3 give the last chunk's queue a = 0, 1, 2, 3 in some order, and with them an input that ends on a dword's edge once and
    inside a dword three times: the GPU module's leads 0, 1, 2, 3 (and 15, which is 3 again) meet both arms of load() on every input"""
    for name in NAMES:
        s, _ = _stream(name)
        ci = _front(name)[0][1][-1]
        a = [(lead + ci.in_off) & 3 for lead in M.IN_LEADS]
        assert sorted(a[:4]) == [0, 1, 2, 3] and a[4] == a[3]
        assert ci.in_off + ci.clen == len(s)
        assert sorted((len(s) - (ci.in_off - x)) % 4 for x in a[:4]) == [0, 1, 2, 3]
    for lead in range(4):
        ev = _front("rlen-1", lead)[1]
        a = (lead + 259) & 3
        assert ev.get(f"queue-a{a}") == 1 and bool(ev.get("queue-tail-partial-dword")) == ((16 + a) % 4 != 0) and ev.get("queue-dword-past-end")
    for name in ("rlen-63", "rlen-128"):
        assert not [e for e in ("class-6", "class-7") if _front(name)[1].get(e)]
    assert not _front("roll-after-22", 1)[1].get("queue-roll-after-4-byte-symbol") and _front("roll-after-22", 0)[1].get("queue-roll-after-4-byte-symbol")


@pytest.mark.parametrize("mut", [m for m in M.MUTANTS if m not in M.EQUIVALENT and m not in M.BATCH_MUTANTS])
def test_every_mutant_changes_the_named_input(mut):
    assert set(DETECTS) == set(M.MUTANTS) - set(M.EQUIVALENT) - set(M.BATCH_MUTANTS) and set(BLIND) <= set(DETECTS)

    def changed(name, lead):
        try:
            return M.front(_stream(name)[0], lead, mut) != _front(name, lead)[0]
        except AssertionError as e:                          # the model's own bounds assertion: the mutant leaves a buffer
            assert "outside" in str(e), e
            return True

    assert changed(*DETECTS[mut]), f"{mut} changes nothing on {DETECTS[mut]}"
    if mut in BLIND:
        assert not changed(*BLIND[mut]), f"{mut} shows on {BLIND[mut]}, which lacks its arm"


@pytest.mark.parametrize("mut", sorted(M.EQUIVALENT))
def test_equivalent_mutants_change_nothing(mut):
    assert mut in M.MUTANTS and len(M.EQUIVALENT[mut]) > 40, "every entry carries its reason"
    for name in NAMES:
        s, _ = _stream(name)
        status, infos, freqs, totals, syms, ranks, bits = _front(name)[0]
        if mut in M.HDR_MUTANTS:
            assert M.headers(s, 1 << 40, mut) == (status, infos, freqs, totals), name
        elif mut in M.RLE_MUTANTS:
            assert [M.rle(syms, ci, None, mut) for ci in infos] == [(r, 0) for r in ranks], name
        else:
            for lead in ((0,) if len(syms) > 1000 else (0, 1, 2, 3)):
                base = _front(name, lead)[0][4]
                for ci in infos:
                    assert M.rans(s, ci, lead, mut) == (base[ci.rle_off: ci.rle_off + ci.rlen], 0), (name, lead)
    for name in CRAFTED:                                     # malformed input included: the verdict, the chunks listed, every symbol and rank
        assert M.front(_stream(name)[0], 0, mut) == _front(name)[0], name
    if mut == "tile-bound-lt":
        assert {64, 128} <= {ci.rlen for n in ("rlen-64", "rlen-128") for ci in _front(n)[0][1]}      # it ran where the last tile is whole


def test_batch(oracle):
    """BATCH in one call, then reversed on the same arena: a block with every offset non-zero, a zero-heavy block where a dense one's
    ranks stood -- and the clear that makes that harmless"""
    streams = [_stream(n)[0] for n in M.BATCH]
    texts = [_stream(n)[1] for n in M.BATCH]
    want = [(M.OK, t.tobytes()) for t in texts]
    arena, ev1, ev2 = bytearray(), {}, {}
    assert M.decode(oracle, streams, [len(t) for t in texts], [0, 1, 2, 3, 15], None, ev1, arena) == want
    first = bytearray(arena)
    assert M.decode(oracle, streams[::-1], [len(t) for t in texts[::-1]], [15, 3, 2, 1, 0], None, ev2, arena) == want[::-1]
    assert ev1.get("batch-block-offsets-nonzero") and ev2.get("batch-block-offsets-nonzero") and not ev1.get("batch-zero-over-dense")
    assert ev2.get("batch-zero-over-dense", 0) > 1000 and not ev1.get("batch-order-not-identity")
    print({e: (ev1.get(e), ev2.get(e)) for e in BATCH_REACH})
    # without the clear the first call already differs (a fresh arena is not zero), and so does the second on the first one's leavings
    assert M.decode(oracle, streams, [len(t) for t in texts], None, "no-rank-clear") != want
    assert M.decode(oracle, streams[::-1], [len(t) for t in texts[::-1]], None, "no-rank-clear", None, first) != want[::-1]
    # (an equivalent mutant sends valid rank arrays through the model's own rank decoder, the one the mutants' arrays need)
    assert M.decode(oracle, streams, [len(t) for t in texts], None, "gather-limit-22") == want
    # a block that does not fit takes nothing from the others
    caps = [len(t) for t in texts]
    caps[1] -= 1
    got = M.decode(oracle, streams, caps)
    assert got[1] == (M.E_CAPACITY, b"") and got[:1] + got[2:] == want[:1] + want[2:]


def test_big_chain_launch_order(oracle):
    s, t = _stream("big-chain")
    assert np.array_equal(oracle.ans_decode(s, len(t)), t)
    ev = {}
    assert M.decode(oracle, [s], [len(t)], None, None, ev) == [(M.OK, t.tobytes())]
    status, infos, _, _ = M.headers(s, len(t))
    order = M.dec_order(infos)
    assert len(infos) == 1100 and ev.get("batch-order-not-identity") and sorted(order) == list(range(1100))
    rl = [infos[c].rlen >> 8 for c in order]
    assert rl == sorted(rl, reverse=True) and len(set(rl)) >= 2 and max(ci.rlen for ci in infos) > 256 > min(ci.rlen for ci in infos)


def test_host_walk_agrees_with_the_model(oracle):
    """jam.ans_decoded_size is a host walk of its own over the same headers: (bytes, chunks) on every crafted stream"""
    from jampack_amd.api import ans_decoded_size
    for name in NAMES + ("big-chain",):
        s, t = _stream(name)
        status, infos, _, totals = M.headers(s, 1 << 40)
        assert status == M.OK and ans_decoded_size(s) == (totals[0], len(infos)) == (len(t), len(infos)), name


# ---- the refusal side ------------------------------------------------------------------------------------------------------------------------
def _oracle_verdict(oracle, s, cap):
    from oracle.pyoracle import OracleError
    try:
        return oracle.ans_decode(s, cap).tobytes()
    except OracleError:
        return None


def test_the_pieces_rebuild_the_oracles_stream(oracle):
    """leb_encode + model_pairs + rans_encode_pairs give ans_encode's bytes: what the refused streams are built from is the encoder"""
    for t in (M.base_text(), M.side_text(), M.case("rlen-131"), M.case("dense-5000"), M.case("zero-heavy-6000"), M.case("zeros-1MiB")):
        fields, pay, _ = M.chunk_of_text(oracle, t)
        assert b"".join(fields) + pay == oracle.ans_encode(t).tobytes()
    assert M.leb5(1 << 31)[:4] < bytes([0x80] * 4) and oracle.leb_decode(M.leb5(300, 7)) == (300, 5) and oracle.leb_decode(M.leb5(12345678)) == (12345678, 5)
    assert oracle.leb_decode(M.leb5(1 << 31))[0] == -(1 << 31)             # the oracle's int32: a count below zero
    for v in (0, 1, 2, 126, 127, (1 << 20) + 2048):
        assert oracle.rle_encode(np.zeros(v, dtype=np.uint8)).tolist() == M.digits(v)


def test_the_refusal_lists_are_whole():
    fired = {e for why in M.REASON.values() for e in why}
    alone = {why[0] for why in M.REASON.values() if len(why) == 1}
    gone = {e for e in M.UNREACHABLE if e.startswith("refuse-")}
    assert set(M.REASON) == set(M.REFUSED) and not set(M.REFUSED) & set(M.STILL_ACCEPTED)
    assert fired | gone == set(M.REFUSE_EVENTS) and not fired & gone and len(set(M.REFUSE_EVENTS)) == len(M.REFUSE_EVENTS)
    assert alone == fired, f"no stream isolates {sorted(fired - alone)}"
    assert gone == {"refuse-max-chunks", "refuse-ip-past-len", "refuse-rle-symbol-over-256"}
    assert set(M.REFUSAL_MUTANTS) <= set(DETECTS) | set(M.EQUIVALENT) and set(M.REFUSAL_MUTANTS) & set(M.EQUIVALENT) == {"no-since-limit"}
    assert {n for n, _ in list(DETECTS.values()) + list(BLIND.values())} <= set(NAMES) | set(CRAFTED)


@pytest.mark.parametrize("name", list(M.REFUSED))
def test_refused_stream_trips_the_named_test_and_no_other(oracle, name):
    s, cap = _stream(name)
    status, reasons, stage, inputs = M.verdict(s, cap)
    capacity = name.startswith("capacity-")
    assert status == (M.E_CAPACITY if capacity else M.E_CORRUPT), (name, status)
    assert reasons == tuple(sorted(M.REASON[name])), f"{name}: refused by {reasons}, made for {M.REASON[name]}"
    assert stage == ("headers" if set(reasons) <= set(M.HEADER_REFUSALS) else "payload")
    assert _oracle_verdict(oracle, s, cap) is None, f"{name}: the oracle accepts it"
    assert M.decode(oracle, [s], [cap]) == [(status, b"")]
    for lead in M.IN_LEADS[1:]:                              # the verdict does not depend on where the stream lies
        assert M.verdict(s, cap, lead)[:3] == (status, reasons, stage), (name, lead)
    assert len(s) <= 2048 and cap <= M.CHUNK and (cap <= 8192 or name == "rle-count-wraps"), "streams stay small"
    assert bool(inputs.get("rle-count-wraps")) == (name == "rle-count-wraps")
    print(name, len(s), "bytes, capacity", cap, "->", status, reasons, stage)


@pytest.mark.parametrize("name", list(M.STILL_ACCEPTED))
def test_accepted_neighbour_gives_the_oracles_bytes(oracle, name):
    s, cap = _stream(name)
    want = _oracle_verdict(oracle, s, cap)
    assert want is not None and len(want) == cap, f"{name}: the oracle refuses it"
    status, reasons, stage, inputs = M.verdict(s, cap)
    assert (status, reasons, stage) == (M.OK, (), None)
    assert M.decode(oracle, [s], [cap]) == [(M.OK, want)]
    assert bool(inputs.get("hdr-5-byte-value-wraps")) == (name == "olen-5-bytes-wrapped")
    if name.startswith("surplus-payload-"):
        ev = _front(name)[1]
        assert not ev.get("queue-taken-equals-clen") and _front("valid-base")[1].get("queue-taken-equals-clen") == 1
    if name.startswith("empty-chunk-"):
        infos = _front(name)[0][1]
        at = {"alone": 0, "first": 0, "middle": 1, "last": len(infos) - 1}[name[12:]]
        assert infos[at][1:4] == (16, 0, 0) and len(infos) == (1 if name.endswith("alone") else 3)
    if name == "freq-two-moved":
        # inside the scope rank_rows_model draws for arrays that are not an encoder's: its decode() raises Undefined outside it
        import rank_rows_model as R
        r, f = oracle.rank_encode(M.moved_text())
        f[M.MOVED[0]] += 1
        f[M.MOVED[1]] -= 1
        assert R.decode(r.tobytes(), f.tolist()) == want == R.walk(r.tobytes(), f.tolist())[0]
        assert want != M.moved_text().tobytes() and 0 in M.moved_text(), "another text than the valid one; the text holds a zero byte"


def test_what_each_refused_stream_is_made_of(oracle):
    """the properties the builders promise, read back from the streams"""
    fields, pay, f = M.chunk_of_text(oracle, M.base_text())
    hdr = len(b"".join(fields))
    assert hdr == 259 + 2 and [len(x) for x in fields[256:]] == [2, 1, 2]        # 300 and rlen take two bytes each
    s, _ = _stream("since-5-at-window-edge@1")
    assert bytes(s[59:65]) == bytes(5) + b"\x80" and not [b for b in s[:59] if not b & 0x80]
    s, _ = _stream("window-of-64-continuation-bytes@1")
    assert not s[64:128].any() and s[128] == 0x80
    assert len(_stream("cut-at-window-edge@1")[0]) % 64 == 0 and len(_stream("cut-one-byte-past-window-edge@1")[0]) % 64 == 1
    # the isolating case for taken() > clen: A's own bytes are all there, its clen is one short, B's header starts on A's last byte
    s, cap = _stream("rans-taken-over-clen")
    st, infos, _, _ = M.headers(s, cap)
    assert st == M.OK and len(infos) == 2 and infos[0].clen == len(pay) - 1 and infos[1].in_off - 0 > infos[0].in_off + infos[0].clen
    assert bytes(s[:256]) == b"".join(fields[:256]) and bytes(s[infos[0].in_off: infos[0].in_off + len(pay)]) == pay
    ev = {}
    assert M.rans(s, infos[0], 0, None, ev)[1] == 1 and ev.get("refuse-taken-over-clen") and not ev.get("refuse-states")
    assert M.rans(s, infos[1], 0)[1] == 0                   # B is whole
    # the wrap: 2^32 + 2^20 zeros and ranks in all, every separator at or beyond olen
    syms, olen = M._wraps()
    total = sum(1 for x in syms if x > 1) + 2048 * ((1 << 21) - 2) + (1 << 20) + 2048
    assert total == (1 << 32) + (1 << 20) and olen == 1 << 20 and len(syms) == 43028
    # 21 digits over the edge of the first pass
    s, cap = _stream("rle-21-digits-over-pass-edge")
    ci = M.headers(s, cap)[1][0]
    syms = oracle.rans_decode_chunk(s[ci.in_off: ci.in_off + ci.clen], ci.rlen)
    assert ci.rlen == 4091 + 21 + 50 and M.PASS == 4096
    assert syms[4090] > 1 and (syms[4091: 4112] <= 1).all() and syms[4112] > 1


def test_precedence_of_capacity_and_corruption(oracle):
    """the header walk of a whole block ends before any payload is looked at: a block whose second chunk does not fit is E_CAPACITY
    though its first payload is corrupt, and one whose first header is malformed is E_CORRUPT though the capacity is short for the
    rest.  The oracle decodes chunk by chunk and refuses either for its own reason: the kernels are held to the model's status"""
    flipped, _ = _stream("rans-last-byte-flipped")
    side = oracle.ans_encode(M.side_text())
    chain = np.concatenate((flipped, side))
    cap = M.T0_LEN + len(M.side_text())
    assert M.verdict(chain, cap)[:3] == (M.E_CORRUPT, ("refuse-states",), "payload")
    assert M.verdict(chain, cap - 1)[:3] == (M.E_CAPACITY, ("refuse-capacity-at-chunk-2",), "headers")
    assert M.decode(oracle, [chain], [cap - 1]) == [(M.E_CAPACITY, b"")] and _oracle_verdict(oracle, chain, cap - 1) is None
    bad, _ = _stream("total-olen-plus-1@1")
    assert M.verdict(bad, 10)[:3] == (M.E_CORRUPT, ("refuse-total-ne-olen",), "headers") and _oracle_verdict(oracle, bad, 10) is None


def test_refusals_in_a_batch(oracle):
    """every refused stream between valid ones in one call: each block has its own status, the valid ones their bytes; the status word of
    a payload-refused block is its own though the launch order of 1100 chains is not the identity"""
    names = [n for pair in zip(M.REFUSED, M.BATCH * 9) for n in pair]
    streams = [_stream(n)[0] for n in names]
    caps = [(_stream(n)[1] if n in CRAFTED else len(_stream(n)[1])) for n in names]
    got = M.decode(oracle, streams, caps, [M.IN_LEADS[i % 5] for i in range(len(names))])
    for n, g, s, cap in zip(names, got, streams, caps):
        assert g == ((M.verdict(s, cap)[0], b"") if n in CRAFTED else (M.OK, _stream(n)[1].tobytes())), n
    big, t = _stream("big-chain")
    two = np.concatenate((oracle.ans_encode(M.side_text()), _stream("rans-last-byte-flipped")[0]))
    ev = {}
    got = M.decode(oracle, [big, two, _stream("rlen-65")[0]], [len(t), len(M.side_text()) + M.T0_LEN, 65], None, None, ev)
    assert [g[0] for g in got] == [0, M.E_CORRUPT, 0] and got[0][1] == t.tobytes() and ev.get("batch-order-not-identity")


def test_host_walk_on_refused_streams(oracle):
    """jam.ans_decoded_size, the host walk behind the sizing of archives: corrupt where the model's header walk says so, the declared
    size where only payload or symbols are bad (the sizing reads no payload) or only the capacity is short (it has none)"""
    import jampack_amd as jam
    from jampack_amd.api import ans_decoded_size
    for name in CRAFTED:
        s, cap = _stream(name)
        status, infos, _, totals = M.headers(s, 1 << 40)
        if status == M.OK:
            assert ans_decoded_size(s) == (totals[0], len(infos)), name
        else:
            with pytest.raises(jam.JampackError) as e:
                ans_decoded_size(s)
            assert e.value.status == M.E_CORRUPT, name
