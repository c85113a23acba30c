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
addresses to the GPU module."""
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
}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def _stream(name):
    return M.stream(_oracle(), name)


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
        return M.front(_stream(name)[0], lead, mut) != _front(name, lead)[0]

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
