"""rank_rows_model on the CPU: the codec equals the oracle, walk() -- k_dec_rank's row scheme -- decodes every crafted text, the crafted texts
reach every arm of the scheme (pinned by name), and every switch that changes one token of the scheme is either caught by named texts or
shown to be equivalent.

The events are conditions on the INPUTS of test_gpu_rank_rows.py, not measurements of the kernel: a builder change that loses an arm fails
here.  What hostile arrays (every entry but the buckets' first ones overwritten) add is asserted too: walk() equals the reference on them,
ends, and reaches the two arms no valid stream reaches.  Arrays in which two buckets name the same start position are out of scope
(rank_rows_model's docstring): nothing is asserted about them.

What the model counts per crafted text and which mutants each text catches (`python tests/test_rank_rows_model.py` prints this table):

text            bytes  top-up full/cut  land cur/other  past-known  drops <64/>=64  fast-exit>=64  mutants caught
two-1               1        0/0             0/0               0       1/0                  0    -
two-2               2        0/0             0/0               0       2/0                  0    -
two-63             63        0/0             0/0               0       2/0                  0    -
two-64             64        0/0             0/0               0       2/0                  0    fast-end-late
two-65             65        0/0             0/0               0       2/0                  0    fast-end-late
two-127           127        0/0             0/0               0       2/0                  0    fast-end-late
two-128           128        0/0             0/0               0       2/0                  0    fast-end-late
two-129           129        0/0             0/0               0       2/0                  0    nv2-no-reset, fast-end-late
one-1               1        0/0             0/0               0       1/0                  0    -
one-64             64        0/0             0/0               0       1/0                  0    -
one-65             65        0/0             0/0               1       1/0                  0    nv2-no-reset
one-66             66        0/1             1/0               1       1/0                  0    pcnt-uncut
one-200           200        2/1             3/0               3       1/0                  0    inflight-fast-64, pcnt-uncut, land-off+1
one-5000         5000       77/1            78/0              78       1/0                  0    inflight-fast-64, pcnt-uncut, land-off+1
sizes-shuffled   1203        6/9             2/13              0      16/0                  0    inflight-fast-64, nv2-no-reset, pcnt-uncut, land-off+1, fast-end-late
sizes-sorted     1203        4/8            12/0              14      16/0                  0    norm-le, inflight-fast-64, nv2-no-reset, land-off+1
runs-200        16000      246/5           240/11            240       5/0                  0    unknown-known, inflight-fast-64, pcnt-uncut, land-off+1
runs-1-150       6180       93/5            74/24             74       5/0                  0    unknown-known, inflight-fast-64, pcnt-uncut, land-off+1
rr-64            4497        0/64            1/63              0      64/0                  0    inflight-fast-64, pcnt-uncut, land-off+1
rr-65            4567        0/65            1/64              0      64/1               4437    inflight-fast-64, pcnt-uncut, land-off+1
rr-68            4777        0/68            1/67              0      64/4               4641    inflight-fast-64, pcnt-uncut, land-off+1
rr-69            4847        0/69            1/68              0      64/5               4709    inflight-fast-64, pcnt-uncut, land-off+1
rr-250          17517        0/250           1/249             0      64/186            17017    inflight-fast-64, pcnt-uncut, land-off+1
rr-256          17937        0/256           1/255             0      64/192            17425    pcnt-uncut
ladder          98685     1904/229           1/2132            0      64/192            90181    nv2-no-reset, land-off+1
noise           30000      226/247           0/473             0      64/192            21807    nv2-no-reset, pcnt-uncut, land-off+1
noise-runs      30000      200/249           0/449             4      64/192            10674    norm-le, unknown-known, nv2-no-reset, pcnt-uncut, land-off+1

Equivalent mutants (decode every crafted text; the reasons are rank_rows_model.EQUIVALENT): loaded-gt-init, loaded-gt-general, left-f,
land-nv-exact, slack-64.  stale-twin decodes every valid text and differs from the reference on hostile arrays only (HOSTILE_ONLY): it is
the kernel as it was before these tests.  No valid or hostile array reaches the clip `cnt > rest`."""
import numpy as np
import pytest

import rank_rows_model as M

# event -> crafted texts that must reach it (noise is never the only one)
REACHED_BY = {
    "fast": ["two-64", "two-129", "rr-64", "ladder"],
    "fast-zeros": ["sizes-shuffled", "runs-200", "runs-1-150"],
    "fast-exit-64": ["rr-65", "rr-68", "rr-69", "rr-256", "ladder"],
    "insert<64": ["two-63", "two-64", "rr-64", "sizes-shuffled", "ladder"],
    "insert>=64": ["rr-65", "rr-68", "rr-69", "rr-256", "ladder"],
    "drop<64": ["two-1", "one-1", "sizes-sorted", "rr-64"],
    "drop>=64": ["rr-65", "rr-68", "rr-69", "rr-256", "ladder"],
    "last-drop": list(M.TEXTS),
    "drop-behind-zeros": ["one-64", "one-66", "sizes-sorted", "runs-200"],
    "run-past-known-64": ["one-65", "one-66", "one-5000", "sizes-sorted", "runs-200"],
    "run-past-known-part": ["runs-200", "runs-1-150"],
    "topup-full": ["one-200", "one-5000", "sizes-shuffled", "runs-200", "ladder"],
    "topup-cut": ["one-66", "one-200", "sizes-shuffled", "sizes-sorted", "ladder"],
    "topup-empty-row": ["one-66", "one-5000", "sizes-sorted", "runs-200"],
    "land-current": ["one-66", "sizes-shuffled", "runs-1-150", "ladder"],
    "land-other": ["sizes-shuffled", "runs-200", "rr-64", "ladder"],
    "used-64": ["ladder"],
    "zero-progress": ["ladder"],
    "general-tail": ["two-1", "two-63", "two-64", "one-65", "rr-256", "ladder"],
}
# mutant -> exactly the crafted texts that mis-decode or trip an invariant of walk()
CAUGHT_BY = {
    "norm-le": ["sizes-sorted", "noise-runs"],
    "unknown-known": ["runs-200", "runs-1-150", "noise-runs"],
    "inflight-fast-64": ["one-200", "one-5000", "sizes-shuffled", "sizes-sorted", "runs-200", "runs-1-150", "rr-64", "rr-65", "rr-68", "rr-69",
                         "rr-250"],
    "nv2-no-reset": ["two-129", "one-65", "sizes-shuffled", "sizes-sorted", "ladder", "noise", "noise-runs"],
    "pcnt-uncut": ["one-66", "one-200", "one-5000", "sizes-shuffled", "runs-200", "runs-1-150", "rr-64", "rr-65", "rr-68", "rr-69", "rr-250", "rr-256",
                   "noise", "noise-runs"],
    "land-off+1": ["one-200", "one-5000", "sizes-shuffled", "sizes-sorted", "runs-200", "runs-1-150", "rr-64", "rr-65", "rr-68", "rr-69", "rr-250",
                   "ladder", "noise", "noise-runs"],
    "fast-end-late": ["two-64", "two-65", "two-127", "two-128", "two-129", "sizes-shuffled"],
}
# hostile arrays ("text/kind") on which the kernel's former reading of the twin's counters differs from the reference
STALE_TWIN_DIFFERS = ["ladder/uniform", "ladder/sparse", "ladder/flips", "sizes-shuffled/flips", "runs-1-150/uniform", "runs-1-150/sparse",
                      "rr-69/uniform", "rr-69/sparse", "rr-69/flips"]
HOSTILE = [(name, kind) for name in M.HOSTILE_FROM for kind in M.HOSTILE_KINDS]


def _freq(f):
    return np.array(f, dtype=np.int32)


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.TEXTS)
def test_codec_and_walk_equal_the_oracle(oracle, name):
    t = M.crafted(name)
    R, freq = M.crafted_ranks(name)
    er, ef = oracle.rank_encode(t)
    assert R == er.tobytes() and freq == ef.tolist()
    assert M.decode(R, freq) == t.tobytes() == oracle.rank_decode(er, ef).tobytes()
    ok, ev = M.crafted_walk(name)
    assert ok is True, ev
    print(name, len(t), {k: v for k, v in ev.items() if not isinstance(v, set)})


def test_the_builders_are_what_their_names_say():
    assert len(M.crafted("ladder")) == 98_685 and max(len(M.crafted(n)) for n in M.TEXTS) < 100_000
    assert sorted(np.bincount(M.crafted("sizes-shuffled")).tolist()) == sorted(M.SIZES) == sorted(np.bincount(M.crafted("sizes-sorted")).tolist())
    assert np.count_nonzero(np.diff(M.crafted("sizes-sorted").astype(int))) == len(M.SIZES) - 1               # contiguous
    for n in M.TWO_N:
        assert set(M.crafted_ranks(f"two-{n}")[0][2:]) <= {1} and len(M.crafted(f"two-{n}")) == n
    for n in M.ONE_N:
        assert set(M.crafted_ranks(f"one-{n}")[0]) == {0} and len(M.crafted(f"one-{n}")) == n
    for d in M.RR_D:
        R, freq = M.crafted_ranks(f"rr-{d}")
        starts = np.cumsum([0] + [freq[s] for s in M.sorted_map(freq)])[:-1]
        assert set(np.delete(_u8(R), starts).tolist()) == {d - 1}
    assert all(M.crafted(name)[0] == 0 or 0 in M.crafted(name) for name in M.HOSTILE_FROM)


# ---- event coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_arm_is_reached_by_named_texts():
    assert set(REACHED_BY) | set(M.UNREACHABLE) == set(M.EVENTS) and not set(REACHED_BY) & set(M.UNREACHABLE)
    for event, names in REACHED_BY.items():
        assert names, event
        for name in names:
            assert M.crafted_walk(name)[1].get(event, 0) > 0, (event, name)
    for event, why in M.UNREACHABLE.items():                       # no valid text reaches them, noise included
        assert why
        assert not any(M.crafted_walk(name)[1].get(event) for name in M.TEXTS), event


def test_rank_and_depth_sets():
    ev = M.crafted_walk("ladder")[1]
    assert ev["fast-ranks"] == set(range(1, 256))
    assert ev["drop-depths"] == set(range(1, 256))
    assert {63, 64, 67, 68} <= ev["general-ranks"]
    crafted = [n for n in M.TEXTS if not n.startswith("noise")]
    union = set().union(*(M.crafted_walk(n)[1]["general-ranks"] for n in crafted))
    assert 255 in M.crafted_walk("rr-256")[1]["general-ranks"]          # the last byte of the packed register's lane 47
    for d in M.RR_D:
        assert M.crafted_walk(f"rr-{d}")[1]["general-ranks"] == {d - 1}
    for k in range(48):                                              # every lane of the packed register
        assert union & set(range(64 + 4 * k, 68 + 4 * k)), k
    print("general-path ranks of the crafted texts:", len(union), "missing", sorted(set(range(1, 256)) - union))


def test_the_tail_cannot_reach_the_packed_register():
    """at i >= fast_end at most 63 symbols still occur: inserts up to 61, drops up to 62, in every crafted text"""
    for name in M.TEXTS:
        R, freq = M.crafted_ranks(name)
        log = []
        M.walk(R, freq, None, log)
        fast_end = len(R) - M.TAIL if len(R) >= M.ROW else 0
        assert not [e for at, e in log if at >= fast_end and e in ("insert>=64", "drop>=64", "fast", "fast-zeros")], name


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------
def test_the_mutant_tables_name_every_switch_once():
    assert set(CAUGHT_BY) | set(M.EQUIVALENT) | set(M.HOSTILE_ONLY) == set(M.MUTANTS)
    assert len(CAUGHT_BY) + len(M.EQUIVALENT) + len(M.HOSTILE_ONLY) == len(M.MUTANTS)


@pytest.mark.parametrize("mutant", sorted(CAUGHT_BY))
def test_mutant_is_caught_by_crafted_texts(mutant):
    caught = [name for name in M.TEXTS if M.crafted_walk(name, mutant)[0] is not True]
    assert caught == CAUGHT_BY[mutant]
    assert [n for n in caught if not n.startswith("noise")], "caught by noise alone: craft a text for it"


@pytest.mark.parametrize("mutant", sorted(set(M.EQUIVALENT) | set(M.HOSTILE_ONLY)))
def test_mutant_decodes_every_valid_text(mutant):
    assert (M.EQUIVALENT.get(mutant) or M.HOSTILE_ONLY[mutant])
    for name in M.TEXTS:
        assert M.crafted_walk(name, mutant)[0] is True, name


# ---- hostile arrays -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", HOSTILE)
def test_hostile_arrays(oracle, name, kind):
    """the reference is defined on them (distinct starts, symbol 0 has a bucket); walk() gives its bytes and ends.  All but `zeros` visit an
    exhausted bucket with uniq == 0 -- with every rank zero each bucket is one run and the walk ends on the last drop, like a valid one"""
    R, freq = M.hostile(name, kind)
    exp = M.decode(R, freq)
    assert exp == oracle.rank_decode(_u8(R), _freq(freq)).tobytes()
    T, ev = M.walk(R, freq)
    assert T == exp
    assert not ev.get("clip")
    assert bool(ev.get("uniq-0")) == (kind != "zeros")
    stale, _ = M.walk(R, freq, "stale-twin")
    assert (stale != exp) == (f"{name}/{kind}" in STALE_TWIN_DIFFERS)
    assert bool(ev.get("twin")) >= (stale != exp)
    print(name, kind, {k: v for k, v in ev.items() if not isinstance(v, set)})


def test_duplicate_starts_are_refused_not_judged():
    R, freq = M.crafted_ranks("two-64")
    bad = bytearray(R)
    bad[32] = bad[0]                                                 # the second bucket names the first one's position
    with pytest.raises(M.Undefined):
        M.walk(bytes(bad), freq)
    with pytest.raises(M.Undefined):
        M.decode(bytes(bad), freq)


def _table():
    yield "text            bytes  top-up full/cut  land cur/other  past-known  drops <64/>=64  fast-exit>=64  mutants caught"
    for n in M.TEXTS:
        ev = M.crafted_walk(n)[1]
        mu = [m for m, names in CAUGHT_BY.items() if n in names]
        yield (f"{n:<15}{len(M.crafted(n)):>6}  {ev.get('topup-full', 0):>7}/{ev.get('topup-cut', 0):<7}  {ev.get('land-current', 0):>6}/"
               f"{ev.get('land-other', 0):<7}  {ev.get('run-past-known-64', 0) + ev.get('run-past-known-part', 0):>8}  {ev.get('drop<64', 0):>6}/"
               f"{ev.get('drop>=64', 0):<7}  {ev.get('fast-exit-64', 0):>11}    {', '.join(mu) or '-'}").rstrip()


def test_the_table_in_the_docstring_is_the_models():
    assert "\n".join(_table()) in __doc__


if __name__ == "__main__":
    print("\n".join(_table()))
