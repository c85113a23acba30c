"""inv_walk_model on the CPU: walk() -- the inverse BWT's splitter walk, slot ranking and copy-out as bwt_inv.hip does them -- gives the
oracle's text on every valid crafted image and the oracle's refusal on every corrupt one, the crafted images reach every case of the scheme
(pinned by name), and every switch that changes one token of the scheme is either caught by named images or shown to be equivalent.

The events are conditions on the INPUTS of test_gpu_inv_walk.py, not measurements of the kernels: a builder change that loses a case fails
here.  The model's bounds assertions hold on every image, the corrupt ones included: that is the evidence, gathered before any of them is
given to the device, that no access of the kernels leaves its buffer on them.

What the model counts per image, and the mutants each image tells from the scheme (`python tests/test_inv_walk_model.py` prints this table).
events: without lut-shift-*, tiles-*, last-splitter-inside and len-mod16-* (the columns in front and nearly every image).  mutants: how
many of the 13 caught ones the image catches, and by name those that fewer than half of the images catch.

image              bytes      I  sub-lists  longest  ovf  shift  tiles  events | mutants
rand-120             120     59          3       81    0      0      1  slots-pow2-below | 6
rand-120-len1        120     39          3       79    0      0      1  len-1, slots-pow2-below | 6
min-120              120      1          2      109    0      0      1  head-is-splitter, I-is-1, slots-pow2-below | 7: head-splitter-not-skipped
max-120              120    120          3       96    0      0      1  I-is-n, slots-pow2-below | 5
one-120              120    120          3       64    0      0      1  I-is-n, len-1, slots-pow2-below | 5
rand-121             121    103          3       82    0      0      1  slots-pow2-below, raw-tail | 6
rand-359             359    178          5       90    0      0      1  slots-pow2-above, raw-tail | 9: two-rounds-fewer
rand-240             240      5          5       80    0      0      1  slots-pow2-above | 9: two-rounds-fewer
rand-240-head        240    222          4       92    0      0      1  head-is-splitter, slots-pow2-above | 9: head-splitter-not-skipped
one-240              240    240          5       92    0      0      1  I-is-n, len-1, slots-pow2-above | 8: two-rounds-fewer
bits-240             240    160          5       94    0      0      1  slots-pow2-above | 9: two-rounds-fewer
rand-360             360    302          6      153    0      0      1  last-splitter-outside, len-1, slots-pow2-below | 8
rand-480             480    286          8      123    0      0      1  last-splitter-outside, slots-pow2-above | 8
rand-600             600    126         10      162    0      0      1  last-splitter-outside, slots-pow2-above | 9: two-rounds-fewer
rand-720             720    264         12      172    0      0      1  last-splitter-outside, slots-pow2-below | 8
rand-840             840    657         14      278    1      0      1  last-splitter-outside, len-1, slots-pow2-at | 8
rand-960             960    720         16      203    0      0      1  slots-pow2-at | 8
rand-960-256         960    862         16      256    0      0      1  len-256, slots-pow2-at | 9: overflow-before-stop
rand-1080           1080    424         18      206    0      0      1  slots-pow2-above | 9: two-rounds-fewer
rand-1320           1320    850         21      153    0      0      1  last-splitter-outside, slots-pow2-above | 9: two-rounds-fewer
rand-1920-256       1920    347         31      256    0      0      1  len-256, len-1, slots-pow2-below | 9: overflow-before-stop
rand-1920-257       1920   1702         31      257    1      0      1  len-257, len-1, slots-pow2-at | 8
rand-2040           2040   1348         33      236    0      0      1  slots-pow2-above | 9: two-rounds-fewer
rand-4080           4080   2915         65      257    1      0      1  len-257, slots-pow2-above | 9: two-rounds-fewer
rand-4200           4200   2178         67      436    2      1      1  len-257, len-1, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
bits-4200           4200   3074         67      241    0      1      1  len-1, empty-buckets-skipped>=200, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
rand-8160           8160   4541        129      263    3      1      1  len-257, len-1, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
rand-8280           8280   6055        130      388    4      2      2  last-splitter-outside, len-257, len-1, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
rand-16320         16320  11822        256      443    5      2      2  len-1, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
rand-16440-512     16440   1116        258      512    4      3      3  len-512, len-1, slots-pow2-above | 10: overflow-before-stop, lut-no-skip, two-rounds-fewer
rand-16440-513     16440  16100        258      577    8      3      3  len-513, len-1, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
rand-16440-chain3  16440  11542        258      833    5      3      3  ovf-chain-3, len-1, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
rand-65520         65520  19297       1025      910   17      4      8  len-257, ovf-chain-3, len-1, slots-pow2-above | 9: lut-no-skip, two-rounds-fewer
rand-65639         65639  26347       1025      373   20      4      8  len-1, slots-pow2-above, raw-tail | 9: lut-no-skip, two-rounds-fewer
swap-valid           240      5          5       80    0      0      1  slots-pow2-above | 9: two-rounds-fewer
swap-blind           240      5          5       80    0      0      1  slots-pow2-above, short-head, blind-cycle | 8: two-rounds-fewer
swap-self            240      5          5       72    0      0      1  slots-pow2-above, short-head, self-link | 8: copy-no-d-gt-n
swap-multi           240      5          5       80    0      0      1  slots-pow2-above, short-head, multi-splitter-cycle | 8: copy-no-d-gt-n
swap-self-ovf        960    720         16      259    1      0      1  slots-pow2-above, short-head, self-link-overflow | 8: copy-no-d-gt-n
index-0              240      0          0        0    0      0      1  index-0 | 0
index-beyond         240      0          0        0    0      0      1  index-beyond | 0
index-huge           960      0          0        0    0      0      1  index-beyond | 0
index-wrong          240      6          5      145    0      0      1  slots-pow2-above, short-head, multi-splitter-cycle, index-valid-but-wrong | 8: copy-no-d-gt-n

Equivalent: one-round-fewer (inv_walk_model.EQUIVALENT: jpk_bits_for(max_slots) rounds already cover a chain of max_slots slots; the round
behind them is slack, two fewer is caught by every image whose head chain is longer than half that power of two).  largest-c-strict changes
no byte of any image -- the `while` behind the table makes up for it -- and is caught only by the model's own statement that the table is
exact at lut_shift 0; images with lut_shift >= 1 cannot tell it from the scheme.
Unreachable: guard-steps (`++steps > n`) and guard-slots (`ns >= max_slots`), by no valid and no corrupt image: the Map of any image is a
permutation (inv_walk_model's docstring has the argument); the model shows it for these images and for 300 random two-byte swaps and index
edits, it does not prove it for all.  A one-symbol text does not reach empty-buckets-skipped: its table is exact, the `while` never runs."""
import numpy as np
import pytest

import inv_walk_model as M
from golden_util import small

LAYOUT_EVENTS = ("last-splitter-inside", "len-mod16-0", "len-mod16-nonzero")

# event -> crafted images that must reach it
REACHED_BY = {
    "last-splitter-outside": ["rand-360", "rand-840", "rand-8280"],
    "last-splitter-inside": ["rand-120", "rand-960", "rand-1920-257", "rand-65520"],
    "head-is-splitter": ["min-120", "rand-240-head"],
    "I-is-1": ["min-120"],
    "I-is-n": ["max-120", "one-120", "one-240"],
    "len-256": ["rand-960-256", "rand-1920-256"],
    "len-257": ["rand-1920-257", "rand-4080", "rand-4200", "rand-8160", "rand-8280", "rand-65520"],
    "len-512": ["rand-16440-512"],
    "len-513": ["rand-16440-513"],
    "ovf-chain-3": ["rand-16440-chain3", "rand-65520"],
    "len-mod16-0": ["rand-120", "rand-960-256", "rand-16440-512"],
    "len-mod16-nonzero": ["rand-120", "min-120", "rand-1920-257", "rand-16440-513"],
    "len-1": ["rand-120-len1", "one-120", "rand-1920-257"],
    "lut-shift-0": ["rand-120", "rand-4080"],
    "lut-shift-1": ["rand-4200", "bits-4200", "rand-8160"],
    "lut-shift-2": ["rand-8280", "rand-16320"],
    "lut-shift-3": ["rand-16440-512", "rand-16440-513", "rand-16440-chain3"],
    "lut-shift-4": ["rand-65520", "rand-65639"],
    "tiles-1": ["rand-120", "rand-8160"],
    "tiles-2": ["rand-8280", "rand-16320"],
    "tiles-3": ["rand-16440-512"],
    "tiles-8": ["rand-65520", "rand-65639"],
    "empty-buckets-skipped>=200": ["bits-4200"],
    "slots-pow2-below": ["rand-120", "rand-1920-256"],
    "slots-pow2-at": ["rand-840", "rand-960", "rand-960-256", "rand-1920-257"],
    "slots-pow2-above": ["rand-240", "rand-4200", "rand-65520"],
    "raw-tail": ["rand-121", "rand-359", "rand-65639"],
    "short-head": ["swap-blind", "swap-self", "swap-multi", "swap-self-ovf", "index-wrong"],
    "blind-cycle": ["swap-blind"],
    "self-link": ["swap-self"],
    "self-link-overflow": ["swap-self-ovf"],
    "multi-splitter-cycle": ["swap-multi", "index-wrong"],
    "index-0": ["index-0"],
    "index-beyond": ["index-beyond", "index-huge"],
    "index-valid-but-wrong": ["index-wrong"],
}
CORRUPT = ("swap-blind", "swap-self", "swap-multi", "swap-self-ovf", "index-0", "index-beyond", "index-huge", "index-wrong")
INDEX_REFUSED = ("index-0", "index-beyond", "index-huge")          # k_inv_prep refuses them: no kernel behind it does anything

# mutant -> exactly the crafted images that tell it from the scheme (another text, another verdict or a tripped invariant), either as
# the images that catch it or as the images that do not
CAUGHT_BY = {
    "overflow-before-stop": ["rand-960-256", "rand-1920-256", "rand-16440-512"],             # sub-lists of 256 and of 512: the verdict's novf
    "head-splitter-not-skipped": ["min-120", "rand-240-head"],
    "lut-no-skip": ["rand-4200", "bits-4200", "rand-8160", "rand-8280", "rand-16320", "rand-16440-512", "rand-16440-513", "rand-16440-chain3",
                    "rand-65520", "rand-65639"],
    "copy-no-d-gt-n": ["swap-self", "swap-multi", "swap-self-ovf", "index-wrong"],            # a copy that would start in front of T
    "two-rounds-fewer": ["rand-359", "rand-240", "one-240", "bits-240", "rand-600", "rand-1080", "rand-1320", "rand-2040", "rand-4080", "rand-4200",
                         "bits-4200", "rand-8160", "rand-8280", "rand-16320", "rand-16440-512", "rand-16440-513", "rand-16440-chain3", "rand-65520",
                         "rand-65639", "swap-valid", "swap-blind"],
}
SMALL_120 = ("rand-120", "rand-120-len1", "min-120", "max-120", "one-120", "rand-121")
MISSED_BY = {
    "map-i-le-I": ("max-120", "one-120", "one-240") + INDEX_REFUSED,                          # I = n: no i with i == I
    "flush-offset+16": INDEX_REFUSED,
    "flush-offset-16": INDEX_REFUSED,
    "no-partial-flush": INDEX_REFUSED,
    "splitter-of-no-hash": SMALL_120 + INDEX_REFUSED,                                         # n = 120: lane 1's 64 is walked over either way
    "is-splitter-no-hash": SMALL_120 + INDEX_REFUSED,
    "copy-d-le-len": CORRUPT,                                                                # they fail either way
    "largest-c-strict": ("rand-4200", "bits-4200", "rand-8160", "rand-8280", "rand-16320", "rand-16440-512", "rand-16440-513",
                         "rand-16440-chain3", "rand-65520", "rand-65639") + INDEX_REFUSED,
}
SELECTIVE = tuple(CAUGHT_BY)


def _expected_catchers(mutant):
    if mutant in CAUGHT_BY:
        return list(CAUGHT_BY[mutant])
    return [n for n in M.NAMES if n not in MISSED_BY[mutant]]


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.VALID))
def test_valid_images_give_the_oracles_text(oracle, name):
    img, t = M.image(name), M.crafted_text(name)
    r = M.crafted_walk(name)
    assert not isinstance(r, str), r
    assert r.status == 0 and r.head_dist == r.n == len(t) - len(t) % 120
    assert r.text == t.tobytes() == oracle.bwt_inverse(img).tobytes()
    v, text = M.verdict(img)
    assert v == r.verdict() and text == r.text
    assert sum(r.sub) == r.n and r.novf == sum((s - 1) // M.CAP for s in r.sub)
    print(name, r.verdict(), dict(r.events))


@pytest.mark.parametrize("name", list(M.EDITED))
def test_edited_images_get_the_oracles_verdict(oracle, name):
    """the still-valid edit is the image of ANOTHER text, which the oracle gives too; the others are refused by both, and the model's
    bounds assertions hold on them"""
    from oracle.pyoracle import OracleError
    img = M.image(name)
    r = M.crafted_walk(name)
    assert not isinstance(r, str), r
    base = M.crafted_walk(M.EDITED[name][0])
    if name in CORRUPT:
        assert r.status == M.E_CORRUPT and r.text is None
        with pytest.raises(OracleError):
            oracle.bwt_inverse(img)
        assert (r.I == 0 and r.head_dist == 0 and r.novf == 0) if name in INDEX_REFUSED else (0 < r.head_dist < r.n)
    else:
        assert name == "swap-valid" and r.status == 0
        assert r.text == oracle.bwt_inverse(img).tobytes() != base.text
    print(name, r.verdict(), dict(r.events))


def test_golden_images(oracle):
    """the stored images of at least 120 sorted bytes (up to 65 536): the model gives the stored text"""
    g = small()
    done = 0
    for key in sorted(g):
        if not key.endswith(".bwt") or len(g[key]) - M.TRAILER < M.UNITS:
            continue
        r = M.walk(g[key])
        assert r.status == 0 and r.text == g[key[:-4] + ".in"].tobytes() == oracle.bwt_inverse(g[key]).tobytes(), key
        done += 1
    assert done >= 8


# ---- event coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_event_is_reached_by_named_images():
    assert set(REACHED_BY) | set(M.UNREACHABLE) == set(M.EVENTS) and not set(REACHED_BY) & set(M.UNREACHABLE)
    for event, names in REACHED_BY.items():
        assert names, event
        for name in names:
            assert M.events_of(name).get(event, 0) > 0, (event, name)
    for event, why in M.UNREACHABLE.items():
        assert why
        assert not any(M.events_of(name).get(event) for name in M.NAMES), event
    assert set(CORRUPT) == {n for n in M.EDITED if M.crafted_walk(n).status != 0}


def test_the_builders_are_what_their_names_say():
    assert max(len(M.image(n)) for n in M.NAMES) == 65_520 + 119 + M.TRAILER
    for name, (kind, length, seed) in M.VALID.items():
        r = M.crafted_walk(name)
        assert len(M.crafted_text(name)) == length and r.n == length - length % 120
    assert set(M.crafted_text("bits-4200").tolist()) == {0, 255} and M.crafted_walk("bits-4200").max_skip >= 254
    assert M.crafted_walk("one-240").max_skip == 0 == M.crafted_walk("one-120").max_skip           # a one-symbol text's table is exact
    assert 256 in M.crafted_walk("rand-960-256").sub and M.crafted_walk("rand-960-256").novf == 0   # exactly a slot: no overflow slot
    r = M.crafted_walk("rand-1920-257")
    assert 257 in r.sub and r.novf == 1 and r.slot_len[r.layout["nsplit"] + 1] == 1                 # the overflow slot holds one byte
    assert max(M.crafted_walk("rand-16440-chain3").sub) == 833 and max(M.crafted_walk("rand-65520").sub) == 910
    assert M.crafted_walk("rand-65520").nslots == 1042 > 1024
    r = M.crafted_walk("swap-self-ovf")
    assert r.novf == 1 and r.slot_next[r.layout["nsplit"] + 1] == M.splitter_of(r.slot_next[r.layout["nsplit"] + 1]) // M.STRIDE
    for n in (960, 1920, 16320):
        assert n % M.STRIDE == 0
    assert [M.layout(n)["lut_shift"] for n in (4080, 4200, 8160, 8280, 16320, 16440, 65520)] == [0, 1, 1, 2, 2, 3, 4]
    assert [M.layout(n)["ntiles"] for n in (8160, 8280, 16320, 16440, 65520)] == [1, 2, 2, 3, 8]


def test_the_hash_is_the_kernels():
    """splitter_of and is_splitter agree, one splitter per stride, and the vectorised flags are the same.  That the hash is the KERNEL's is
    shown on the device: the overflow slots it counts depend on where the splitters lie (test_gpu_inv_walk.py)"""
    assert M.mix32(0) == 0 and M.splitter_of(0) == 0
    for k in range(2048):
        j = M.splitter_of(k)
        assert j // M.STRIDE == k and M.is_splitter(j)
        assert sum(M.is_splitter(k * M.STRIDE + d) for d in range(M.STRIDE)) == 1
    flags = M._splitter_flags(4096, None)
    assert [j for j in range(4096) if flags[j]] == [M.splitter_of(k) for k in range(64)]


def test_overflow_slot_numbers_and_extra_rounds_do_not_matter():
    """the atomicAdd's order, the batch form's longer round count and its pos_base: same text, same verdict"""
    for name in ("rand-4200", "rand-16440-513", "rand-16440-chain3", "swap-self-ovf", "swap-self", "swap-multi", "swap-valid", "rand-1920-257"):
        good = M.crafted_walk(name)
        for kw in (dict(lane_order="down"), dict(lane_order=7), dict(extra_rounds=1), dict(extra_rounds=6), dict(pos_base=0xFFFFF000),
                   dict(pos_base=65_639, extra_rounds=5, lane_order=3)):
            r = M.crafted_walk(name, None, kw.get("lane_order", "up"), kw.get("extra_rounds", 0), kw.get("pos_base", 0))
            assert not isinstance(r, str), (name, kw, r)
            assert r.verdict() == good.verdict() and r.text == good.text, (name, kw)


def test_random_edits_keep_the_invariants(oracle):
    """300 random edits of small images (two-byte swaps, xor of a byte, another index): the model's bounds hold on all of them, neither
    guard is reached, and its verdict is the oracle's"""
    from oracle.pyoracle import OracleError
    rng = np.random.default_rng(11)
    valid = 0
    for k in range(300):
        base = ("rand-240", "rand-960", "bits-240", "rand-1920-257", "one-240", "rand-360")[k % 6]
        img = M.image(base).copy()
        n = M.crafted_walk(base).n
        kind = k % 3
        if kind == 0:
            a, b = rng.integers(0, n, 2)
            img[a], img[b] = img[b], img[a]
        elif kind == 1:
            img[rng.integers(0, n)] ^= 1 << rng.integers(0, 8)
        else:
            ln = len(img) - M.TRAILER
            img[ln: ln + 4] = np.frombuffer(int(rng.integers(0, n + 3)).to_bytes(4, "little"), dtype=np.uint8)
        r = M.walk(img)
        assert not r.events.get("guard-steps") and not r.events.get("guard-slots")
        try:
            exp = oracle.bwt_inverse(img).tobytes()
        except OracleError:
            exp = None
        assert r.text == exp and (r.status == 0) == (exp is not None), (base, k)
        valid += exp is not None
    assert 0 < valid < 300


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------
def test_the_mutant_tables_name_every_switch_once():
    assert set(CAUGHT_BY) | set(MISSED_BY) | set(M.EQUIVALENT) == set(M.MUTANTS)
    assert len(CAUGHT_BY) + len(MISSED_BY) + len(M.EQUIVALENT) == len(M.MUTANTS)
    for names in list(CAUGHT_BY.values()) + list(MISSED_BY.values()):
        assert set(names) <= set(M.NAMES)


@pytest.mark.parametrize("mutant", sorted(set(CAUGHT_BY) | set(MISSED_BY)))
def test_mutant_is_caught_by_named_images(mutant):
    got = [name for name in M.NAMES if M.caught(name, mutant)]
    assert got == _expected_catchers(mutant)
    assert got, mutant


@pytest.mark.parametrize("mutant", sorted(M.EQUIVALENT))
def test_equivalent_mutant_changes_nothing(mutant):
    assert M.EQUIVALENT[mutant]
    assert not [name for name in M.NAMES if M.caught(name, mutant)]


def _table():
    yield "image              bytes      I  sub-lists  longest  ovf  shift  tiles  events | mutants"
    for n in M.NAMES:
        r, ev = M.crafted_walk(n), M.events_of(n)
        named = [e for e in M.EVENTS if ev.get(e) and e not in LAYOUT_EVENTS and not e.startswith(("lut-shift", "tiles-"))]
        mu = [m for m in M.MUTANTS if m not in M.EQUIVALENT and n in _expected_catchers(m)]
        sel = [m for m in mu if m in SELECTIVE]
        yield (f"{n:<18}{len(M.image(n)) - M.TRAILER:>6} {r.I:>6}  {len(r.sub):>9}  {max(r.sub) if r.sub else 0:>7}  {r.novf:>3}  "
               f"{r.layout['lut_shift']:>5}  {r.layout['ntiles']:>5}  {', '.join(named) or '-'} | {len(mu)}{': ' if sel else ''}{', '.join(sel)}").rstrip()


def test_the_table_in_the_docstring_is_the_models():
    assert "\n".join(_table()) in __doc__


if __name__ == "__main__":
    print("\n".join(_table()))
