"""Plain-Python restatement of round 0's finish of the forward BWT's suffix sort (jampack_amd/csrc/bwt_fwd_r0.hip: r0_tile_heads, k_r0_count,
k_r0_scan, k_r0_finish in both forms) and of the run-length kernels behind it (k_run_first, k_run_scan, k_run_fill).  No GPU, no library: the
crafted texts of test_r0_tile_model.py and test_gpu_r0_finish.py are built here, and this model says which slots of the kernels' tiles they
put a head, a singleton or a short suffix on.

Premise: plain byte keys (JPK_KEY_BITS=8, which alone turns the variable-length keys off: var_keys_eligible asks for key_force_bits() == 0), so
round 0 sorts on the first DEPTH = 7 bytes of every suffix, zero padded.  Zero bytes are allowed in the text (sa_window_model forbids them): a
suffix that ties with another only on padding is short, and a short suffix is always a head.

The sorted list.  Slot j of the unsorted list is suffix n-1-j and the LSD sort is stable, so the list is ordered by key, ties by DESCENDING
position.  short[s] = s + 7 > n;  head[j] = j == 0, or the key differs from the slot in front, or either of the two suffixes is short;
survivor[j] = not (head[j] and head[j+1]) with head[n] = True;  the rank of a slot is the index of its group's head;  a run member is a survivor
whose seven key bytes are equal.  survivors() is what the library reports as sa_round_active[1] (SaState::m[1]), large_members() what it
reports as sa_round_large[1]; with no survivor the sort ends after round 0 (sa_rounds == 1).

The kernels cut the list into tiles of CT = 4096 slots, a tile into four waves of 1024 slots, a wave into sixteen rows of 64 (one ballot word).
kind_counts() names where heads, singletons and short suffixes lie against those edges; run_kind_counts() does the same for the run-length
kernels, which cut the TEXT into tiles of 4096 bytes with sixteen consecutive positions per thread.  finish(t, drop=...) and
run_lengths(t, drop=...) are "rule dropped" twins: the same computation with one cross-edge rule left out, so that a CPU test can show that
the crafted text for a kind tells the twin from the rule.

What the model cannot reach, and does not pretend to:
  * Whether the look-back of k_r0_finish really walks a second batch of 64 predecessors depends on timing (a predecessor that has published its
    prefix ends the walk).  The input fixes only that the head lies 65 or more tiles in front.
  * The grid stride of these kernels: the grid is cap_grid(n, CT, 2^20) (4096 workgroups for k_run_*), one workgroup per tile at any size a
    test can afford.
  * wg_scan (k_r0_scan, k_run_scan) gives every thread 32 tiles and a chunk 8192: a text of more than 32 tiles crosses thread segments, more
    than 256 tiles eight of them and more; the second wave starts at 2048 tiles (8 MiB) and the second chunk at 8192 tiles (32 MiB), out of
    a quick test's reach.
  * LHL used where LHW belongs (phase 0 of k_r0_finish) changes nothing: a word without a head so far falls through to the carry either way, so
    there is no twin for it; "lhl-word-only" is the nearest fault that shows.
"""
import functools
import types
from collections import Counter

import numpy as np

import sa_window_model as W

CT = 4096           # slots per tile (bwt_fwd.hpp); bytes per tile of the run-length kernels
WAVE = 1024         # slots of one wave: 16 rows
ROW = 64            # slots of one row: one ballot word
SEG = 16            # consecutive text positions per thread of k_run_fill
LOOK = 64           # predecessors one batch of the look-back reads
DEPTH = W.DEPTH
NONE = 0xFFFFFFFF
REP = 0x01010101010101

KINDS = (
    # n against the tile
    "n-below-one-row", "n-multiple-of-4096", "n-one-past-a-tile", "n-one-short-of-a-tile",
    # heads and carry
    "tile-without-head", "head-on-tile-first-slot", "head-65-or-more-tiles-in-front",
    "group-straddles-tile-edge", "group-straddles-wave-edge", "group-straddles-row-edge",
    "pair-straddles-tile-edge", "pair-straddles-wave-edge", "pair-straddles-row-edge",
    # singletons decided across an edge
    "singleton-on-tile-last-slot", "singleton-on-row-last-lane", "singleton-on-wave-last-slot",
    # short suffixes
    "short-on-row-last-lane", "short-on-wave-last-slot", "short-on-tile-last-slot", "short-on-tile-first-slot", "short-between-two-equal-keys",
    # the list's end
    "last-slot-survives", "no-survivors", "survivors-multiple-of-4096",
)
RUN_KINDS = (
    "run-members-present", "run-crosses-tile-edge", "tile-without-boundary", "tiles-without-boundary-in-a-row", "run-ends-on-tile-last-byte",
    "run-ends-text", "thread-segment-without-boundary", "more-than-256-tiles",
)
# the twins: rule dropped -> (the kind whose text shows it, that text)
DROPS = {
    "row-short-carry": ("short-on-row-last-lane", "short-row"),          # S >> 63 of the row before is not carried
    "row-key-handoff": ("group-straddles-row-edge", "group-row"),        # readlane 63: the row's last key is not handed on
    "wave-load": ("pair-straddles-wave-edge", "pair-wave"),              # kb, sb: the pair in front of a wave's first slot is ignored
    "wave-short-carry": ("short-on-wave-last-slot", "short-wave"),       # r0_short(sb ...) is not applied
    "tile-short-carry": ("short-on-tile-last-slot", "short-tile"),       # ... at a tile's first slot
    "short-shift": ("short-between-two-equal-keys", "zeros-tail"),       # S << 1: "the suffix in front of me is short" is dropped everywhere
    "he64-as-1": ("pair-straddles-tile-edge", "pair-tile"),              # HE[64]: the next tile's first slot is taken as a head
    "he64-as-0": ("singleton-on-tile-last-slot", "rand256-8192"),        # ... as no head
    "carry-nearest-tile": ("tile-without-head", "long-run"),             # the carry comes from the tile in front only
    "carry-one-batch": ("head-65-or-more-tiles-in-front", "long-run"),   # ... from one batch of 64 predecessors only (max and sum)
    "lhl-word-only": ("group-straddles-row-edge", "group-row"),          # LHL without its running max: own word and the one in front
}
RUN_DROPS = {
    "tafter-ignored": ("run-crosses-tile-edge", "runs-3tiles"),
    "tafter-nearest-tile": ("tiles-without-boundary-in-a-row", "long-run"),
    "next-segment-only": ("thread-segment-without-boundary", "runs-3tiles"),     # the threads behind me: the next one only, no min-scan
}


# ---- the sorted list and round 0's finish ----------------------------------------------------------------------------------------------
def sorted_list(t):
    """(sa, key): slot j of the sorted list holds suffix sa[j], key[j] is its zero-padded 7-byte key"""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    n = len(t)
    pad = np.concatenate((t, np.zeros(DEPTH, dtype=np.uint8)))
    key = np.zeros(n, dtype=np.uint64)
    for k in range(DEPTH):
        key = (key << np.uint64(8)) | pad[k: k + n].astype(np.uint64)
    order = np.lexsort((-np.arange(n, dtype=np.int64), key))
    return order.astype(np.int64), key[order]


def _by_tile(a, fill):
    """a padded with `fill` to whole tiles, one row per tile"""
    nt = -(-len(a) // CT)
    out = np.full(nt * CT, fill, dtype=a.dtype)
    out[: len(a)] = a
    return out.reshape(nt, CT)


def finish(t, drop=None):
    """Round 0's finish of text t: n, sa, key, short, head, survivor, rank (per slot; -1: no head found), run (per slot), starts / sizes of the
    groups, survivors (the total the last tile leaves in the state).  drop: one of DROPS, the same with that rule left out."""
    assert drop is None or drop in DROPS, drop
    sa, key = sorted_list(t)
    n = len(sa)
    j = np.arange(n, dtype=np.int64)
    short = sa + DEPTH > n
    row0 = (j % ROW == 0) & (j > 0) & (j % WAVE != 0)
    wave0 = (j % WAVE == 0) & (j > 0)
    tile0 = (j % CT == 0) & (j > 0)
    differs = np.ones(n, dtype=bool)
    differs[1:] = key[1:] != key[:-1]
    front_short = np.zeros(n, dtype=bool)
    front_short[1:] = short[:-1]
    if drop == "row-short-carry":
        front_short[row0] = False
    if drop == "row-key-handoff":               # the key in front of the wave stays in the register
        differs[row0] = key[row0] != key[np.maximum(j[row0] // WAVE * WAVE - 1, 0)]
    if drop == "wave-load":                     # nothing loaded: a zero key, not short
        differs[wave0] = key[wave0] != 0
        front_short[wave0] = False
    if drop == "wave-short-carry":
        front_short[wave0 & ~tile0] = False
    if drop == "tile-short-carry":
        front_short[tile0] = False
    if drop == "short-shift":
        front_short[:] = False
    head = differs | short | front_short
    head[0] = True
    nexth = np.concatenate((head[1:], [True]))
    tile_last = (j % CT == CT - 1) & (j + 1 < n)
    if drop == "he64-as-1":
        nexth[tile_last] = True
    if drop == "he64-as-0":
        nexth[tile_last] = False
    survivor = ~(head & nexth)
    # ranks the way the tiles find them: the last head inside the tile, or the carry (1 + the last head in front of the tile)
    hidx = _by_tile(np.where(head, j, -1), -1)
    local = np.maximum.accumulate(hidx, axis=1)
    nt = len(local)
    last = local[:, -1] + 1                                             # 1 + last head of the tile, 0: none
    if drop == "lhl-word-only":
        words = hidx.reshape(nt, CT // ROW, ROW)
        inword = np.maximum.accumulate(words, axis=2)
        before = np.concatenate((np.full((nt, 1), -1, dtype=np.int64), inword[:, :-1, -1]), axis=1)
        local = np.where(inword >= 0, inword, before[:, :, None]).reshape(nt, CT)
    tile_surv = _by_tile(survivor, False).sum(axis=1)
    if drop == "carry-nearest-tile":
        carry = np.concatenate(([0], last[:-1]))
        total = int(tile_surv.sum())
    elif drop == "carry-one-batch":
        carry = np.array([last[max(0, k - LOOK): k].max(initial=0) for k in range(nt)], dtype=np.int64)
        total = int(tile_surv[max(0, nt - 1 - LOOK):].sum())
    else:
        carry = np.concatenate(([0], np.maximum.accumulate(last)[:-1]))
        total = int(tile_surv.sum())
    rank = np.where(local >= 0, local, carry[:, None] - 1).reshape(-1)[:n]
    run = survivor & (key == (key >> np.uint64(48)) * np.uint64(REP))
    starts = np.flatnonzero(head)
    sizes = np.diff(np.concatenate((starts, [n])))
    return types.SimpleNamespace(n=n, sa=sa, key=key, short=short, head=head, survivor=survivor, rank=rank, run=run, starts=starts, sizes=sizes,
                                 survivors=total)


def survivors(t):
    """sa_round_active[1]: the suffixes round 0 leaves unresolved"""
    return finish(t).survivors


def large_members(t):
    """sa_round_large[1]: the members of groups above 1024 in the list round 1 starts with (sa_window_model.large_members)"""
    return W.large_members(finish(t).sizes)


def ends_after_round_0(t):
    """no survivor: the library reports sa_rounds == 1"""
    return finish(t).survivors == 0


# ---- slot geometry --------------------------------------------------------------------------------------------------------------------------
def _crossings(a, b, unit):
    """edges at multiples of `unit` between slots a and b (a < b), per element"""
    return b // unit - a // unit


def kind_counts(t, f=None):
    """how often the sorted list of t shows every kind of KINDS"""
    f = f or finish(t)
    n = f.n
    j = np.arange(n, dtype=np.int64)
    c = Counter()
    c["n-below-one-row"] = n < ROW
    c["n-multiple-of-4096"] = n % CT == 0
    c["n-one-past-a-tile"] = n > CT and n % CT == 1
    c["n-one-short-of-a-tile"] = n % CT == CT - 1
    nt = -(-n // CT)
    c["tile-without-head"] = nt - len(np.unique(f.starts // CT))
    first = np.arange(1, nt, dtype=np.int64) * CT
    c["head-on-tile-first-slot"] = f.head[first].sum()
    c["head-65-or-more-tiles-in-front"] = (~f.head[first] & (first // CT - f.rank[first] // CT > LOOK)).sum()
    big = f.sizes >= 2
    gs, gl, two = f.starts[big], f.starts[big] + f.sizes[big] - 1, f.sizes[big] == 2
    tile = _crossings(gs, gl, CT)
    wave = _crossings(gs, gl, WAVE) - tile                              # wave edges that are no tile edges
    row = _crossings(gs, gl, ROW) - tile - wave
    for name, x in (("tile", tile), ("wave", wave), ("row", row)):
        c[f"group-straddles-{name}-edge"] = (x > 0).sum()
        c[f"pair-straddles-{name}-edge"] = ((x > 0) & two).sum()
    inner = j + 1 < n                                                   # behind the last slot lies nothing: a head by definition
    tile_last = (j % CT == CT - 1) & inner
    wave_last = (j % WAVE == WAVE - 1) & (j % CT != CT - 1) & inner
    row_last = (j % ROW == ROW - 1) & (j % WAVE != WAVE - 1) & inner
    single = ~f.survivor
    c["singleton-on-tile-last-slot"] = (single & tile_last).sum()
    c["singleton-on-wave-last-slot"] = (single & wave_last).sum()
    c["singleton-on-row-last-lane"] = (single & row_last).sum()
    c["short-on-tile-last-slot"] = (f.short & tile_last).sum()
    c["short-on-wave-last-slot"] = (f.short & wave_last).sum()
    c["short-on-row-last-lane"] = (f.short & row_last).sum()
    c["short-on-tile-first-slot"] = (f.short & (j % CT == 0) & (j > 0)).sum()
    if n >= 3:
        c["short-between-two-equal-keys"] = (f.short[1:-1] & (f.key[1:-1] == f.key[:-2]) & (f.key[1:-1] == f.key[2:])).sum()
    c["last-slot-survives"] = bool(f.survivor[n - 1])
    c["no-survivors"] = f.survivors == 0
    c["survivors-multiple-of-4096"] = f.survivors > 0 and f.survivors % CT == 0
    return Counter({k: int(v) for k, v in c.items() if v})


# ---- run lengths ------------------------------------------------------------------------------------------------------------------------------
def _boundary(t):
    """run_ends_at: i is the last byte of the text or differs from its successor"""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    return np.concatenate((t[1:] != t[:-1], [True]))


def _next_true(b):
    """per position the first index >= it where b is set (NONE: none)"""
    idx = np.where(b, np.arange(len(b), dtype=np.int64), NONE)
    return np.minimum.accumulate(idx[::-1])[::-1]


def run_lengths(t, drop=None):
    """RL[i] = bytes equal to t[i] from i on -- the reference rule.  drop: one of RUN_DROPS, the tiled computation of k_run_first / k_run_scan /
    k_run_fill with that rule left out (32-bit wrap-around included)."""
    assert drop is None or drop in RUN_DROPS, drop
    b = _boundary(t)
    n = len(b)
    i = np.arange(n, dtype=np.int64)
    if drop is None:
        return _next_true(b) + 1 - i
    bt = _by_tile(b, False)
    nt = len(bt)
    inside = np.stack([_next_true(row) for row in bt]) if drop != "next-segment-only" else None
    first = np.array([np.flatnonzero(row)[0] + k * CT if row.any() else NONE for k, row in enumerate(bt)], dtype=np.int64)
    after = np.full(nt, NONE, dtype=np.int64)                          # exclusive suffix min
    if drop == "tafter-nearest-tile":
        after[:-1] = first[1:]
    elif drop != "tafter-ignored":
        after[:-1] = np.minimum.accumulate(first[::-1])[::-1][1:]
    if drop == "next-segment-only":
        segs = bt.reshape(nt, CT // SEG, SEG)
        own = np.stack([[_next_true(s) for s in tile] for tile in segs])                 # (nt, 256, 16): inside my own sixteen
        own = np.where(own != NONE, own + (np.arange(CT // SEG, dtype=np.int64) * SEG)[None, :, None], NONE)
        nxt = np.concatenate((own[:, 1:, 0], np.full((nt, 1), NONE, dtype=np.int64)), axis=1)
        nb = np.where(own != NONE, own, nxt[:, :, None]).reshape(nt, CT)
    else:
        nb = inside
    base = (np.arange(nt, dtype=np.int64) * CT)[:, None]
    nb = np.where(nb != NONE, nb + base, after[:, None]).reshape(-1)[:n]
    return (nb + 1 - i) & NONE


def run_kind_counts(t, f=None):
    """how often the text shows every kind of RUN_KINDS (a run that counts has DEPTH bytes or more: only those leave run members)"""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    f = f or finish(t)
    n = len(t)
    b = _boundary(t)
    rl = run_lengths(t)
    i = np.arange(n, dtype=np.int64)
    ends = np.flatnonzero(b)
    length = np.diff(np.concatenate(([-1], ends)))                     # of the run that ends at ends[k]
    c = Counter()
    c["run-members-present"] = f.run.sum()
    c["run-crosses-tile-edge"] = (~b & (i % CT == CT - 1)).sum()
    quiet = ~_by_tile(b, False).any(axis=1)
    c["tile-without-boundary"] = quiet.sum()
    c["tiles-without-boundary-in-a-row"] = (quiet[1:] & quiet[:-1]).sum()
    c["run-ends-on-tile-last-byte"] = ((ends % CT == CT - 1) & (ends + 1 < n) & (length >= DEPTH)).sum()
    c["run-ends-text"] = length[-1] >= DEPTH
    c["thread-segment-without-boundary"] = (rl[::SEG] > SEG).sum()     # (segments start at multiples of 16: the tile is one)
    c["more-than-256-tiles"] = -(-n // CT) > 256
    return Counter({k: int(v) for k, v in c.items() if v})


# ---- builders -----------------------------------------------------------------------------------------------------------------------------------
# byte values: filler 1..19 (sorts in front of everything but zeros), stems 20..40 with 20 only as a stem's first byte, the ending's bytes
# 41..49 and 250..254, tail digits 50..249, 0xFF ends a record (sa_window_model's plan)
FILL_HI = 19
ENDING7 = np.array(W.ENDING[-7:], dtype=np.uint8)


def _filled(seed, body, where, target):
    """filler + body, with as many filler bytes (random, 1..19: each adds one suffix in front of everything in body) as bring slot
    where(text) to `target`"""
    fill = np.random.default_rng(seed).integers(1, FILL_HI + 1, 3 * CT).astype(np.uint8)
    need = target - where(body)
    assert 0 <= need <= len(fill), need
    t = np.concatenate((fill[:need], body))
    assert where(t) == target
    return t


def slot_of_suffix(t, s):
    return int(np.flatnonzero(sorted_list(t)[0] == s)[0])


def short_at(seed, slot, copies=2):
    """The text's last suffix, the single byte X = 200, lies on `slot`; `copies` times X + six zeros stand in the text, so the slots behind it
    hold `copies` suffixes whose key equals its padded key: they are a group of their own only because the slot in front is short."""
    rec = [np.array([200, 0, 0, 0, 0, 0, 0, 60 + k], dtype=np.uint8) for k in range(copies)]
    body = np.concatenate(rec + [np.array([150, 151, 152, 153, 154, 155, 200], dtype=np.uint8)])
    return _filled(seed, body, lambda t: slot_of_suffix(t, len(t) - 1), slot)


def group_at(seed, slot, members):
    """`members` copies of one 7-byte stem (first byte 20, below every byte but the filler's) in records of sa_window_model's form; the stem's
    group starts on `slot`"""
    rng = np.random.default_rng(seed)
    stem = np.concatenate((np.array([[20]], dtype=np.uint8), W._chain(rng, 1, DEPTH - 1, 21, W.STEM_HI)), axis=1)
    body = np.concatenate((W._records(rng, stem, [members]).reshape(-1), ENDING7))
    skey = int.from_bytes(bytes(stem[0]), "big")

    def where(t):
        return int(np.flatnonzero(sorted_list(t)[1] == np.uint64(skey))[0])
    return _filled(seed, body, where, slot)


def long_run(seed, fill, length):
    """`fill` filler bytes, one run of `length` bytes 30, the ending: one group of length - 6 run members whose head lies on slot `fill`"""
    rng = np.random.default_rng(seed)
    return np.concatenate((rng.integers(1, FILL_HI + 1, fill).astype(np.uint8), np.full(length, 30, dtype=np.uint8), ENDING7))


def period_2(periods):
    """bytes 30, 31 alternating and the ending: two groups of periods - 3 members each (the six suffixes that reach the ending are alone)"""
    return np.concatenate((np.tile(np.array([30, 31], dtype=np.uint8), periods), ENDING7))


def with_runs(seed, n, runs, lo=1, hi=255):
    """n random bytes of [lo, hi], then the runs: (first position, length, byte); a length that reaches n ends the text inside the run"""
    t = np.random.default_rng(seed).integers(lo, hi + 1, n).astype(np.uint8)
    for p, length, byte in runs:
        t[p: p + length] = byte
        if p:
            t[p - 1] = byte ^ 1 or 2
        if p + length < n:
            t[p + length] = byte ^ 1 or 2
    return t


def _rand(seed, n, values):
    return np.random.default_rng(seed).choice(np.array(values, dtype=np.uint8), n)


TEXTS = (
    "n-50", "abc-4095", "zab-4097", "rand256-8192",
    "short-row", "short-wave", "short-tile", "short-tile-first", "zeros-tail",
    "pair-row", "pair-wave", "pair-tile", "group-row", "group-wave", "group-tile",
    "survivors-4096", "runs-3tiles", "long-run", "tiles-257",
)


@functools.lru_cache(maxsize=None)
def crafted(name):
    """the crafted texts by name (read-only: share, do not change)"""
    t = {
        "n-50": lambda: _rand(1, 50, (0, 1, 2, 3)),
        "abc-4095": lambda: _rand(2, CT - 1, (1, 2, 3)),
        "zab-4097": lambda: _rand(3, CT + 1, (0, 1, 2)),                               # zeros; the second tile holds one slot
        "rand256-8192": lambda: _rand(4, 2 * CT, range(256)),
        "short-row": lambda: short_at(5, ROW - 1),
        "short-wave": lambda: short_at(6, WAVE - 1),
        "short-tile": lambda: short_at(7, CT - 1),
        "short-tile-first": lambda: short_at(8, CT),
        # three zeros end the text and nine stand inside it: suffixes n-1, n-2, n-3 and three run members all have the key 0
        "zeros-tail": lambda: np.concatenate((_rand(9, 150, range(1, 256)), np.zeros(9, dtype=np.uint8), _rand(10, 150, range(1, 256)),
                                              np.zeros(3, dtype=np.uint8))),
        "pair-row": lambda: group_at(11, ROW - 1, 2),
        "pair-wave": lambda: group_at(12, WAVE - 1, 2),
        "pair-tile": lambda: group_at(13, CT - 1, 2),
        "group-row": lambda: group_at(14, 40, 200),                                    # slots 40 .. 239: four rows
        "group-wave": lambda: group_at(15, 1000, 100),
        "group-tile": lambda: group_at(16, 4000, 300),
        "survivors-4096": lambda: period_2(CT // 2 + 3),                                # 2 x 2048 survivors in one tile and a few slots
        # a run over the first tile edge, one that ends on the second tile's last byte, one inside a thread's sixteen, one that ends the text
        "runs-3tiles": lambda: with_runs(18, 3 * CT - 20, ((CT - 30, 70, 77), (2 * CT - 40, 40, 78), (5002, 9, 79), (3 * CT - 60, 40, 80))),
        # the head of the run's group on slot 1000; 67 tiles of run members behind it
        "long-run": lambda: long_run(19, 1000, 67 * CT),
        # 257 tiles and a bit: runs over whole tiles far apart, one of them over the 256th tile's edges
        "tiles-257": lambda: with_runs(20, 257 * CT + 100, ((40 * CT - 10, 3 * CT + 20, 90), (255 * CT - 5, CT + 2000, 91), (100000, 8, 92))),
    }[name]()
    t = np.ascontiguousarray(t, dtype=np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def crafted_finish(name):
    return finish(crafted(name))
