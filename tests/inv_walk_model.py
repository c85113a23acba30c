"""Plain-Python restatement of the inverse BWT of jampack_amd/csrc/bwt_inv.hip: hashed splitters, the per-lane walk into 256-byte scratch
slots, the ranking of the slots by pointer jumping, the copy-out, the head check.  No GPU and nothing of jampack_amd: it works from a BWT
image alone (n sorted bytes, the raw tail of len % 120 bytes, the 480-byte trailer), and the crafted images of test_inv_walk_model.py and
test_gpu_inv_walk.py are built here (text + seed or text + named edit; the forward transform is the oracle's).

The scheme.  cum[] and nxt[] (the reference's Map minus one) come from a stable counting sort done tile by tile as k_hist / the scan /
k_build_nxt do it, with the batch form's pos_base added by the shared scan and taken off again in 32-bit arithmetic.  nxt takes every value
of -1 .. n-1 but j0 = I - 1 exactly once, WHATEVER the image holds: the chain structure of any image, corrupt or not, is one path from the
head j0 to the position whose nxt is -1, plus cycles.  The image is valid when the path covers all n positions.  One lane per 64 positions
of F-space starts at its hashed splitter (splitter_of), lane nsplit at the head; each walks to the next splitter, turns every position into
its symbol (a 4096-entry table over position >> lut_shift, then `while (cum[c + 1] <= j) c++`), packs 16 symbols into four registers and
flushes them as one 16-byte store; a sub-list of more than CAP = 256 bytes goes on in an overflow slot.  The slots are ranked by
jpk_bits_for(max_slots) + 1 rounds of pointer jumping between two buffer pairs (32-bit wrapping adds), every slot is copied to
T[n - dist ..], and the head's distance must be n.

Overflow slot numbers.  The kernel takes them from an atomicAdd, i.e. in an order that the hardware decides.  walk() takes them in the
order in which it visits the lanes (`lane_order`: "up", "down" or a seed) and the tests assert that text and verdict do not depend on it.

Invariants, asserted while it walks (Invariant is raised where the kernel would leave its buffers or rely on something false):
  * every index into scratch, slot_len / slot_next, dist / link, lut, cum, nxt and T is in range, every value read has been written, a
    flush is 16-byte aligned and stays inside its own slot;
  * every F-position is visited by at most one lane; the build writes every nxt entry exactly once;
  * novf <= n / CAP;
  * the table alone names the symbol when lut_shift == 0;
  * on a valid image the head's distance is n and the slots' [n - dist, n - dist + len) are pairwise disjoint and cover T.

What the model shows about the two corrupt-input guards of k_walk: a lane visits each position at most once and no two lanes visit the same
one -- the head has no predecessor, every other start is a splitter, and a walk ends in front of the next splitter -- so a lane makes at most
n - 1 steps (`++steps > n` never fires), and every overflow slot follows CAP positions of its own plus one more, so novf * CAP + 1 <= n and
nsplit + 1 + novf < max_slots (`ns >= max_slots` never fires).  Both need a Map that is not a permutation, which no image gives: walk()
counts them as the events guard-steps and guard-slots and the tests assert that no valid or corrupt image reaches them.  (The mutant
map-i-le-I has such a Map; there the model stops earlier, at the second visit of a position.)  Both stay in the kernel.

The symbol table: the binary search leaves the largest c with cum[c] <= q << lut_shift, so with lut_shift == 0 the `while` never runs, on a
one-symbol text either; it runs for positions that share a table cell with a bucket edge, and skips 254 empty buckets at once when the
alphabet is {0, 255} and lut_shift >= 1."""
import functools
import os
import sys
from collections import Counter

import numpy as np

# ---- constants of bwt_inv.hip, by the names the kernels give them -------------------------------------------------------------------
TB = 256
ITEMS = 32
TILE = TB * ITEMS          # bytes per tile of the Map build
STRIDE = 64                # one splitter per 64 positions of F-space
CAP = 256                  # scratch bytes per slot
LUT = 4096
NIL = 0xFFFFFFFF
UNITS = 120                # JPK_BWT_UNITS: sorted lengths are multiples of it
TRAILER = 480
E_CORRUPT = -3             # JPK_E_CORRUPT
M32 = 0xFFFFFFFF

EVENTS = (
    "last-splitter-outside", "last-splitter-inside",       # splitter_of(nsplit - 1) >= n / < n
    "head-is-splitter",                                    # j0 = I - 1 is a splitter: its own lane writes an empty slot
    "I-is-1", "I-is-n",
    "len-256", "len-257", "len-512", "len-513",            # a sub-list of exactly that many bytes
    "ovf-chain-3",                                         # a sub-list over 768 bytes: three chained overflow slots
    "len-mod16-0", "len-mod16-nonzero", "len-1",           # a lane stops without / with a partial flush; a one-byte sub-list
    "lut-shift-0", "lut-shift-1", "lut-shift-2", "lut-shift-3", "lut-shift-4",
    "tiles-1", "tiles-2", "tiles-3", "tiles-8",
    "empty-buckets-skipped>=200",                          # one lookup's `while` skips that many buckets
    "slots-pow2-below", "slots-pow2-at", "slots-pow2-above",   # nsplit + 1 + novf against the largest power of two <= max_slots
    "raw-tail",
    # corrupt images
    "short-head",                                          # the head path covers fewer than n positions
    "blind-cycle",                                         # a cycle without a splitter: never walked
    "self-link",                                           # a cycle with one splitter, <= CAP bytes: slot_next[s] == s
    "self-link-overflow",                                  # a cycle with one splitter, > CAP bytes: an overflow slot links to its owner
    "multi-splitter-cycle",
    "index-0", "index-beyond", "index-valid-but-wrong",
    # the corrupt-input guards of k_walk
    "guard-steps", "guard-slots",
)
UNREACHABLE = {
    "guard-steps": "nxt is a permutation of -1 .. n-1 without j0: no lane visits a position twice, so steps <= n - 1",
    "guard-slots": "an overflow slot follows CAP positions of its lane alone and one more: novf <= (n - 1) / CAP < max_slots - nsplit - 1",
}

# name -> what the switch changes.  Parameters of walk() and of nothing else.
MUTANTS = {
    "overflow-before-stop": "the overflow test of k_walk runs before the stop test",
    "head-splitter-not-skipped": "the lane of a splitter that is the head walks too",
    "map-i-le-I": "nxt = i - 1 for i <= I instead of i < I",
    "flush-offset+16": "the partial flush goes to (len & ~15) + 16",
    "flush-offset-16": "the partial flush goes to (len & ~15) - 16",
    "no-partial-flush": "no flush of the last len & 15 bytes",
    "lut-no-skip": "the table's symbol is taken as it is, no `while (cum[c + 1] <= j) c++`",
    "splitter-of-no-hash": "splitter_of(k) = k * STRIDE, is_splitter as it is",
    "is-splitter-no-hash": "is_splitter(j) = (j % STRIDE == 0), splitter_of as it is",
    "two-rounds-fewer": "jpk_bits_for(max_slots) - 1 rounds of pointer jumping",
    "copy-d-le-len": "copy-out leaves a slot with d <= len instead of d < len",
    "copy-no-d-gt-n": "copy-out without the d > n test",
    "largest-c-strict": "the table search keeps cum[mid] < pos instead of <= (no byte changes: the `while` makes up for it, and runs at lut_shift 0)",
    # cannot change a byte or a verdict: EQUIVALENT
    "one-round-fewer": "jpk_bits_for(max_slots) rounds of pointer jumping",
}
EQUIVALENT = {
    "one-round-fewer": "r rounds cover chains of 2^r slots; a chain has at most max_slots < 2^jpk_bits_for(max_slots) slots, so the last "
                       "round finds every link NIL already (two-rounds-fewer is caught).  For the same reason no image can tell the buffer pair "
                       "the batch form reads at the end, rounds & 1, from the other one, which is one round behind",
}

class Invariant(AssertionError):
    """walk() met a state the kernels must never be in"""


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def splitter_of(k):
    return k * STRIDE + (mix32(k) & (STRIDE - 1))


def is_splitter(j):
    return (j & (STRIDE - 1)) == (mix32(j // STRIDE) & (STRIDE - 1))


def bits_for(v):
    """jpk_bits_for"""
    return int(v).bit_length()


def layout(n):
    """what inv_layout and the enqueue compute from n"""
    ntiles = (n + TILE - 1) // TILE
    nsplit = (n + STRIDE - 1) // STRIDE
    max_slots = nsplit + 1 + n // CAP + 2
    lut_shift = 0
    while ((n - 1) >> lut_shift) >= LUT:
        lut_shift += 1
    return dict(ntiles=ntiles, nsplit=nsplit, max_slots=max_slots, lut_shift=lut_shift, rounds=bits_for(max_slots) + 1)


def parse(image):
    """(bytes as an array, len, n, trailer index)"""
    a = np.frombuffer(bytes(image), dtype=np.uint8)
    ln = len(a) - TRAILER
    if ln < UNITS:
        raise ValueError("fewer than 120 sorted bytes: not the inverse BWT's kernels")
    n = ln - ln % UNITS
    return a, ln, n, int.from_bytes(a[ln: ln + 4].tobytes(), "little")


def _idx(what, i, size):
    if not 0 <= i < size:
        raise Invariant(f"{what}[{i}] of {size}")


def build_map(B, n, I, pos_base=0, mutant=None):
    """(cum[257], nxt[n]) as k_hist, the exclusive scan over the (symbol, tile) table, k_cum and k_build_nxt make them"""
    ntiles = (n + TILE - 1) // TILE
    hist = np.zeros((256, ntiles), dtype=np.int64)
    for bx in range(ntiles):
        hist[:, bx] = np.bincount(B[bx * TILE: min(n, (bx + 1) * TILE)], minlength=256)
    flat = hist.reshape(-1)
    tileoff = (((np.cumsum(flat) - flat) + pos_base) & M32).reshape(256, ntiles)      # what the shared scan leaves: pos_base in front
    cum = [int((tileoff[c, 0] - pos_base) & M32) for c in range(256)] + [n]
    nxt = np.full(n, -2, dtype=np.int64)
    for bx in range(ntiles):
        seg = B[bx * TILE: min(n, (bx + 1) * TILE)]
        order = np.argsort(seg, kind="stable")                       # within the tile: by symbol, then by position (cnt[w][d] + rnk)
        sym = seg[order].astype(np.int64)
        first = np.cumsum(hist[:, bx]) - hist[:, bx]
        dst = ((tileoff[sym, bx] - pos_base) & M32) + (np.arange(len(seg)) - first[sym])
        if len(dst) and (dst.min() < 0 or dst.max() >= n):
            raise Invariant(f"build: nxt[{int(dst.min())} .. {int(dst.max())}] of {n}")
        if np.any(nxt[dst] != -2):
            raise Invariant("build: an nxt entry is written twice")
        i = order + bx * TILE
        keep = (i <= I) if mutant == "map-i-le-I" else (i < I)
        nxt[dst] = np.where(keep, i - 1, i)
    if np.any(nxt == -2):
        raise Invariant("build: an nxt entry is never written")
    return cum, nxt.tolist()


def _splitter_flags(n, mutant):
    j = np.arange(n, dtype=np.uint64)
    if mutant == "is-splitter-no-hash":
        return ((j & 63) == 0).tolist()
    x = j >> np.uint64(6)
    m = np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return ((j & np.uint64(63)) == (x & np.uint64(63))).tolist()


class Result(dict):
    """status, I, novf, head_dist (the verdict), text (bytes, or None where status != 0), events (Counter), sub (the sub-lists' lengths),
    slot_len / slot_next, owner (overflow slot -> its lane), nslots, layout"""
    __getattr__ = dict.__getitem__

    def verdict(self):
        return {k: self[k] for k in ("status", "I", "novf", "head_dist")}


def walk(image, mutant=None, lane_order="up", extra_rounds=0, pos_base=0):
    """the kernels of one inverse BWT on one image -> Result.  lane_order: the order in which the lanes of k_walk run ("up", "down" or a
    seed).  extra_rounds: the batch form runs as many rounds as its largest job needs.  pos_base: the batch form's offset."""
    assert mutant is None or mutant in MUTANTS, mutant
    a, ln, n, I = parse(image)
    lay = layout(n)
    nsplit, max_slots, lut_shift = lay["nsplit"], lay["max_slots"], lay["lut_shift"]
    ev = Counter()
    ev[f"lut-shift-{lut_shift}"] += 1
    ev[f"tiles-{lay['ntiles']}"] += 1
    ev["last-splitter-outside" if splitter_of(nsplit - 1) >= n else "last-splitter-inside"] += 1
    if ln > n:
        ev["raw-tail"] += 1
    T = bytearray(ln)
    res = Result(status=0, I=I, novf=0, head_dist=0, text=None, events=ev, sub=[], slot_len=None, slot_next=None, nslots=0, layout=lay, n=n)

    # ---- k_inv_prep ----
    if not 1 <= I <= n:
        ev["index-0" if I == 0 else "index-beyond"] += 1
        res.update(status=E_CORRUPT, I=0)                              # every later kernel leaves at once
        return res
    if I == 1:
        ev["I-is-1"] += 1
    if I == n:
        ev["I-is-n"] += 1

    B = a[:n]
    cum, nxt = build_map(B, n, I, pos_base, mutant)

    # ---- the symbol table of k_walk ----
    lut = [0] * LUT
    for q in range(LUT):
        pos = q << lut_shift
        lo, hi = 0, 256
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if (cum[mid] < pos) if mutant == "largest-c-strict" else (cum[mid] <= pos):
                lo = mid
            else:
                hi = mid
        lut[q] = lo

    # ---- k_walk ----
    issp = _splitter_flags(n, mutant)
    j0 = I - 1
    if issp[j0]:
        ev["head-is-splitter"] += 1
    scratch = bytearray(max_slots * CAP)
    written = bytearray(max_slots * CAP)
    slot_len = [None] * max_slots
    slot_next = [None] * max_slots
    visited = bytearray(n)
    novf = 0
    owner = {}                                             # overflow slot -> the lane whose sub-list it continues
    max_skip = 0
    lanes = list(range(nsplit + 1))
    if lane_order == "down":
        lanes.reverse()
    elif lane_order != "up":
        lanes = np.random.default_rng(lane_order).permutation(nsplit + 1).tolist()
    for k in lanes:
        if k == nsplit:
            j = j0
        else:
            j = k * STRIDE if mutant == "splitter-of-no-hash" else splitter_of(k)
            if j >= n or (j == j0 and mutant != "head-splitter-not-skipped"):
                slot_len[k], slot_next[k] = 0, NIL
                continue
        slot, length, steps, total = k, 0, 0, 0
        reg = bytearray(16)
        base = slot * CAP

        def flush(off, slot):
            if off % 16 or off < slot * CAP or off + 16 > (slot + 1) * CAP:
                raise Invariant(f"slot {slot}: a flush at scratch offset {off}")
            _idx("scratch", off + 15, len(scratch))
            scratch[off: off + 16] = reg
            written[off: off + 16] = b"\x01" * 16
            reg[:] = bytes(16)

        while True:
            _idx("nxt", j, n)
            if visited[j]:
                raise Invariant(f"lane {k}: position {j} is visited a second time")
            visited[j] = 1
            _idx("lut", j >> lut_shift, LUT)
            c = lut[j >> lut_shift]
            skip = 0
            if mutant != "lut-no-skip":
                while True:
                    _idx("cum", c + 1, 257)
                    if cum[c + 1] > j:
                        break
                    c += 1
                    skip += 1
            if skip and lut_shift == 0:
                raise Invariant(f"position {j}: the table is exact at lut_shift 0 and the while ran")
            max_skip = max(max_skip, skip)
            reg[length & 15] = c
            length += 1
            total += 1
            if length & 15 == 0:
                flush(base + length - 16, slot)
            nx = nxt[j]
            link, stop = NIL, False
            if nx < 0:
                stop = True
            else:
                steps += 1
                if steps > n:
                    stop = True
                    ev["guard-steps"] += 1
                elif issp[nx]:
                    stop, link = True, nx // STRIDE
            ended = False
            for phase in (("overflow", "stop") if mutant == "overflow-before-stop" else ("stop", "overflow")):
                _idx("slot_len", slot, max_slots)
                if phase == "stop" and stop:
                    if length & 15 and mutant != "no-partial-flush":
                        off = base + (length & ~15)
                        off += 16 if mutant == "flush-offset+16" else -16 if mutant == "flush-offset-16" else 0
                        flush(off, slot)
                    slot_len[slot], slot_next[slot] = length, link
                    ev["len-mod16-nonzero" if length & 15 else "len-mod16-0"] += 1
                    ended = True
                    break
                if phase == "overflow" and length == CAP:
                    ns = nsplit + 1 + novf
                    novf += 1
                    if ns >= max_slots:
                        slot_len[slot], slot_next[slot] = length, NIL
                        ev["guard-slots"] += 1
                        ended = True
                        break
                    slot_len[slot], slot_next[slot] = length, ns
                    owner[ns] = k
                    slot, length = ns, 0
                    base = slot * CAP
            if ended:
                break
            j = nx
        res["sub"].append(total)
    if novf > n // CAP:
        raise Invariant(f"novf {novf} > n / CAP = {n // CAP}")
    for total in res["sub"]:
        for L in (256, 257, 512, 513, 1):
            if total == L:
                ev[f"len-{L}"] += 1
        if total > 3 * CAP:
            ev["ovf-chain-3"] += 1
    if max_skip >= 200:
        ev["empty-buckets-skipped>=200"] += 1
    res["max_skip"] = max_skip

    # ---- k_rank_init, k_rank_jump: two buffer pairs, round r reads pair r & 1 ----
    nslots = min(nsplit + 1 + novf, max_slots)
    pow2 = 1 << (bits_for(max_slots) - 1)
    ev["slots-pow2-below" if nslots < pow2 else "slots-pow2-at" if nslots == pow2 else "slots-pow2-above"] += 1
    dist = [[None] * max_slots, [None] * max_slots]
    link = [[None] * max_slots, [None] * max_slots]
    for s in range(nslots):
        if slot_len[s] is None or slot_next[s] is None:
            raise Invariant(f"slot {s} of {nslots} in use was never written by the walk")
        dist[0][s], link[0][s] = slot_len[s], slot_next[s]
    rounds = lay["rounds"] + extra_rounds - {"one-round-fewer": 1, "two-rounds-fewer": 2}.get(mutant, 0)
    for r in range(rounds):
        di, li, do, lo_ = dist[r & 1], link[r & 1], dist[(r & 1) ^ 1], link[(r & 1) ^ 1]
        for s in range(nslots):
            d, l = di[s], li[s]
            if l != NIL:
                _idx("dist", l, nslots)
                d = (d + di[l]) & M32
                l = li[l]
            do[s], lo_[s] = d, l
    final = dist[rounds & 1]                                           # final_in_b = rounds & 1

    # ---- k_head_check / k_b_finish ----
    _idx("dist", nsplit, nslots)
    head = final[nsplit]
    status = 0
    if head != n or nsplit + 1 + novf > max_slots:
        status = E_CORRUPT

    # ---- k_copy_out ----
    cover = bytearray(n)
    for s in range(nslots):
        length = slot_len[s]
        if length == 0:
            continue
        d = final[s]
        if mutant != "copy-no-d-gt-n" and d > n:
            continue
        if (d <= length) if mutant == "copy-d-le-len" else (d < length):
            continue
        for b in range(length):
            _idx("scratch", s * CAP + b, len(scratch))
            if not written[s * CAP + b]:
                raise Invariant(f"slot {s}: byte {b} of {length} was never flushed")
            _idx("T", n - d + b, n)
            T[n - d + b] = scratch[s * CAP + b]
            cover[n - d + b] = min(cover[n - d + b] + 1, 2)
    T[n:ln] = a[n:ln].tobytes()                                        # k_inv_tail

    res.update(status=status, novf=novf, head_dist=head, nslots=nslots, slot_len=slot_len, slot_next=slot_next, owner=owner)
    if status == 0:
        if mutant is None and (cover.count(1) != n):
            raise Invariant("a valid image's slots do not tile T")
        res["text"] = bytes(T)
    else:
        ev["short-head"] += 1
    if mutant is None:
        _chain_events(res, nxt, issp, j0)
    return res


def _chain_events(res, nxt, issp, j0):
    """the structure of the chain itself -- the head path and the cycles, with their splitters -- checked against what the walk left"""
    n, ev = res["n"], res["events"]
    seen = bytearray(n)
    j, path = j0, 0
    while j >= 0:
        if seen[j]:
            raise Invariant("the head path closes on itself")
        seen[j] = 1
        path += 1
        j = nxt[j]
    if path != res["head_dist"]:
        raise Invariant(f"head distance {res['head_dist']}, the head path has {path} positions")
    if (path == n) != (res["status"] == 0):
        raise Invariant("the verdict is not `the head path covers the block`")
    selfs = 0
    for s in range(n):
        if seen[s]:
            continue
        j, size, sp = s, 0, 0
        while not seen[j]:
            seen[j] = 1
            size += 1
            sp += issp[j]
            j = nxt[j]
        if j != s:
            raise Invariant("a chain that is neither the head path nor a cycle")
        if sp == 0:
            ev["blind-cycle"] += 1
        elif sp == 1:
            ev["self-link" if size <= CAP else "self-link-overflow"] += 1
            selfs += size <= CAP
        else:
            ev["multi-splitter-cycle"] += 1
    got = sum(1 for s in range(res["nslots"]) if res["slot_next"][s] == s)
    if got != selfs:
        raise Invariant(f"{selfs} one-splitter cycles of <= CAP bytes, {got} self-linked slots")
    back = sum(1 for s, k in res["owner"].items() if res["slot_next"][s] == k)
    if back != ev.get("self-link-overflow", 0):
        raise Invariant(f"{ev.get('self-link-overflow', 0)} long one-splitter cycles, {back} overflow slots that link to their owner")


def verdict(image):
    """{status, I, novf, head_dist} of an image, and its text where status == 0"""
    r = walk(image)
    return r.verdict(), r["text"]


# ---- crafted images --------------------------------------------------------------------------------------------------------------------
def text(kind, length, seed):
    rng = np.random.default_rng([seed, length])
    if kind == "rand":
        t = rng.integers(0, 256, length)
    elif kind == "bits":                                   # alphabet {0, 255}: 254 empty buckets between the two
        t = rng.integers(0, 2, length) * 255
    elif kind == "one":                                    # one symbol: I = n, the chain runs down F-space
        t = np.full(length, seed)
    elif kind == "first-min":                              # the whole text is the smallest suffix: I = 1
        t = rng.integers(1, 256, length)
        t[0] = 0
    elif kind == "first-max":                              # ... the largest: I = n
        t = rng.integers(0, 255, length)
        t[0] = 255
    else:
        raise KeyError(kind)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    t.setflags(write=False)
    return t


# name -> (kind, bytes, seed).  The seeds were found once by search on the CPU (seconds); test_inv_walk_model.py pins what each image reaches.
VALID = {
    "rand-120": ("rand", 120, 0),
    "rand-120-len1": ("rand", 120, 33),            # a one-byte sub-list
    "min-120": ("first-min", 120, 1),              # I = 1: the head is position 0, which is splitter_of(0)
    "max-120": ("first-max", 120, 1),              # I = n
    "one-120": ("one", 120, 255),
    "rand-121": ("rand", 121, 2),                  # raw tails of 1 and 119 bytes
    "rand-359": ("rand", 359, 3),
    "rand-240": ("rand", 240, 0),
    "rand-240-head": ("rand", 240, 28),            # the head is a splitter
    "one-240": ("one", 240, 7),
    "bits-240": ("bits", 240, 1),
    "rand-360": ("rand", 360, 0),                  # the last stride's splitter lies at j >= n
    "rand-480": ("rand", 480, 0),
    "rand-600": ("rand", 600, 0),
    "rand-720": ("rand", 720, 0),
    "rand-840": ("rand", 840, 0),
    "rand-960": ("rand", 960, 0),                  # n % 64 == 0; 16 slots in use of 21
    "rand-960-256": ("rand", 960, 271),            # a sub-list of exactly 256 bytes, no overflow slot
    "rand-1080": ("rand", 1080, 0),
    "rand-1320": ("rand", 1320, 0),
    "rand-1920-256": ("rand", 1920, 40),
    "rand-1920-257": ("rand", 1920, 29),           # one of 257: one overflow slot that holds one byte; 32 slots in use
    "rand-2040": ("rand", 2040, 0),
    "rand-4080": ("rand", 4080, 59),               # n - 1 = 4079: the last length with lut_shift 0
    "rand-4200": ("rand", 4200, 36),               # lut_shift 1
    "bits-4200": ("bits", 4200, 1),                # 254 empty buckets skipped in one lookup
    "rand-8160": ("rand", 8160, 63),               # one tile, lut_shift 1
    "rand-8280": ("rand", 8280, 12),               # two tiles, lut_shift 2
    "rand-16320": ("rand", 16320, 0),              # two tiles, lut_shift 2
    "rand-16440-512": ("rand", 16440, 320),        # three tiles, lut_shift 3
    "rand-16440-513": ("rand", 16440, 2369),
    "rand-16440-chain3": ("rand", 16440, 276),     # a sub-list of 833 bytes
    "rand-65520": ("rand", 65520, 191),            # 910 bytes in one sub-list; 1042 slots in use: more than 1024
    "rand-65639": ("rand", 65639, 0),              # the largest: 65 520 + 119
}
# name -> (valid image, edit).  Edits: ("swap", a, b) exchanges two sorted bytes, ("index", v) rewrites trailer[0].
EDITED = {
    "swap-valid": ("rand-240", ("swap", 32, 234)),             # still valid: the image of another text
    "swap-blind": ("rand-240", ("swap", 59, 74)),              # a cycle without a splitter
    "swap-self": ("rand-240", ("swap", 181, 228)),             # a cycle with one splitter
    "swap-multi": ("rand-240", ("swap", 113, 122)),            # a cycle with several
    "swap-self-ovf": ("rand-960", ("swap", 140, 246)),         # a cycle with one splitter, longer than a slot
    "index-0": ("rand-240", ("index", 0)),
    "index-beyond": ("rand-240", ("index", 241)),
    "index-huge": ("rand-960", ("index", 0x80000000)),
    "index-wrong": ("rand-240", ("index", 6)),                 # 1 <= I <= n, not the text's
}
NAMES = tuple(VALID) + tuple(EDITED)


@functools.lru_cache(maxsize=None)
def _oracle():
    try:
        from oracle.pyoracle import Oracle
    except ImportError:                                    # run as a script, outside pytest: the repository root is not on the path
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle.pyoracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def crafted_text(name):
    return text(*VALID[name])


@functools.lru_cache(maxsize=None)
def image(name):
    """the BWT image of a crafted text (the oracle's forward transform), or of one with its named edit"""
    if name in VALID:
        img = _oracle().bwt_forward(crafted_text(name)).copy()
    else:
        base, edit = EDITED[name]
        img = image(base).copy()
        ln = len(img) - TRAILER
        if edit[0] == "swap":
            a, b = edit[1], edit[2]
            img[a], img[b] = img[b], img[a]
        elif edit[0] == "index":
            img[ln: ln + 4] = np.frombuffer(int(edit[1]).to_bytes(4, "little"), dtype=np.uint8)
        else:
            raise KeyError(edit)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def crafted_walk(name, mutant=None, lane_order="up", extra_rounds=0, pos_base=0):
    """walk() of a crafted image, computed once and shared: a Result, or the Invariant's text"""
    try:
        return walk(image(name), mutant, lane_order, extra_rounds, pos_base)
    except Invariant as e:
        return str(e)


def events_of(name):
    """the events of a crafted image: what walk() counts, plus what only the edit knows"""
    r = crafted_walk(name)
    assert not isinstance(r, str), (name, r)
    ev = Counter(r["events"])
    if name in EDITED and EDITED[name][1][0] == "index":
        base, v = crafted_walk(EDITED[name][0]), EDITED[name][1][1]
        if 1 <= v <= r["n"] and v != base["I"]:
            ev["index-valid-but-wrong"] += 1
    return ev


def caught(name, mutant):
    """does the image tell the mutant from the scheme: a tripped invariant, another verdict, another text"""
    good, bad = crafted_walk(name), crafted_walk(name, mutant)
    assert not isinstance(good, str), (name, good)
    return isinstance(bad, str) or bad.verdict() != good.verdict() or bad["text"] != good["text"]
