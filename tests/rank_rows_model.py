"""Plain-Python restatement of the sorted-rank codec (rank.cpp:45-151) and of the row scheme by which k_dec_rank (jampack_amd/csrc/ans_dec_rank.hip)
decodes it.  No GPU, no library: the crafted texts of test_rank_rows_model.py and test_gpu_rank_rows.py are built here, and walk() says which
arms of the kernel a rank array reaches.

The codec.  encode(T) -> (R, freq) and decode(R, freq) restate the reference: ranks are move-to-front ranks, stored bucket by bucket in
GenerateSortedMap order (larger frequency first, ties by the smaller symbol); the first entry of a bucket is the symbol's first-appearance
index, i.e. its start position in the decoder's list.  decode() starts from a list of zeros, as the oracle does.  A position that no bucket
names therefore holds a copy of symbol 0; a corrupt array may pull such a copy to the front, and if freq[0] == 0 the reference then reads a
bucket it never set up.  decode() raises Undefined there: hostile arrays are taken from texts that hold a zero byte.

The row scheme.  walk(R, freq) -> (T, events) follows k_dec_rank without lanes: a wave-wide register is a Python list, a ballot is a scan.
Every symbol s owns a row of ROW = 64 entries, filled at the start with the ranks behind its bucket's first entry, 0xFF past the bucket's
end, and four counters (RankMeta): `used` entries consumed by fast iterations since the last normalisation, `fast` entries the fast loop
may consume, `nv` entries known and `left` ranks of the bucket, all three as of the last normalisation.  span[s] = (gpos, gend) is what
has not been requested from R yet.  The fast loop consumes z zero ranks and the non-zero rank behind them while z < fast - used and
i < fast_end = len - TAIL, stores ROW bytes at i, and carries the NEXT symbol's row and counters in registers that were read before its own
counter was written; when the next symbol IS the current one (a corrupt list holds it twice) the kernel lets the loop's next test fail
(fend = 0 for that one test), reads the counters again and goes on, which is what walk() does in place.  Everything else is the general path, in the kernel's order: land the top-up in flight and start over; else scan the
known entries, clip to the bytes left, insert or drop, normalise the row, and issue a top-up of want = ROW - nv2 entries, cut to what the
bucket still has, when fewer than RANK_LOW + TOPUP_MARGIN known entries remain.

What the model found (test_rank_rows_model.py asserts all of it):
  * the clip `cnt > rest` is never taken, by valid or hostile arrays: a visit emits at most left + 1 bytes and sum(left + 1) over the
    symbols is len, and once uniq is 0 a visit emits one byte at a time.  The line stays in the kernel (as the DB=4/5 case did);
  * a general-path iteration at i >= fast_end cannot reach the packed register: at most TAIL symbols still occur, so a front drop is at
    most TAIL - 1 = 62 deep, and an insert's rank -- the number of distinct symbols before the symbol's next occurrence, which lies in the
    chunk -- is at most TAIL - 2 = 61.  Inserts and drops at 64 and deeper come from general iterations in front of fast_end (a row
    that ran low, a run past the known entries) and from the fast loop's exit;
  * equivalent mutants: see EQUIVALENT;
  * the kernel used to keep the counters it had read ahead even when the next symbol was the current one, and then decoded corrupt arrays
    differently from the reference (same bytes twice).  Valid streams never get there: HOSTILE_ONLY, mutant "stale-twin".

Arrays in which two buckets name the same start position are out of scope: the kernel's winner is decided by lane order, the oracle's by
sorted-map order, and such a frame fails its crc either way.  walk() and decode() raise Undefined for them and nothing is asserted.
"""
import functools
from collections import Counter

import numpy as np

# ---- constants of k_dec_rank, by the names the kernel gives them ------------------------------------------------------------------------
ROW = 64              # entries per row (rows[256][64]); also the width of the fast loop's store
RANK_LOW = 24         # top a row up when fewer known entries remain ...
TOPUP_MARGIN = 8      # ... `nv2 < RANK_LOW + 8u`
TAIL = 63             # fast_end = len - 63: the general path owns the last 63 bytes
END = 0xFF            # row entries past the end of a bucket
NONE = 256            # psym: no top-up in flight

EVENTS = (
    "fast", "fast-zeros",                       # fast iteration without / with leading zero ranks
    "fast-exit-64",                             # the fast loop leaves for the insert of a rank >= 64
    "insert<64", "insert>=64",                  # general-path insert
    "drop<64", "drop>=64",                      # front drop of an exhausted bucket, by depth
    "last-drop",                                # uniq -> 0, lim = 1
    "drop-behind-zeros",                        # the bucket ends behind a zero run
    "run-past-known-64", "run-past-known-part",  # a zero run covers all known entries: all 64 known / fewer
    "topup-full", "topup-cut",                  # pcnt == want / cut by the bucket's end
    "topup-empty-row",                          # issued with nv2 == 0
    "land-current", "land-other",               # the topped-up symbol is / is not the current one
    "used-64",                                  # fast iterations consumed a row to exactly 64
    "zero-progress",                            # general iteration that emits nothing
    "general-tail",                             # general iteration at i >= fast_end
    "uniq-0",                                   # visit of an exhausted bucket with uniq == 0
    "clip",                                     # cnt > rest
    "twin",                                     # fast iteration whose next symbol is the current one: list positions 0 and 1 hold the same symbol
)
UNREACHABLE = {                                 # by valid arrays; HOSTILE_ONLY names what hostile arrays add
    "clip": "a visit emits at most left + 1 bytes, the symbols' left + 1 add up to len, and with uniq == 0 a visit emits one byte",
    "uniq-0": "valid arrays end with the last drop; hostile arrays reach it",
    "twin": "valid arrays keep list positions 0 and 1 distinct; hostile arrays reach it",
}

# name -> what the switch changes.  Parameters of walk() and of nothing else.
MUTANTS = {
    "norm-le": "normalisation keeps entry l while l + cnt <= nv instead of < nv",
    "unknown-known": "the scan of the general path takes unknown row entries as known",
    "inflight-fast-64": "with a top-up in flight the fast limit is min(64, left2) instead of min(nv2, left2)",
    "nv2-no-reset": "nv2 is not reset to 64 when the whole bucket is loaded",
    "pcnt-uncut": "pcnt = want, not cut to what the bucket still has",
    "land-off+1": "the top-up lands one entry too high",
    "fast-end-late": "fast_end = len - 62",
    # the five below cannot change a byte of a valid stream: EQUIVALENT
    "loaded-gt-init": "all_loaded at the start is gpos > gend instead of >=",
    "loaded-gt-general": "all_loaded in the general path is gpos > gend instead of >=",
    "left-f": "left starts as f instead of f - 1",
    "land-nv-exact": "nv after a landing is poff + pcnt instead of 64",
    "slack-64": "rank_fast_limit's slack is always 64",
    # decodes every valid stream, differs from the reference on corrupt ones: HOSTILE_ONLY
    "stale-twin": "the next symbol's counters are not read again when the next symbol is the current one",
}
EQUIVALENT = {
    "loaded-gt-init": "gpos == gend only delays the flag: the general path tops the row up by min(want, 0) = 0 entries and the landing sets nv = 64",
    "loaded-gt-general": "as loaded-gt-init: a top-up of no entries, then nv = 64 over a tail that normalisation filled with 0xFF",
    "left-f": "the entry behind a bucket's end is 0xFF, and an insert at rank 255 moves the same live list positions as a front drop; "
              "uniq is then one too high, which only deepens later drops past the live positions",
    "land-nv-exact": "the entries behind poff + pcnt are 0xFF either way; with them unknown the scan stops at the same place "
                     "and the next normalisation reads all_loaded",
    "slack-64": "the slack only decides how early a row asks for a top-up, never which entry is read",
}
HOSTILE_ONLY = {
    "stale-twin": "list positions below uniq hold distinct symbols and a valid rank is below uniq, so positions 0 and 1 never hold the same "
                  "symbol; a corrupt rank pulls the copies of symbol 0 that fill the unnamed positions to the front",
}
HOSTILE_EVENTS = ("uniq-0", "twin")            # reached by hostile arrays only


class Undefined(ValueError):
    """the reference has no defined answer for this array"""


class Invariant(AssertionError):
    """walk() met a state the kernel must never be in"""


def sorted_map(freq):
    """GenerateSortedMap (rank.cpp:15-39): symbols with freq > 0, larger frequency first, ties by the smaller symbol"""
    return sorted((s for s in range(256) if freq[s] > 0), key=lambda s: (-freq[s], s))


def encode(T):
    """Postcoder::Encode (rank.cpp:45-90) -> (R as bytes, freq as a list of 256)"""
    T = bytes(T)
    freq = [0] * 256
    lst = []
    for s in T:
        if freq[s] == 0:
            lst.append(s)                       # first-appearance order
        freq[s] += 1
    bucket, pos = {}, 0
    for s in sorted_map(freq):
        bucket[s] = pos
        pos += freq[s]
    R = bytearray(len(T))
    for s in T:
        r = lst.index(s)
        R[bucket[s]] = r
        bucket[s] += 1
        if r:
            del lst[r]
            lst.insert(0, s)
    return bytes(R), freq


def _layout(R, freq):
    """(start list, bucket start per symbol) as rank.cpp:114-123 builds them; Undefined for a start position named twice"""
    n = len(R)
    if min(freq) < 0 or sum(freq) != n:
        raise Undefined("frequencies do not add up to the length")
    lst, start, pos, named = [0] * 256, {}, 0, set()
    for s in sorted_map(freq):
        if R[pos] in named:
            raise Undefined("two buckets name the same start position")
        named.add(R[pos])
        lst[R[pos]] = s
        start[s] = pos
        pos += freq[s]
    return lst, start


def decode(R, freq):
    """Postcoder::Decode (rank.cpp:96-151), the list initialised to zero"""
    R = bytes(R)
    n = len(R)
    lst, start = _layout(R, freq)
    uniq = len(start)
    bpos = {s: start[s] + 1 for s in start}
    bend = {s: start[s] + freq[s] for s in start}
    T = bytearray(n)
    sym = lst[0]
    for i in range(n):
        T[i] = sym
        if sym not in bpos:
            raise Undefined("a list position that no bucket names came to the front and symbol 0 has no bucket")
        if bpos[sym] < bend[sym]:
            r = R[bpos[sym]]
            bpos[sym] += 1
            if r:
                del lst[0]
                lst.insert(r, sym)
                sym = lst[0]
        elif uniq > 0:
            uniq -= 1
            k = max(uniq, 1)                    # do { } while (++k < uniq): at least once
            lst[0:k] = lst[1:k + 1]
            sym = lst[0]
    return bytes(T)


def _fast_limit(nv, left, all_loaded, mutant):
    """rank_fast_limit"""
    slack = ROW if (all_loaded or mutant == "slack-64") else max(nv - RANK_LOW, 0)
    return min(nv, left, slack)


def walk(R, freq, mutant=None, log=None):
    """k_dec_rank's scheme on one chunk -> (T, events).  events: a Counter over EVENTS plus three sets, "fast-ranks" (ranks inserted by the
    fast loop), "general-ranks" (by the general path) and "drop-depths".  log: a list that receives (i, event) in order.
    Raises Invariant where the kernel would store outside its chunk or its row, or would spin."""
    assert mutant is None or mutant in MUTANTS, mutant
    R = bytes(R)
    n = len(R)
    ev = Counter()
    fast_ranks, general_ranks, drop_depths = set(), set(), set()

    def note(name, at):
        ev[name] += 1
        if log is not None:
            log.append((at, name))

    lst, start = _layout(R, freq)
    uniq = len(start)
    T = bytearray(n)
    if n == 0:
        return bytes(T), dict(ev, **{"fast-ranks": fast_ranks, "general-ranks": general_ranks, "drop-depths": drop_depths})
    rows, meta, span = [], [], []
    for s in range(256):
        f = freq[s]
        b = start.get(s, n)                     # an absent symbol's bucket is the empty one behind all others
        g, ge = b + 1, b + f
        rows.append([R[g + j] if g + j < ge else END for j in range(ROW)])
        left = f if mutant == "left-f" else (f - 1 if f else 0)
        gpos = b + 1 + ROW
        loaded = gpos > ge if mutant == "loaded-gt-init" else gpos >= ge
        meta.append([0, _fast_limit(ROW, left, loaded, mutant), ROW, left])            # used, fast, nv, left
        span.append([gpos, ge])
    fast_end = n - TAIL + (mutant == "fast-end-late") if n >= ROW else 0
    sym = lst[0]
    m = list(meta[sym])                         # the current symbol's counters as a register copy
    psym, poff, pcnt, stage = NONE, 0, 0, []
    i = 0
    idle = 0                                    # general iterations in a row that emitted nothing and changed no list
    while True:
        # ---- inner loop ----
        while True:
            used = m[0]
            if used > ROW or m[1] < used:
                raise Invariant(f"i={i} sym={sym}: used {used} fast {m[1]}")
            room = m[1] - used
            row = rows[sym]
            z = next((k for k in range(ROW - used) if row[used + k]), None)
            lim = room if i < fast_end else 0
            if z is None or not z < lim:
                break
            nsym = lst[1]
            r = row[used + z]
            nm = list(meta[nsym])               # read before this symbol's counter is written ...
            if i + ROW > n:
                raise Invariant(f"i={i}: the fast loop's store reaches byte {i + ROW - 1} of {n}")
            T[i:i + ROW] = bytes((sym,)) * ROW
            note("fast-zeros" if z else "fast", i)
            i += z + 1
            idle = 0
            meta[sym][0] = used + z + 1
            if nsym == sym and mutant != "stale-twin":
                nm = list(meta[nsym])           # ... and read again when the list holds the current symbol twice (corrupt arrays only)
                note("twin", i)
            if used + z + 1 == ROW:
                note("used-64", i)
            fast_ranks.add(r)
            if r >= ROW:
                note("fast-exit-64", i)
            del lst[0]
            lst.insert(r, sym)
            sym, m = nsym, nm
        if i >= n:
            break
        # ---- general path ----
        if psym != NONE:                        # land the top-up in flight, start over
            at = poff + (1 if mutant == "land-off+1" else 0)
            if at + pcnt > ROW:
                raise Invariant(f"i={i}: a top-up lands at {at} .. {at + pcnt}")
            rows[psym][at:at + pcnt] = stage
            meta[psym][2] = poff + pcnt if mutant == "land-nv-exact" else ROW
            meta[psym][1] = _fast_limit(meta[psym][2], meta[psym][3], span[psym][0] >= span[psym][1], mutant)
            note("land-current" if psym == sym else "land-other", i)
            psym = NONE
            m = list(meta[sym])
            continue
        if i >= fast_end:
            note("general-tail", i)
        used = m[0]
        rest = n - i
        gpos, gend = span[sym]
        nv, left = m[2] - used, m[3] - used
        if nv < 0 or left < 0:
            raise Invariant(f"i={i} sym={sym}: nv {nv} left {left}")
        row = rows[sym]
        rlk = [row[(j + used) & 63] if (j < nv or mutant == "unknown-known") else END for j in range(ROW)]
        zk = next((j for j in range(ROW) if rlk[j]), ROW)
        stop = zk < nv
        cnt = zk + 1 if stop else zk
        if cnt > rest:
            note("clip", i)
            cnt = rest
        T[i:i + cnt] = bytes((sym,)) * cnt
        at = i
        i += cnt
        keep = (lambda j: j + cnt <= nv) if mutant == "norm-le" else (lambda j: j + cnt < nv)
        shifted = [row[(j + used + cnt) & 63] if keep(j) else END for j in range(ROW)]
        loaded = gpos > gend if mutant == "loaded-gt-general" else gpos >= gend
        nv2 = ROW if (loaded and mutant != "nv2-no-reset") else nv - min(cnt, nv)
        left2 = left - min(cnt, left)
        cur = sym
        changed = False
        if stop:
            if zk < left:
                r = rlk[zk]
                note("insert>=64" if r >= ROW else "insert<64", at)
                general_ranks.add(r)
                del lst[0]
                lst.insert(r, sym)
                sym = lst[0]
                changed = True
            elif uniq > 0:
                uniq -= 1
                lim = max(uniq, 1)
                note("drop>=64" if lim >= ROW else "drop<64", at)
                drop_depths.add(lim)
                if uniq == 0:
                    note("last-drop", at)
                if zk:
                    note("drop-behind-zeros", at)
                lst[0:lim] = lst[1:lim + 1]
                sym = lst[0]
                changed = True
            else:
                note("uniq-0", at)
        elif nv:
            note("run-past-known-64" if nv == ROW else "run-past-known-part", at)
        if cnt == 0:
            note("zero-progress", at)
        idle = 0 if (cnt or changed) else idle + 1
        if idle > 1:
            raise Invariant(f"i={i} sym={cur}: two general iterations in a row without progress")
        rows[cur] = shifted
        if not loaded and nv2 < RANK_LOW + TOPUP_MARGIN:
            want = ROW - nv2
            avail = gend - gpos
            pcnt = want if mutant == "pcnt-uncut" else min(want, avail)
            if gpos + pcnt > n:
                raise Invariant(f"i={i}: a top-up reads R[{gpos} .. {gpos + pcnt}) of {n}")
            poff = nv2
            stage = list(R[gpos:gpos + pcnt])
            psym = cur
            note("topup-full" if pcnt == want else "topup-cut", at)
            if nv2 == 0:
                note("topup-empty-row", at)
            fast = min(ROW, left2) if mutant == "inflight-fast-64" else _fast_limit(nv2, left2, True, mutant)
            span[cur][0] = gpos + want
        else:
            fast = _fast_limit(nv2, left2, loaded, mutant)
        meta[cur] = [0, fast, nv2, left2]
        m = list(meta[sym])
    return bytes(T), dict(ev, **{"fast-ranks": fast_ranks, "general-ranks": general_ranks, "drop-depths": drop_depths})


# ---- crafted texts ----------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 33, 41, 64, 65, 66, 67, 88, 89, 97, 128, 129, 130, 200)      # bucket sizes around the row depth, 65 and their doubles
TWO_N = (1, 2, 63, 64, 65, 127, 128, 129)
ONE_N = (1, 64, 65, 66, 200, 5000)
RR_D = (64, 65, 68, 69, 250, 256)        # 250: rank 249, the one packed lane (248 .. 251) whose general-path inserts the ladder misses


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


def two(n):
    """two alternating bytes: every rank is 1, no zero rank, lengths at the tail boundary"""
    return _u8(np.array([0, 7])[np.arange(n) % 2])


def one(n):
    """one byte: a single bucket holding one zero run.  n = 65: the first window holds the whole bucket; 66: a top-up cut to one entry"""
    return _u8(np.zeros(n))


def sizes(shuffled, seed=5):
    """one symbol (0, 1, 2 ...) per bucket size of SIZES; shuffled, or every symbol's occurrences contiguous in order of size, largest first
    (the order of the buckets in R)"""
    t = np.repeat(np.arange(len(SIZES)), SIZES)
    if shuffled:
        return _u8(np.random.default_rng(seed).permutation(t))
    return _u8(t[::-1])


def runs(lengths, nsym=5, nruns=80, seed=6):
    """few symbols in runs: lengths = 200 (zero runs longer than a row, crossing top-ups) or (1, 150) (uniform in that range)"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, nsym, nruns)
    s[0] = 0
    ln = np.full(nruns, lengths) if isinstance(lengths, int) else rng.integers(lengths[0], lengths[1] + 1, nruns)
    return _u8(np.repeat(s, ln))


def round_robin(d):
    """every rank is d - 1: list positions 63 and 64 (both ends of the packed register's lane 0), 67 | 68 and 255 (the last byte of lane 47).
    70 rounds: buckets above 65 entries, so rows run low and the general path inserts at that depth too"""
    return _u8(np.arange(70 * d + 17) % d)


def ladder():
    """arange(3 d) % d for d = 2 .. 256: every insert rank and every drop depth 1 .. 255"""
    return _u8(np.concatenate([np.arange(3 * d) % d for d in range(2, 257)]))


def noise(with_runs, seed=8):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, 30_000)
    if with_runs:
        t = np.repeat(t, rng.integers(1, 4, len(t)))[:30_000]
    return _u8(t)


TEXTS = tuple([f"two-{n}" for n in TWO_N] + [f"one-{n}" for n in ONE_N] + ["sizes-shuffled", "sizes-sorted", "runs-200", "runs-1-150"]
              + [f"rr-{d}" for d in RR_D] + ["ladder", "noise", "noise-runs"])
HOSTILE_FROM = ("ladder", "sizes-shuffled", "runs-1-150", "rr-69")              # every one holds a zero byte
HOSTILE_KINDS = ("zeros", "uniform", "sparse", "flips")


@functools.lru_cache(maxsize=None)
def crafted(name):
    kind, _, arg = name.partition("-")
    if kind == "two":
        return two(int(arg))
    if kind == "one":
        return one(int(arg))
    if kind == "sizes":
        return sizes(arg == "shuffled")
    if kind == "runs":
        return runs(200) if arg == "200" else runs((1, 150))
    if kind == "rr":
        return round_robin(int(arg))
    if kind == "ladder":
        return ladder()
    if kind == "noise":
        return noise(arg == "runs")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def crafted_ranks(name):
    """encode() of a crafted text"""
    return encode(crafted(name).tobytes())


@functools.lru_cache(maxsize=None)
def crafted_walk(name, mutant=None):
    """(decoded exactly?, events or the Invariant's text) of a crafted text under a mutant: computed once, shared"""
    R, freq = crafted_ranks(name)
    try:
        T, ev = walk(R, freq, mutant)
    except Invariant as e:
        return False, str(e)
    return T == crafted(name).tobytes(), ev


def hostile(name, kind, seed=9):
    """(R, freq) of a crafted text with every entry but the buckets' first ones overwritten: zeros, uniform bytes, sparse non-zero bytes
    (one in 40), or 1 % of the entries replaced.  The start positions stay distinct."""
    R, freq = crafted_ranks(name)
    rng = np.random.default_rng([seed, HOSTILE_FROM.index(name), HOSTILE_KINDS.index(kind)])
    a = np.frombuffer(R, dtype=np.uint8).copy()
    keep = np.zeros(len(a), dtype=bool)
    pos = 0
    for s in sorted_map(freq):
        keep[pos] = True
        pos += freq[s]
    rnd = rng.integers(0, 256, len(a)).astype(np.uint8)
    if kind == "zeros":
        new = np.zeros_like(a)
    elif kind == "uniform":
        new = rnd
    elif kind == "sparse":
        new = np.where(rng.random(len(a)) < 1 / 40, np.maximum(rnd, 1), 0).astype(np.uint8)
    else:
        new = np.where(rng.random(len(a)) < 0.01, rnd, a).astype(np.uint8)
    return np.where(keep, a, new).astype(np.uint8).tobytes(), list(freq)


# ---- two-chunk images of the product path (ANS_CHUNK = 1 MiB) ---------------------------------------------------------------------------
CHUNK = 1 << 20
IMAGES = ("zeros+ladder", "ladder-split", "sizes-split")
LADDER_SPLIT = 384          # bytes of the ladder's d = 256 phase (its last 768 bytes) that stay in chunk one: one round and a half


@functools.lru_cache(maxsize=None)
def image(name):
    """zeros+ladder: a chunk of zero bytes, then the ladder as a chunk of its own (a non-zero out_off).  ladder-split: the edge falls
    LADDER_SPLIT bytes into the ladder's round robin of 256, so chunk one ends inside it -- its last 63 bytes are last occurrences, front
    drops from depth 62 down, behind 192 drops at 64 and deeper -- and chunk two starts with a fresh list in the middle of a round.  sizes-split: the edge falls inside
    sizes-shuffled.  The fill in front is zero bytes: symbol 0 of the crafted part gets a bucket of about a MiB."""
    if name == "zeros+ladder":
        head, body = CHUNK, crafted("ladder")
    elif name == "ladder-split":
        body = crafted("ladder")
        head = CHUNK - (len(body) - 768 + LADDER_SPLIT)
    elif name == "sizes-split":
        body = crafted("sizes-shuffled")
        head = CHUNK - 600
    else:
        raise KeyError(name)
    return _u8(np.concatenate((np.zeros(head, dtype=np.uint8), body)))
