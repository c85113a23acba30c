"""The middle of the rANS encoder restated in plain Python: the class ordinals (k_cls_count, k_cls_prefix, k_cls_ord), the QuasiModel tables
(k_quasi_build) and the QuasiModel half of k_pairs -- and the crafted inputs that reach its index edges.  No GPU code is imported; the
functions that need the oracle take it as an argument.

The reference rebuilds a QuasiModel sequentially after EXP + 1 symbols of its class.  The kernels turn that into a closed-form schedule
(qbound: interval q of a class covers the class ordinals [qbound(q), qbound(q + 1))), a stable ordinal per symbol built in four layers
(symbols of the class in front of the tile, in the waves in front of this one, in this wave's earlier iterations, in the lanes below),
per-interval mantissa histograms (an LDS copy for the interval the tile starts in, global atomics for the later ones), one wave per
(interval, class, chunk) that builds the table of interval r from the histogram of interval r - 1 unless the class never gets there, and a
lookup qcdf[qinterval(ord)] in k_pairs.  The model follows the code, layer by layer, so that ONE changed token of it (MUTANTS) is one
changed line here.

  Arena           what survives from one call to the next in the context's arena: qhist (cleared by every call) and qcdf (never
                  cleared: a table the skip rule leaves out keeps what an earlier call built there).  A fresh one holds STALE words
  run(chunks)     the stage on the RLE0 symbol streams of one call's chunks -> per chunk the mantissa words of the classes >= 2 (the
                  model owns nothing else), the ordinals, and what reach() needs.  `mut` names ONE changed token (MUTANTS)
  splice(...)     the oracle's pairs with the model's words in the places the model owns
  reach(symbols)  named events of the scheme a stream reaches; conditions on the input alone
  CASES / decoy / IMAGES / GROUP   the inputs.  decoy(name) has the case's length and class sequence and every mantissa mirrored: the same
                  arena layout, and every bin and table it leaves behind is wrong for the case

Mutants that cannot change a word (EQUIVALENT, with the reason) are kept: the test asserts that they change none."""
import functools

import numpy as np

CHUNK = 1 << 20
ATILE = 4096
TB = 256
W = TB // 64                       # waves per tile
IT = ATILE // TB                   # 64-symbol iterations per wave: symbol i = ts + w * 1024 + it * 64 + l
NQ = 32
QSTRIDE = 132
STALE_HIST = 3                     # a histogram bin nobody cleared
STALE_CDF = 0x0BAD                 # a table word nobody wrote: two of them side by side are a frequency of 0

MUTANTS = (
    "qbound-lo+1", "qbound-hi+1",          # qbound: one more on the doubling branch / on the + 65 537 branch
    "qinterval-<",                         # qinterval: qbound(q + 1) < k
    "skip+2", "skip-next-bound",           # k_quasi_build: clstotal < qbound(r) + 2 / clstotal < qbound(r + 1)
    "hist-of-r",                           # k_quasi_build: the table of interval r from the histogram of interval r
    "flush-q0+1",                          # k_cls_ord: the LDS copy flushed to interval q0 + 1
    "wave-prefix-inclusive",               # k_cls_ord: s += v; cnt[k] = s
    "wave-count-stuck",                    # k_cls_ord: cnt[w][e] not advanced
    "below-le",                            # k_cls_ord: m & lanemask_le
    "plus1-dropped",                       # k_quasi_build: F = F >> lg
    "remainder-to-last",                   # k_quasi_build: 65536 - t3 to the class's last symbol
    "carry-dropped",                       # k_quasi_build: no carry from one register of 64 lanes to the next
    "cdf-end-unwritten",                   # k_quasi_build: cdf[A] not written
    "m-without-base",                      # k_pairs: m = sym
    "table-offset-c8",                     # k_pairs: c * 8 + (e - 2)
    "qhist-clear-short",                   # the call's memset: nch * 6 * (NQ - 1) * QSTRIDE words
    # equivalent ones
    "qbound-switch-12", "qbound-switch-14",        # qbound: q <= 12 / q <= 14
    "q0-from-base+1",                      # k_cls_ord: q0 = qinterval(clsbase + 1)
    "lg->=",                               # k_quasi_build: while ((tot >> lg) + A >= 65536)
    "skip-<=",                             # k_quasi_build: clstotal <= qbound(r)
    "match-any-without-valid",             # k_cls_ord: match_any<3>(e, true)
    "count-unclamped",                     # k_cls_count: the i < n mask of the ragged tile dropped, its clamped loads counted
)
# mutant -> why no input can tell it from the scheme
EQUIVALENT = {
    "qbound-switch-12": "the two branches agree at q = 13: 8 (2^13 - 1) + 13 + 0 * 65537",
    "qbound-switch-14": "and at q = 14: interval 13 is 8 * 2^13 + 1 = 65 537 ordinals long, the step of the second branch",
    "q0-from-base+1": "which interval the LDS copy stands for is free: the symbols of that interval go to the copy, the copy goes to that "
                      "interval, and every other symbol goes to its own bin.  (The flush target alone is not: flush-q0+1)",
    "lg->=": "a table is built from a COMPLETE interval, tot = 16 (8 * 2^k + 1) = 2^(k + 7) + 16: no shift of that plus an alphabet of "
             "4 .. 129 is 65 536",
    "skip-<=": "the table of interval r is read by the ordinals >= qbound(r): a class of exactly qbound(r) symbols has ordinals up to "
               "qbound(r) - 1 and never reads it; the kernel's < builds one table more than is read",
    "match-any-without-valid": "the lanes past the chunk's end are the highest lanes of the last iteration that has symbols: they are below "
                               "nobody, they lead no update themselves, and what they add to the running count of class 0 is read only "
                               "by iterations and waves that hold no symbol",
    "count-unclamped": "the clamped loads repeat the chunk's last symbol in the chunk's last tile: only clstotal of that symbol's class "
                       "grows, the exclusive prefix of no tile does.  A QuasiModel table is then built for an interval no ordinal reaches "
                       "and nobody reads it (the AdaptiveModel's item count of a class 0/1 stream is adapt_segment_model's, not this "
                       "model's)",
}
BIG = 100_000                              # cases above this many symbols run BIG_MUTANTS only in the test's sweep
BIG_MUTANTS = ("qbound-hi+1", "qbound-switch-14", "qbound-switch-12", "skip+2", "skip-<=", "qhist-clear-short", "count-unclamped")

_CLS = np.array([0, 0] + [int(s).bit_length() - 1 for s in range(2, 128)] + [7] * 129, dtype=np.int8)      # sym_class of 0 .. 256


def sym_class(s):
    return _CLS[s]


def class_base(e):
    return 0 if e == 0 else 1 << e


def class_alpha(e):
    return 129 if e == 7 else 2 if e == 0 else 1 << e


_BASE = np.array([class_base(e) for e in range(8)], dtype=np.int64)
_ALPHA = np.array([class_alpha(e) for e in range(8)], dtype=np.int64)


def qbound(q, mut=None):
    sw = 12 if mut == "qbound-switch-12" else 14 if mut == "qbound-switch-14" else 13
    if q <= sw:
        return 8 * ((1 << q) - 1) + q + (mut == "qbound-lo+1")
    return 8 * ((1 << 13) - 1) + 13 + (q - 13) * 65537 + (mut == "qbound-hi+1")


def qinterval(k, mut=None):
    """the kernel's loop on an array of ordinals: the last q < NQ with qbound(q) <= k (clamped at NQ - 1)"""
    b = np.array([qbound(q, mut) for q in range(1, NQ)], dtype=np.int64)
    return np.searchsorted(b, np.asarray(k, dtype=np.int64), side="left" if mut == "qinterval-<" else "right")


def uniform_cdf(A, i):
    if i <= 0:
        return 0
    scale = 65536 // A
    return i * scale + (65536 - scale * A)


# ---- the arena ------------------------------------------------------------------------------------------------------------------------
class Arena:
    """qhist and qcdf of up to `nch` chunks, [chunk * 6 + class - 2][interval][QSTRIDE] each, with room behind them for the reads of a
    mutant (they then see STALE words, as a read past the array would)"""

    def __init__(self, nch=1):
        self.nch = nch
        words = (8 * nch + 2) * NQ * QSTRIDE
        self.qhist = np.full(words, STALE_HIST, dtype=np.int64)
        self.qcdf = np.full(words, STALE_CDF, dtype=np.int64)


def _row(c, e, q):
    return ((c * 6 + (e - 2)) * NQ + q) * QSTRIDE


# ---- k_cls_count, k_cls_prefix, k_cls_ord's ordinals ----------------------------------------------------------------------------------
def ordinals(s, mut=None):
    """the class stage of one chunk as far as it depends on the CLASSES alone -> dict(e, clsbase [tile][8], clstotal [8], ord)"""
    s = np.asarray(s)
    n = len(s)
    T = (n + ATILE - 1) // ATILE
    N = T * ATILE
    e = np.zeros(N, dtype=np.int64)                    # a lane past the end holds symbol 0
    e[:n] = _CLS[s]
    oh = np.zeros((N, 8), dtype=np.int8)               # one-hot class of the valid symbols
    oh[np.arange(n), e[:n]] = 1
    # k_cls_count: per tile and class; the ragged tile's loads are clamped to the last symbol and masked
    clscnt = oh.reshape(T, ATILE, 8).sum(axis=1, dtype=np.int64)
    if mut == "count-unclamped":
        clscnt[T - 1, e[n - 1]] += N - n
    # k_cls_prefix: exclusive over the tiles, and the total
    clsbase = np.cumsum(clscnt, axis=0) - clscnt
    clstotal = clscnt.sum(axis=0)
    # k_cls_ord: wave w of a tile owns its symbols [w * 1024, w * 1024 + 1024), sixteen iterations of 64 lanes
    mh = oh
    if mut == "match-any-without-valid":
        mh = oh.copy()
        mh[n:, 0] = 1
    m5 = mh.reshape(T, W, IT, 64, 8)
    incl = np.cumsum(m5, axis=3, dtype=np.int8)                             # at most 64
    below = incl if mut == "below-le" else incl - m5                       # lanes below me with my class
    pop = incl[:, :, :, -1, :].astype(np.int64)                            # popcount of the match mask, per class
    # the lane that finds nobody below it advances the wave's count -- if it holds a symbol
    if mut in ("wave-count-stuck", "below-le"):                            # (with <= every lane finds itself: nobody advances it)
        adv = np.zeros_like(pop)
    else:
        adv = np.where(oh.reshape(T, W, IT, 64, 8).any(axis=3), pop, 0)
    run = np.cumsum(adv, axis=2) - adv                                     # the wave's count when the iteration starts
    wt = adv.sum(axis=2)                                                   # ... and when the wave is done
    wp = np.cumsum(wt, axis=1) - (0 if mut == "wave-prefix-inclusive" else wt) + clsbase[:, None, :]
    base = (wp[:, :, None, :] + run).reshape(T * W * IT, 8)
    g = np.arange(N) // 64
    own = np.take_along_axis(below.reshape(N, 8), e[:, None], axis=1)[:, 0]
    ord_ = base[g, e] + own.astype(np.int64)
    return {"n": n, "T": T, "e": e[:n], "clsbase": clsbase, "clstotal": clstotal, "ord": ord_[:n]}


# ---- k_cls_ord's histograms -----------------------------------------------------------------------------------------------------------
def _histograms(a, c, s, st, mut):
    n, e, k = st["n"], st["e"], st["ord"]
    sel = np.flatnonzero(e >= 2)
    if not sel.size:
        return
    es, ks = e[sel], k[sel]
    m = np.asarray(s, dtype=np.int64)[sel] - _BASE[es]
    q = qinterval(ks, mut)
    q0 = qinterval(st["clsbase"] + (1 if mut == "q0-from-base+1" else 0), mut)          # [tile][8]: the interval the tile starts in
    q0s = q0[sel // ATILE, es]
    flush = q0s + (1 if mut == "flush-q0+1" else 0)
    tq = np.where(q == q0s, flush, q)                                      # the LDS copy is flushed once, to one interval
    idx = ((c * 6 + (es - 2)) * NQ + tq) * QSTRIDE + m
    a.qhist += np.bincount(idx, minlength=len(a.qhist))


# ---- k_quasi_build --------------------------------------------------------------------------------------------------------------------
def _build(a, c, st, mut, info):
    M32 = 0xFFFFFFFF
    for e in range(2, 8):
        A = class_alpha(e)
        tot_cls = int(st["clstotal"][e])
        for r in range(NQ):
            cdf = a.qcdf[_row(c, e, r): _row(c, e, r) + QSTRIDE]
            if r == 0:
                cdf[: A + 1] = [uniform_cdf(A, i) for i in range(A + 1)]
                continue
            if mut == "skip+2":
                skip = tot_cls < qbound(r, mut) + 2
            elif mut == "skip-next-bound":
                skip = tot_cls < qbound(r + 1, mut)
            elif mut == "skip-<=":
                skip = tot_cls <= qbound(r, mut)
            else:
                skip = tot_cls < qbound(r, mut)
            if skip:
                continue                                                   # this table is never reached: the row keeps what it held
            hr = r if mut == "hist-of-r" else r - 1
            h = a.qhist[_row(c, e, hr): _row(c, e, hr) + 192].copy()
            h[A:] = 0                                                      # three registers of 64 lanes, i < A
            F = (16 * h) & M32
            tot = int(F.sum()) & M32
            lg = 0
            while ((tot >> lg) + A >= 65536) if mut == "lg->=" else ((tot >> lg) + A > 65536):
                lg += 1
            F = (F >> lg) + (0 if mut == "plus1-dropped" else 1)
            F[A:] = 0
            t2 = int(F.sum()) & M32
            F = ((65536 * F) & M32) // t2 if t2 else np.full(192, M32, dtype=np.int64)
            t3 = int(F.sum()) & M32
            rem = (65536 - t3) & M32
            F[A - 1 if mut == "remainder-to-last" else 0] += rem
            F &= M32
            out = np.zeros(192, dtype=np.int64)
            carry = 0
            for k in range(3):
                inc = np.cumsum(F[64 * k: 64 * k + 64])
                out[64 * k: 64 * k + 64] = (carry + inc - F[64 * k: 64 * k + 64]) & M32
                if mut != "carry-dropped":
                    carry += int(inc[-1])
            cdf[:A] = out[:A]
            if mut != "cdf-end-unwritten":
                cdf[A] = 65536
            info[(c, e, r)] = {"lg": lg, "rem": rem, "one-bin": int((h[:A] > 0).sum()) == 1}


# ---- the quasi half of k_pairs --------------------------------------------------------------------------------------------------------
def _pairs(a, c, s, st, mut):
    """-> (mantissa word of every symbol, 0 where the class is 0 or 1; its interval, -1 there)"""
    n, e, k = st["n"], st["e"], st["ord"]
    words = np.zeros(n, dtype=np.uint32)
    qq = np.full(n, -1, dtype=np.int64)
    sel = np.flatnonzero(e >= 2)
    if sel.size:
        es = e[sel]
        sv = np.asarray(s, dtype=np.int64)[sel]
        m = sv if mut == "m-without-base" else sv - _BASE[es]
        q = qinterval(k[sel], mut)
        row = (((c * 8 if mut == "table-offset-c8" else c * 6) + (es - 2)) * NQ + q) * QSTRIDE
        lo = a.qcdf[row + m]
        fr = (a.qcdf[row + m + 1] - lo) & 0xFFFFFFFF
        words[sel] = ((lo | (fr << 16)) & 0xFFFFFFFF).astype(np.uint32)
        qq[sel] = q
    return words, qq


def run(chunks, arena=None, mut=None, pre=None):
    """one call of the stage on the symbol streams `chunks` (one per chunk).  `pre`: the ordinals() of the chunks where the caller has them
    (they depend on the classes alone: a case and its decoy share them).  -> list of dicts, one per chunk: words, q, ord, e, clsbase,
    clstotal, tables {(class, interval): lg, rem, one-bin}"""
    assert mut is None or mut in MUTANTS, mut
    nch = len(chunks)
    a = arena if arena is not None else Arena(nch)
    assert a.nch >= nch
    clear = nch * 6 * (NQ - 1 if mut == "qhist-clear-short" else NQ) * QSTRIDE
    a.qhist[:clear] = 0
    sts = [pre[c] if pre is not None else ordinals(s, mut) for c, s in enumerate(chunks)]
    info = {}
    for c, s in enumerate(chunks):
        _histograms(a, c, s, sts[c], mut)
    for c in range(nch):
        _build(a, c, sts[c], mut, info)
    out = []
    for c, s in enumerate(chunks):
        words, q = _pairs(a, c, s, sts[c], mut)
        out.append(dict(sts[c], words=words, q=q, tables={(e, r): v for (cc, e, r), v in info.items() if cc == c}))
    return out


def splice(oracle_pairs, res):
    """the oracle's pairs with the model's mantissa words of the classes >= 2"""
    p = np.array(oracle_pairs, dtype=np.uint32)
    own = res["e"] >= 2
    p[1::2][own] = res["words"][own]
    return p


# ---- events ---------------------------------------------------------------------------------------------------------------------------
EVENTS = (tuple(f"table-{r}" for r in range(28)) + tuple(f"lg-{k}" for k in range(6)) + ("q-13-to-14", "q-27") +
          tuple(f"total-at-bound{d}@r{w}" for w in ("<=3", "=14") for d in ("-1", "", "+1")) +
          ("tile-starts-at-bound-1", "tile-starts-at-bound", "tile-starts-at-bound+1", "tile-in-one-interval", "tile-spans-3-intervals",
           "tile-spans-9-intervals", "class-absent-from-tile", "class-only-at-4095", "class-only-at-0", "class-skips-a-wave",
           "wave-of-one-class", "wave-of-eight-classes", "last-tile-of-1", "last-tile-of-4095", "rlen-odd-last-quasi") +
          tuple(f"mantissa-top-coded-{e}" for e in range(2, 8)) + ("sym-256", "one-bin-interval", "freq-1-coded", "remainder-ge-64"))


def reach(symbols, res=None):
    """event -> how often (or whether) the stream reaches it.  The tables, widths and remainders are those of the scheme on a fresh arena.
    table-r: classes with a symbol coded in interval r; lg-k, one-bin-interval, remainder-ge-64: tables that code a symbol;
    tile-in-one-interval: a tile with two symbols of a class at least, all in one interval"""
    s = np.asarray(symbols, dtype=np.int64)
    n = len(s)
    res = res if res is not None else run([s])[0]
    e, k, q, T = res["e"], res["ord"], res["q"], res["T"]
    tot, base = res["clstotal"], res["clsbase"]
    pos = np.arange(n)
    tile = pos // ATILE
    quasi = e >= 2
    used = {(v // NQ, v % NQ) for v in np.unique(e[quasi] * NQ + q[quasi]).tolist()}               # (class, interval) that codes a symbol
    tabs = {key: v for key, v in res["tables"].items() if key in used}
    ev = {f"table-{r}": sum(1 for (_, b) in used if b == r) for r in range(28)}
    for g in range(6):
        ev[f"lg-{g}"] = sum(1 for v in tabs.values() if v["lg"] == g)
    ev["q-13-to-14"] = sum(1 for (_, b) in used if b == 14)
    ev["q-27"] = sum(1 for (_, b) in used if b == 27)
    for w, rs in (("<=3", (1, 2, 3)), ("=14", (14,))):
        for d, dv in (("-1", -1), ("", 0), ("+1", 1)):
            ev[f"total-at-bound{d}@r{w}"] = sum(1 for c in range(2, 8) for r in rs if int(tot[c]) == qbound(r) + dv)
    # per tile and class: symbols, intervals, first and last position, waves
    cnt = np.zeros((T, 8), dtype=np.int64)
    np.add.at(cnt, (tile, e), 1)
    bounds = {qbound(r): r for r in range(1, NQ)}
    for d, dv in (("-1", -1), ("", 0), ("+1", 1)):
        ev[f"tile-starts-at-bound{d}"] = sum(1 for t in range(1, T) for c in range(2, 8) if cnt[t, c] and int(base[t, c]) - dv in bounds)
    qs = q[quasi]
    key = (tile[quasi] * 8 + e[quasi]) * NQ + qs
    per = {}
    for v in np.unique(key).tolist():
        per.setdefault(v // NQ, []).append(v % NQ)
    spans = {tc: len(v) for tc, v in per.items()}
    ev["tile-in-one-interval"] = sum(1 for tc, v in spans.items() if v == 1 and cnt[tc // 8, tc % 8] >= 2)
    ev["tile-spans-3-intervals"] = sum(1 for v in spans.values() if v == 3)
    ev["tile-spans-9-intervals"] = sum(1 for v in spans.values() if v >= 9)
    ev["class-absent-from-tile"] = int(sum((cnt[:, c] == 0).sum() for c in range(2, 8) if tot[c]))
    inp = pos % ATILE
    single = quasi & (cnt[tile, e] == 1)
    ev["class-only-at-4095"] = int((single & (inp == ATILE - 1)).sum())
    ev["class-only-at-0"] = int((single & (inp == 0)).sum())
    wv = np.zeros((T, W, 8), dtype=np.int64)
    np.add.at(wv, (tile, inp // (64 * IT), e), 1)
    ev["class-skips-a-wave"] = int(((wv[:, 0, 2:] > 0) & (wv[:, 1, 2:] == 0) & (wv[:, 2, 2:] > 0)).sum())
    G = (n + 63) // 64
    gc = np.zeros((G, 8), dtype=np.int64)
    np.add.at(gc, (pos // 64, e), 1)
    ev["wave-of-one-class"] = int((gc[:, 2:] == 64).sum())
    ev["wave-of-eight-classes"] = int((gc > 0).all(axis=1).sum())
    ev["last-tile-of-1"] = n % ATILE == 1
    ev["last-tile-of-4095"] = n % ATILE == ATILE - 1
    ev["rlen-odd-last-quasi"] = n % 2 == 1 and int(e[-1]) >= 2
    m = s - _BASE[e]
    for c in range(2, 8):
        ev[f"mantissa-top-coded-{c}"] = int(((e == c) & (m == class_alpha(c) - 1) & (q >= 1)).sum())
    ev["sym-256"] = int((s == 256).sum())
    ev["one-bin-interval"] = sum(1 for v in tabs.values() if v["one-bin"])
    ev["freq-1-coded"] = int((quasi & ((res["words"] >> 16) == 1)).sum())
    ev["remainder-ge-64"] = sum(1 for v in tabs.values() if v["rem"] >= 64)
    assert tuple(ev) == EVENTS
    return ev


# ---- the sequential schedule ----------------------------------------------------------------------------------------------------------
def sequential_intervals(n):
    """the interval of each of n ordinals as the reference counts them: a rebuild after EXP + 1 symbols, EXP = 8, 16, ..., 65 536, 65 536"""
    out = []
    expn, seen, q = 8, 0, 0
    for _ in range(n):
        out.append(q)
        seen += 1
        if seen > expn:
            seen, q = 0, q + 1
            expn = expn << 1 if expn < 65536 else 65536
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
ONE_CLASS = tuple((r, d) for r in (1, 2, 3, 10, 13, 14) for d in (-1, 0, 1))
DEEP = qbound(15) + 5
# tile-bounds: class 3's symbols per tile, so that the tiles 1 .. 9 start at qbound(q) - 1, qbound(q), qbound(q) + 1 for q = 1, 2, 5
TILE_BOUNDS_CLASS3 = (8, 1, 1, 15, 1, 1, 225, 1, 1)
TILE_BOUNDS_ALONE = {1: 0, 2: ATILE - 1, 4: 1023, 5: 1024, 7: ATILE - 1, 8: 0}     # where the one class-3 symbol of a tile sits


def _of_classes(rng, cls):
    """a random symbol of each given class"""
    cls = np.asarray(cls)
    return (_BASE[cls] + rng.integers(0, 1 << 30, len(cls)) % _ALPHA[cls]).astype(np.uint16)


def _tile_bounds(rng):
    tiles = []
    for t in range(10):
        x = rng.integers(2, 4, ATILE).astype(np.uint16)                   # class 1: literals, so that the stream decodes to a short text
        x[2::5] = rng.integers(0, 2, len(x[2::5]))                        # single run bits between them
        free = rng.permutation(ATILE)
        if t < 9:
            k3 = TILE_BOUNDS_CLASS3[t]
            at = np.array([TILE_BOUNDS_ALONE[t]]) if t in TILE_BOUNDS_ALONE else np.sort(free[:k3])
            x[at] = _of_classes(rng, np.full(len(at), 3))
        if t == 3:                                                         # class 4 in the waves 0 and 2 of this tile, none in wave 1
            taken = set(at.tolist())
            w0 = [p for p in free.tolist() if p < 1024 and p not in taken][:10]
            w2 = [p for p in free.tolist() if 2048 <= p < 3072 and p not in taken][:10]
            x[w0 + w2] = _of_classes(rng, np.full(20, 4))
        if t == 9:
            x[:64] = _of_classes(rng, np.full(64, 5))                      # one iteration of one class
            x[64:128] = _of_classes(rng, np.arange(64) % 8)                # and one of all eight
        tiles.append(x)
    return np.concatenate(tiles)


@functools.lru_cache(maxsize=None)
def case(name):
    """the named RLE0 symbol stream of one chunk as a read-only uint16 array"""
    rng = np.random.default_rng(sum(name.encode()) * 1000 + len(name))
    if name.startswith("one-class-"):
        r, d = name[len("one-class-"):].split("-", 1)
        s = rng.integers(4, 8, qbound(int(r)) + int(d))
    elif name == "class7-full":
        s = rng.integers(128, 257, CHUNK)
    elif name == "all-256":
        s = np.full(DEEP, 256)
    elif name == "skew-128":
        s = np.full(DEEP, 128)
        s[4096::4097] = 256
    elif name == "skew-128-gap":                                           # ... but none in interval 13: table 14 gives 256 a width of 1
        s = np.full(DEEP, 128)
        s[4096::4097] = 256
        s[qbound(13): qbound(14)] = 128
    elif name == "uniform-300k":
        s = rng.integers(2, 257, 300_000)
    elif name == "tile-bounds":
        s = _tile_bounds(rng)
    elif name in ("ragged-1", "ragged-4095", "odd-last-quasi"):
        s = rng.integers(0, 257, {"ragged-1": ATILE + 1, "ragged-4095": 2 * ATILE - 1, "odd-last-quasi": 3 * ATILE + 1}[name])
        if name == "odd-last-quasi":
            s[-1] = 32 + 17
    elif name == "tops":
        cls = rng.integers(2, 8, 3000)
        s = _of_classes(rng, cls).astype(np.int64)
        top = rng.integers(0, 2, len(cls)) == 1
        s[top] = (_BASE[cls] + _ALPHA[cls] - 1)[top]
    else:
        raise KeyError(name)
    s = np.asarray(s, dtype=np.uint16)
    assert len(s) <= CHUNK and int(s.max()) <= 256
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def decoy(name):
    """the case's length and class sequence, every mantissa mirrored: m -> A - 1 - m, the bit of the classes 0/1 flipped"""
    s = case(name).astype(np.int64)
    e = _CLS[s]
    d = (_BASE[e] + _ALPHA[e] - 1 - (s - _BASE[e])).astype(np.uint16)
    assert np.array_equal(_CLS[d], e)
    d.setflags(write=False)
    return d


CASES = (tuple(f"one-class-{r}-{d}" for r, d in ONE_CLASS) +
         ("class7-full", "all-256", "skew-128", "skew-128-gap", "uniform-300k", "tile-bounds", "ragged-1", "ragged-4095", "odd-last-quasi", "tops"))


def noise(rng, n, alphabet):
    return rng.integers(0, alphabet, n).astype(np.uint8)


SIXTEEN_ALPHABETS = (33, 5, 256, 9, 129, 17, 65, 256, 5, 129, 9, 65, 33, 17)       # chunks 0 .. 13; 14 repeats 3, 15 is one byte


@functools.lru_cache(maxsize=None)
def image(name):
    """a byte text for the product path (several chunks), read-only"""
    if name == "three-chunks":
        rng = np.random.default_rng(3003)
        c0 = noise(rng, CHUNK, 256)                                        # ranks all over: class 7 has every second symbol
        c1 = noise(rng, CHUNK, 7)                                          # ranks 0 .. 6: classes 1 and 2, and zero runs
        c2 = noise(rng, 70_001, 256)
        c2[::3] = c2[1::3][: len(c2[::3])]                                 # short: zero runs and every class
        t = np.concatenate((c0, c1, c2))
        assert len(t) == (2 << 20) + 70_001
    elif name == "sixteen-chunks":
        rng = np.random.default_rng(1616)
        cs = [noise(rng, CHUNK, a) for a in SIXTEEN_ALPHABETS]
        cs[11] = np.full(CHUNK, 77, dtype=np.uint8)                        # one chunk of one byte
        cs.append(cs[3].copy())                                            # chunk 14 = chunk 3: a tie in the launch order
        cs.append(noise(rng, ATILE + 1, 256))
        t = np.concatenate(cs)
        assert len(t) == (15 << 20) + ATILE + 1
    else:
        raise KeyError(name)
    t.setflags(write=False)
    return t


IMAGES = ("three-chunks", "sixteen-chunks")
# what the chunks of three-chunks are there for: (chunk 0, chunk 1, chunk 2)
IMAGE_REACH = {
    "three-chunks": (("table-20", "lg-5", "q-13-to-14", "sym-256", "mantissa-top-coded-7", "remainder-ge-64", "wave-of-eight-classes"),
                     ("table-21", "lg-5", "q-13-to-14", "tile-spans-9-intervals", "mantissa-top-coded-2"),
                     ("table-11", "lg-2", "class-absent-from-tile", "rlen-odd-last-quasi", "sym-256") +
                     tuple(f"mantissa-top-coded-{e}" for e in range(2, 8))),
}
GROUP_SPECS = ((30_000, 6), (35_000, 12), (40_000, 24), (45_000, 48), (50_000, 96), (55_000, 192), (62_000, 256), (70_000, 5))


@functools.lru_cache(maxsize=None)
def group():
    """eight texts of 30 000 - 70 000 bytes, noise over alphabets that give each a different dominant class"""
    rng = np.random.default_rng(8008)
    out = []
    for n, a in GROUP_SPECS:
        t = noise(rng, n, a)
        t.setflags(write=False)
        out.append(t)
    return tuple(out)


GROUP = tuple(f"group-{i}" for i in range(len(GROUP_SPECS)))


def chunks(t):
    t = np.asarray(t, dtype=np.uint8)
    return [t[a: a + CHUNK] for a in range(0, len(t), CHUNK)]


def chunk_symbols(oracle, chunk):
    """the RLE0 symbols of one chunk of bytes, from the oracle's stages"""
    r, _ = oracle.rank_encode(chunk)
    return oracle.rle_encode(r)


def density(chunk):
    """k_density: the bytes that differ from the byte in front of them (the chunk's first byte: from 0)"""
    c = np.asarray(chunk, dtype=np.uint8)
    return int((c[1:] != c[:-1]).sum()) + int(c[0] != 0)


def launch_order(dens):
    """k_order: densest first, ties by chunk number"""
    return sorted(range(len(dens)), key=lambda c: (-dens[c], c))
