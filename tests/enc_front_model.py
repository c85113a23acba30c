"""ans_enc_front.hip restated in plain Python: the scheme of the rank-coding kernels (k_enc_hist, k_enc_prep, k_enc_mtf) and of the RLE0
kernels (k_rle_lz, k_rle_ext, k_rle_tiles<false/true>, k_tile_prefix), tile by tile and group by group with the kernels' own intermediate
tables -- and the crafted inputs that reach their edges.  No GPU code is imported; what needs the oracle takes it as an argument.

The oracle is the reference ALGORITHM (one list, one pass).  This is the kernels' SCHEME, for one chunk:
  hist(T)             per 4096-byte tile the 256 counts and every symbol's last position; the 64-lane groups with their clamped loads and
                      the `valid` mask of a partial last group, one table per wave, the maximum over the four waves
  prep(...)           exclusive per-tile prefix counts, carried last-occurrence stamps, freq, bstart (descending frequency, ties ->
                      smaller symbol first)
  mtf(T, ...)         one wave per tile: the list rebuilt from the stamps (position = number of symbols with a later stamp, nseen = symbols
                      with a stamp), then 64-byte groups: heads, runlen, the rank found in list register 0..3 or taken as nseen++, the
                      shift with its carries lst0[63] -> lst1[0] ..., the scatter to pos[sym], which advances by the run
  rank_front(T)       the three together -> (R, freq, events)
  rle_front(R)        k_rle_lz (leading zeros per tile), k_rle_ext (the chain behind every tile), k_rle_tiles (per 16-byte thread segment:
                      first, the suffix minimum, after, prev, counts, symbols placed at toff + the thread's prefix), k_tile_prefix
                      -> (symbols, rlen, tables); rle_events(R) names what R reaches
Memory nobody wrote holds STALE values, so that a slot left out or a store beside its place shows.  `mut` names ONE changed token of the
scheme (MUTANTS); where the kernel has the token twice (the count pass and the emit pass of k_rle_tiles are one template) the emit pass
alone is changed, which is what a slip in a single-pass rewrite would look like.

Mutants that cannot change a byte (EQUIVALENT, with the reason) are kept: the test asserts that they change none.

The inputs: CASES (texts for the rank coder, none longer than six tiles), RANKS (byte arrays for the RLE0 probe, which takes any array),
IMAGES (product path, 1 MiB chunks) and GROUP (twelve block texts for the grouped encode: the clen / cmap form of the same kernels).
`runs-at-edges` is two texts: its seven runs alone are 24 768 bytes, more than six tiles."""
import functools

import numpy as np

CHUNK = 1 << 20
ATILE = 4096
TB = 256
WAVE = 64
SEG = 16                         # bytes per thread of k_rle_tiles
TRAILER = 480
EMPTY = 0xFFFF                   # a list position behind the symbols seen so far
STALE_RANK = 0xEE                # a rank nobody wrote
STALE_SYM = 0xEEEE               # an RLE0 symbol nobody wrote
STALE_BEFORE = 0                 # the byte in front of a chunk's first (read only by the mutant "prev-at-chunk-start-src")
INF = 0xFFFFFFFF

RANK_MUTANTS = (
    "prep-tie-larger-first",     # k_enc_prep: fk == f && k > s
    "prep-ge",                   # k_enc_prep: fk >= f
    "lastpos-first-lane",        # k_enc_hist: the position of the set's first lane
    "hist-valid-ignored",        # k_enc_hist: the clamped byte of a partial group is counted
    "place-ge",                  # k_enc_mtf: last >= own
    "nseen-from-zero",           # k_enc_mtf: nseen not taken from the stamps
    "carry1-dropped", "carry2-dropped", "carry3-dropped",        # k_enc_mtf: EMPTY enters lst1 / lst2 / lst3 at lane 0
    "part-lt",                   # k_enc_mtf: l < q
    "reg0-shift-lt",             # k_enc_mtf: l < rank
    "lane0-not-walked",          # k_enc_mtf: heads without `|| l == 0`
    "runlen-short",              # k_enc_mtf: nvalid - l - 1
    "pos-plus-one",              # k_enc_mtf: pos[cc] = dpos + 1
    "tilebase-inclusive",        # k_enc_prep: tilecnt[o] = f + n
    "prevc-lane63",              # k_enc_mtf: prevc = readlane(b, 63)
)
RLE_MUTANTS = (
    "ext-no-chain",              # k_rle_ext: e = z
    "ext-over-full-only",        # k_rle_ext: e = (z == tl) ? z + e : 0
    "after-without-ext",         # k_rle_tiles: after = tl
    "prev-at-tile-start-one",    # k_rle_tiles: prev = 1 for every tile's thread 0
    "prev-at-chunk-start-src",   # k_rle_tiles: prev = src[-1] for the chunk's first tile too
    "digits-one-more", "digits-one-less",        # k_rle_tiles<true>: b from 31 - clz / 29 - clz
    "digits-lsb-first",          # k_rle_tiles<true>: b upwards from 0
    "L-without-plus-one",        # k_rle_tiles<true>: L = nxt[k] - (p0 + k)
    "sym-plus-zero",             # k_rle_tiles<true>: v[k] + 0
    "toff-inclusive",            # k_tile_prefix: toff = s + v
)
MUTANTS = RANK_MUTANTS + RLE_MUTANTS
# mutant -> why no input can tell it from the scheme
EQUIVALENT = {
    "prevc-lane63": "prevc only feeds pb of lane 0, and lane 0's head bit is `b != pb || l == 0`: true whatever pb is, so no output depends "
                    "on prevc at all.  Were lane 0 not always walked, the mutant would still change nothing: lane 63 differs from lane "
                    "nvalid - 1 only when nvalid < 64, i.e. te - i0 < 64, so i0 + 64 >= te and the group loop ends without another read of "
                    "prevc; the next tile is another wave, which starts from prevc = 256",
}

RANK_EVENTS = (tuple(f"rank-reg{j}" for j in range(4)) + tuple(f"rank-q0-reg{j}" for j in (1, 2, 3)) + tuple(f"rank-q63-reg{j}" for j in range(4)) +
               ("first-at-63", "first-at-64", "first-at-128", "first-at-192", "first-at-255", "first-in-later-tile", "rebuild-deep",
                "lane0-repeat", "tile-start-repeat", "wave-edge-run", "block-edge-run", "partial-last-group", "tile-of-one-byte", "freq-tie",
                 "all-freq-equal"))
RLE_EVENTS = (("run-over-segment", "run-starts-at-seg-last", "run-over-tile", "run-starts-at-tile-first-prev-nonzero",
                "tile-first-zero-prev-zero", "ext-chain-1", "ext-chain-3", "run-to-chunk-end", "chunk-all-zero") +
               tuple(f"run-len-2^{k}{d}" for k in range(1, 17) for d in ("-1", "", "+1")) + ("sym-256", "last-tile-partial"))
EVENTS = RANK_EVENTS + RLE_EVENTS


def _tiles(n):
    return (n + ATILE - 1) // ATILE


# ---- rank coding ---------------------------------------------------------------------------------------------------------------------
def hist(T, mut=None):
    """k_enc_hist: -> (tilecnt[nt][256], lastpos[nt][256]).  Thread x of the block loads the bytes ts + it * 256 + x, it = 0..15 (clamped
    to the chunk's last byte, masked by `valid`); wave w = x >> 6 counts on its own tables: the first lane of every set of equal valid
    bytes adds the set's size and stores the position of the set's LAST lane (a plain store: later iterations overwrite)."""
    T = np.asarray(T, dtype=np.uint8)
    n = len(T)
    nt = _tiles(n)
    tilecnt = np.zeros((nt, 256), dtype=np.int64)
    lastpos = np.full((nt, 256), -1, dtype=np.int64)
    lane = np.arange(WAVE)
    for t in range(nt):
        ts = t * ATILE
        h = np.zeros((TB // WAVE, 256), dtype=np.int64)
        lp = np.full((TB // WAVE, 256), -1, dtype=np.int64)
        for it in range(ATILE // TB):
            for w in range(TB // WAVE):
                i = ts + it * TB + w * WAVE + lane
                valid = np.ones(WAVE, dtype=bool) if mut == "hist-valid-ignored" else i < n
                if not valid.any():
                    continue
                s = T[np.minimum(i, n - 1)][valid]
                at = i[valid]
                h[w] += np.bincount(s, minlength=256)
                if mut == "lastpos-first-lane":
                    lp[w][s[::-1]] = at[::-1]                                # (repeated indices: the last assignment stays)
                else:
                    lp[w][s] = at
        tilecnt[t] = h.sum(axis=0)
        lastpos[t] = lp.max(axis=0)
    return tilecnt, lastpos


def prep(tilecnt, lastpos, mut=None):
    """k_enc_prep: -> (tilebase, prevlast, freq, bstart)"""
    nt = len(tilecnt)
    f = np.zeros(256, dtype=np.int64)
    p = np.full(256, -1, dtype=np.int64)
    tilebase = np.zeros_like(tilecnt)
    prevlast = np.zeros_like(lastpos)
    for t in range(nt):
        n = tilecnt[t]
        tilebase[t] = f + n if mut == "tilebase-inclusive" else f
        f = f + n
        prevlast[t] = p
        p = np.maximum(lastpos[t], p)
    fk, fs = f[None, :], f[:, None]
    k, s = np.arange(256)[None, :], np.arange(256)[:, None]
    more = fk >= fs if mut == "prep-ge" else fk > fs
    tie = (fk == fs) & ((k > s) if mut == "prep-tie-larger-first" else (k < s))
    bstart = np.where(more | tie, fk, 0).sum(axis=1)
    return tilebase, prevlast, f, bstart


def _heads(tile, mut):
    """the head bits of every 64-byte group of a tile: l < nvalid && (b != pb || l == 0); pb of lane 0 is prevc: 256 at the tile's start,
    then the previous group's byte at lane nvalid - 1 (mutant: lane 63, 0x100 when that lane is past the tile)"""
    tl = len(tile)
    head = np.ones(tl, dtype=bool)
    head[1:] = tile[1:] != tile[:-1]
    prevc = 256
    for i0 in range(0, tl, WAVE):
        nvalid = min(WAVE, tl - i0)
        head[i0] = (int(tile[i0]) != prevc) or mut != "lane0-not-walked"
        prevc = (int(tile[i0 + 63]) if nvalid == WAVE else 0x100) if mut == "prevc-lane63" else int(tile[i0 + nvalid - 1])
    return head


def mtf(T, tilebase, prevlast, bstart, mut=None):
    """k_enc_mtf: -> (R with STALE_RANK where nothing was written, per-head log).  The log holds, per tile, (nseen at the tile's start,
    [head positions], [ranks], [first-occurrence flags])"""
    T = np.asarray(T, dtype=np.uint8)
    n = len(T)
    R = bytearray([STALE_RANK]) * (3 * n + 2 * ATILE)
    log = []
    for t in range(_tiles(n)):
        ts = t * ATILE
        te = min(ts + ATILE, n)
        tl = te - ts
        pos = (bstart + tilebase[t]).tolist()
        # the list before the tile: every symbol with a stamp goes to position #{symbols with a later stamp}
        last = prevlast[t]
        seen = np.flatnonzero(last >= 0)
        nseen = 0 if mut == "nseen-from-zero" else len(seen)
        lst = [EMPTY] * 257
        own = last[seen]
        later = (last[None, :] >= own[:, None]) if mut == "place-ge" else (last[None, :] > own[:, None])
        for s, at in zip(seen.tolist(), later.sum(axis=1).tolist()):
            lst[at] = s
        r0, r1, r2, r3 = lst[0:64], lst[64:128], lst[128:192], lst[192:256]
        nseen0 = nseen
        tile = T[ts:te]
        hp = np.flatnonzero(_heads(tile, mut))
        gend = np.minimum((hp >> 6) * WAVE + WAVE, tl)                        # i0 + nvalid of the head's group
        nxt = np.append(hp[1:], tl)
        ext = np.minimum(nxt, gend) - hp                                      # lanes whose head this is
        run = ext.copy()                                                      # runlen: to the next head of the group, or nvalid - l
        if mut == "runlen-short":
            run[nxt >= gend] -= 1
        ranks, firsts = [], []
        tb = tile.tolist()
        for p, e, rn in zip(hp.tolist(), ext.tolist(), run.tolist()):
            cc = tb[p]
            dpos = pos[cc]
            first = False
            try:
                rank = r0.index(cc)                                           # among the first 64: the common case
            except ValueError:
                if cc in r1:
                    rank = 64 + r1.index(cc)
                elif cc in r2:
                    rank = 128 + r2.index(cc)
                elif cc in r3:
                    rank = 192 + r3.index(cc)
                else:
                    rank = nseen                                              # first occurrence in the chunk
                    nseen += 1
                    first = True
                j, q = rank >> 6, rank & 63
                m = q if mut == "part-lt" else q + 1                          # lanes l <= q move in the register holding the position
                if j >= 1:
                    c1 = EMPTY if mut == "carry1-dropped" else r0[63]
                    if j == 1:
                        r1[:m] = ([c1] + r1[:63])[:m]
                    else:
                        c2 = EMPTY if mut == "carry2-dropped" else r1[63]
                        r1 = [c1] + r1[:63]
                        if j == 2:
                            r2[:m] = ([c2] + r2[:63])[:m]
                        else:
                            c3 = EMPTY if mut == "carry3-dropped" else r2[63]
                            r2 = [c2] + r2[:63]
                            r3[:m] = ([c3] + r3[:63])[:m]
            m = min(rank if mut == "reg0-shift-lt" else rank + 1, 64)          # first register: lanes l <= rank move, cc enters at 0
            if m > 0:
                r0[:m] = ([cc] + r0[:63])[:m]
            pos[cc] = dpos + (1 if mut == "pos-plus-one" else rn)
            assert 0 <= dpos and dpos + e <= len(R)
            R[dpos] = rank & 0xFF
            if e > 1:
                R[dpos + 1: dpos + e] = bytes(e - 1)                          # repeats: rank 0, right behind their head
            ranks.append(rank)
            firsts.append(first)
        log.append((nseen0, hp, np.array(ranks, dtype=np.int64), np.array(firsts, dtype=bool)))
    return np.frombuffer(bytes(R), dtype=np.uint8), log


def rank_events(T, freq, log):
    """event -> how often the text reaches it"""
    T = np.asarray(T, dtype=np.uint8)
    n = len(T)
    ev = dict.fromkeys(RANK_EVENTS, 0)
    for t, (nseen0, hp, ranks, firsts) in enumerate(log):
        ts = t * ATILE
        tl = min(ATILE, n - ts)
        found = ~firsts
        for j in range(4):
            ev[f"rank-reg{j}"] += int((found & (ranks >> 6 == j)).sum())
            ev[f"rank-q63-reg{j}"] += int((found & (ranks == 64 * j + 63)).sum())
            if j:
                ev[f"rank-q0-reg{j}"] += int((found & (ranks == 64 * j)).sum())
        for v in (63, 64, 128, 192, 255):
            ev[f"first-at-{v}"] += int((firsts & (ranks == v)).sum())
        if t > 0:
            ev["first-in-later-tile"] += int(firsts.sum())
            ev["rebuild-deep"] += int(nseen0 > 192 and bool(found[0]) and int(ranks[0]) >= 64)
            if T[ts] == T[ts - 1] and ranks[0] == 0 and not firsts[0]:            # rank 0 from the rebuilt list
                ev["tile-start-repeat"] += 1
                ev["block-edge-run" if (t - 1) % 4 == 3 else "wave-edge-run"] += 1
        g0 = hp[(hp & 63 == 0) & (hp > 0)]
        ev["lane0-repeat"] += int((T[ts + g0] == T[ts + g0 - 1]).sum())
        ev["partial-last-group"] += int(tl % WAVE != 0)
        ev["tile-of-one-byte"] += int(tl == 1)
    f = np.asarray(freq)
    nz = np.sort(f[f > 0])
    ev["freq-tie"] = int((nz[1:] == nz[:-1]).sum())
    ev["all-freq-equal"] = int(len(nz) == 256 and nz[0] == nz[-1])
    return ev


def rank_front(T, mut=None):
    """-> (R: the chunk's n ranks and, behind them, whatever landed outside -- STALE_RANK where nothing did; freq; events)"""
    assert mut is None or mut in RANK_MUTANTS, mut
    tilecnt, lastpos = hist(T, mut)
    tilebase, prevlast, freq, bstart = prep(tilecnt, lastpos, mut)
    R, log = mtf(T, tilebase, prevlast, bstart, mut)
    return R, freq.astype(np.int32), rank_events(T, freq, log)


# ---- RLE0 ------------------------------------------------------------------------------------------------------------------------------
def _bit_length(x):
    x = np.asarray(x, dtype=np.int64).copy()
    n = np.zeros(x.shape, dtype=np.int64)
    while (x > 0).any():
        n += x > 0
        x >>= 1
    return n


def rle_front(R, mut=None):
    """-> (symbols uint16[rlen], rlen, the tables (lz, ext, tcount, toff))"""
    assert mut is None or mut in RLE_MUTANTS, mut
    R = np.asarray(R, dtype=np.uint8)
    n = len(R)
    nt = _tiles(n)
    src = np.zeros(nt * ATILE, dtype=np.int64)
    src[:n] = R
    tl = np.minimum(ATILE, n - np.arange(nt) * ATILE)                          # [tile]
    pin = np.arange(ATILE).reshape(1, TB, SEG)                                 # p0 + k
    ok = pin < tl[:, None, None]
    v = np.where(ok, src.reshape(nt, TB, SEG), 1)
    nz = ok & (v != 0)
    # k_rle_lz: thread x looks at the bytes k * 256 + x; the block's minimum
    strided = np.where(nz.reshape(nt, ATILE), np.arange(ATILE)[None, :], INF).reshape(nt, ATILE // TB, TB)
    lz = np.minimum(strided.min(axis=1).min(axis=1), tl)
    # k_rle_ext: zeros that follow the end of tile t without interruption
    ext = np.zeros(nt, dtype=np.int64)
    e = 0
    for t in range(nt - 1, -1, -1):
        ext[t] = e
        z = int(lz[t])
        if mut == "ext-no-chain":
            e = z
        elif mut == "ext-over-full-only":
            e = z + e if z == tl[t] else 0
        else:
            e = z + e if z == tl[t] else z
    # k_rle_tiles: thread x owns the bytes [16 x, 16 x + 16)
    first = np.where(nz, pin, INF).min(axis=2)                                 # [tile, thread]
    after = np.full((nt, TB), INF, dtype=np.int64)                             # exclusive suffix minimum over the threads
    after[:, :-1] = np.minimum.accumulate(first[:, ::-1], axis=1)[:, ::-1][:, 1:]
    behind = tl if mut == "after-without-ext" else tl + ext
    after = np.where(after == INF, behind[:, None], after)
    nxt = np.zeros((nt, TB, SEG), dtype=np.int64)                              # next non-zero position behind every byte of the segment
    nn = after.copy()
    for k in range(SEG - 1, -1, -1):
        nxt[:, :, k] = nn
        nn = np.where(nz[:, :, k], pin[:, :, k], nn)
    p0 = pin[:, :, 0] + np.zeros((nt, 1), dtype=np.int64)
    ts = (np.arange(nt) * ATILE)[:, None]
    before = np.where(ts + p0 > 0, src[np.maximum(ts + p0 - 1, 0)], STALE_BEFORE)     # src[p0 - 1]
    prev = np.where(p0 - 1 < tl[:, None], before, 1)
    start_prev = before[:, 0].copy()
    if mut != "prev-at-chunk-start-src":
        start_prev[0] = 1
    if mut == "prev-at-tile-start-one":
        start_prev[:] = 1
    prev[:, 0] = start_prev
    pv = np.concatenate((prev[:, :, None], v[:, :, :-1]), axis=2)              # the byte before (valid bytes are a prefix of the tile)
    runstart = ok & (v == 0) & (pv != 0)
    rs = np.flatnonzero(runstart.ravel())
    pflat = np.broadcast_to(pin, (nt, TB, SEG)).ravel()
    L = nxt.ravel()[rs] - pflat[rs] + 1
    cnt_e = nz.astype(np.int64).ravel()
    cnt_e[rs] = _bit_length(L) - 1                                             # 31 - clz(L)
    cnt = cnt_e.reshape(nt, TB, SEG).sum(axis=2)
    incl = np.cumsum(cnt, axis=1)
    tcount = incl[:, -1]
    # k_tile_prefix
    toff = np.zeros(nt, dtype=np.int64)
    s = 0
    for t in range(nt):
        toff[t] = s + int(tcount[t]) if mut == "toff-inclusive" else s
        s += int(tcount[t])
    rlen = s
    # k_rle_tiles<true>
    Le = L - 1 if mut == "L-without-plus-one" else L
    top = _bit_length(Le) - 2 + {"digits-one-more": 1, "digits-one-less": -1}.get(mut, 0)      # the first b of the digit loop
    em_e = nz.astype(np.int64).ravel()
    em_e[rs] = np.maximum(top + 1, 0)
    em = em_e.reshape(nt, TB, SEG)
    off = ((toff[:, None] + incl - cnt)[:, :, None] + np.cumsum(em, axis=2) - em).ravel()
    out = np.full(rlen + n + 64, STALE_SYM, dtype=np.uint16)
    off = np.clip(off, 0, len(out) - 32)
    nzf = nz.ravel()
    out[off[nzf]] = v.ravel()[nzf] + (0 if mut == "sym-plus-zero" else 1)
    offr = off[rs]
    for d in range(int(top.max()) + 1 if len(top) else 0):
        m = top >= d
        b = np.full(int(m.sum()), d) if mut == "digits-lsb-first" else top[m] - d
        out[offr[m] + d] = (Le[m] >> b) & 1
    return out[:rlen].copy(), rlen, (lz, ext, tcount, toff)


def rle_events(R):
    R = np.asarray(R, dtype=np.uint8)
    n = len(R)
    ev = dict.fromkeys(RLE_EVENTS, 0)
    z = np.concatenate(([0], (R == 0).astype(np.int8), [0]))
    d = np.diff(z)
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)                     # runs [s, e)
    ln = e - s
    ev["run-over-segment"] = int((s // SEG != (e - 1) // SEG).sum())
    ev["run-starts-at-seg-last"] = int(((s % SEG == SEG - 1) & (ln >= 2)).sum())
    ev["run-over-tile"] = int((s // ATILE != (e - 1) // ATILE).sum())
    ev["run-starts-at-tile-first-prev-nonzero"] = int(((s % ATILE == 0) & (s > 0)).sum())
    ev["tile-first-zero-prev-zero"] = int(((e - 1) // ATILE - s // ATILE).sum())
    # whole zero tiles (the chunk's partial last tile counts when it is all zero) behind the tile the run starts in: what ext[] chains
    whole = np.where(e == n, _tiles(n), e // ATILE) - (s // ATILE + 1)
    ev["ext-chain-1"] = int((whole == 1).sum())
    ev["ext-chain-3"] = int((whole == 3).sum())
    ev["run-to-chunk-end"] = int((e == n).sum())
    ev["chunk-all-zero"] = int(len(s) == 1 and s[0] == 0 and e[0] == n)
    for k in range(1, 17):
        for dd, name in ((-1, "-1"), (0, ""), (1, "+1")):
            ev[f"run-len-2^{k}{name}"] = int((ln == (1 << k) + dd).sum())
    ev["sym-256"] = int((R == 255).sum())
    ev["last-tile-partial"] = int(n % ATILE != 0)
    return ev


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def chunks(t):
    t = np.asarray(t, dtype=np.uint8)
    return [t[a: a + CHUNK] for a in range(0, len(t), CHUNK)]


def noise_runs(n, seed, alphabet=256, mean_run=3, long_every=97, long_run=150):
    """seeded noise over `alphabet` symbols with runs: geometric run lengths, every long_every-th run a long one"""
    rng = np.random.default_rng(seed)
    k = n // 2 + 16
    sym = rng.integers(0, alphabet, k)
    ln = rng.geometric(1.0 / mean_run, k)
    ln[::long_every] = long_run
    return np.repeat(sym, ln)[:n].astype(np.uint8)


def _perm(seed):
    return np.random.default_rng(seed).permutation(256).astype(np.uint8)


def round_robin(n, d, start=0):
    return ((np.arange(n) + start) % d).astype(np.uint8)


def staircase():
    """five tiles and 63 bytes over a permuted alphabet.  Tile 0 brings in symbols 0..99 (first occurrences at nseen 63 and 64), tile 1
    100..149 (128), tile 2 150..219 (192), tile 3 220..255 (255) beside a cycle over 80 old ones; tile 4 starts, with all 256 seen, on a
    symbol that tile 3 left at least 64 deep, and walks 200 symbols round robin"""
    pm = _perm(5)
    parts = []
    for lo, hi, old in ((0, 100, 0), (100, 150, 40), (150, 220, 10), (220, 256, 80)):
        new = np.arange(lo, hi)
        cyc = np.concatenate((new, np.arange(old)[::-1]))                     # the new ones in order, then `old` old ones
        tile = np.resize(cyc, ATILE)
        tile[len(cyc): len(cyc) + 200] = np.repeat(new[:20], 10)              # a few runs
        parts.append(tile)
    parts.append((np.arange(ATILE + 63) * 7 + 90) % 200 + 0)                  # 90 is not among tile 3's symbols (220..255, 0..79)
    return pm[np.concatenate(parts)]


def _filler(n, seed, avoid):
    """n bytes without two equal neighbours over 70 symbols (ranks up to 69), none of them `avoid`"""
    rng = np.random.default_rng(seed)
    t = (np.cumsum(rng.integers(1, 70, n)) % 70 + 100).astype(np.uint8)
    assert avoid not in t
    return t


def _place_runs(n, runs, seed):
    """filler with the runs (start, length, byte) laid over it; a run's neighbours differ from its byte"""
    t = _filler(n, seed, 0)
    for a, ln, b in runs:
        assert a + ln <= n and not (t[a - 1] == b or (a + ln < n and t[a + ln] == b))
        t[a: a + ln] = b
    return t


def runs_at_edges():
    """runs of 63, 4096, 4097, 64, 65 and 4095 bytes starting at offsets 63, 4095, 4095, 1, 4095 and 4095 of their tiles; the run of 65
    crosses the edge 3|4 (a block edge of k_enc_mtf), the others' edges lie inside a block"""
    runs = ((63, 63, 1), (4095, 4096, 2), (4096 + 4095, 4097, 3), (3 * 4096 + 1, 64, 4), (3 * 4096 + 4095, 65, 5), (4 * 4096 + 4095, 4095, 6))
    return _place_runs(6 * ATILE - 1, runs, 21)


def runs_at_edges_long():
    """one run of 3 * 4096 bytes from offset 4095 of tile 1: over the edges 1|2, 2|3 and 3|4 (the last one a block edge of k_enc_mtf)"""
    return _place_runs(5 * ATILE + 63, ((4096 + 4095, 3 * 4096, 7), (1, 63, 8)), 22)


SHUFFLED_LENS = (4095, 4096, 4097, 4 * 4096, 4 * 4096 + 1, 5 * 4096 + 63)
RR = (64, 65, 128, 129, 192, 193, 256)


@functools.lru_cache(maxsize=None)
def case(name):
    """the named text as a read-only uint8 array"""
    if name == "rr-256-exact":
        t = _perm(6)[round_robin(2 * ATILE, 256)]
    elif name.startswith("rr-"):
        d = int(name[3:])
        t = _perm(d)[round_robin(3 * ATILE + 17, d)]
    elif name == "staircase":
        t = staircase()
    elif name == "runs-at-edges":
        t = runs_at_edges()
    elif name == "runs-at-edges-long":
        t = runs_at_edges_long()
    elif name == "shuffled-256":
        t = noise_runs(3 * ATILE + 1000, 31)
    elif name.startswith("shuffled-256-"):
        n = int(name.split("-")[2])
        t = noise_runs(n, 32 + n % 7)
    else:
        raise KeyError(name)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    t.setflags(write=False)
    return t


CASES = (tuple(f"rr-{d}" for d in RR) + ("rr-256-exact", "staircase", "runs-at-edges", "runs-at-edges-long", "shuffled-256") +
         tuple(f"shuffled-256-{n}" for n in SHUFFLED_LENS))

LADDER = tuple(range(1, 41)) + tuple((1 << k) + d for k in range(6, 17) for d in (-1, 0, 1))
ALL_ZERO = (1, 15, 16, 17, 4096, 4097, 3 * 4096, 1 << 20, (1 << 20) + 1)


def ladder(shift=0):
    """`shift` non-zero bytes, then zero runs of every length in LADDER, each followed by one non-zero byte that cycles through 1..255"""
    parts = [np.arange(shift) % 255 + 1]
    for i, ln in enumerate(LADDER):
        parts += [np.zeros(ln, dtype=np.int64), np.array([i % 255 + 1])]
    return np.concatenate(parts)


def whole_tiles():
    """zero runs over exactly 1 and exactly 3 tiles, and each of them one byte short and one byte long at either end, between tiles of
    non-zero bytes that cycle through 1..255"""
    parts = []
    for k in (1, 3):
        for da, db in ((0, 0), (1, 0), (-1, 0), (0, -1), (0, 1)):
            seg = np.arange((k + 2) * ATILE) % 255 + 1
            seg[ATILE + da: (k + 1) * ATILE + db] = 0
            parts.append(seg)
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def ranks(name):
    """the named byte array for the RLE0 probe (any bytes: it need not be a rank array)"""
    if name == "ladder":
        r = ladder()
    elif name.startswith("ladder+"):
        r = ladder(int(name[7:]))
    elif name == "whole-tiles":
        r = whole_tiles()
    elif name.startswith("all-zero-"):
        r = np.zeros(int(name[9:]))
    elif name == "zero-at-last-byte":
        r = np.arange(ATILE + 1) % 255 + 1
        r[-1] = 0
    elif name == "only-255":
        r = np.full(ATILE + SEG, 255)
    else:
        raise KeyError(name)
    r = np.ascontiguousarray(r, dtype=np.uint8)
    r.setflags(write=False)
    return r


RANKS = ("ladder", "ladder+1", "ladder+15", "ladder+4095", "whole-tiles") + tuple(f"all-zero-{n}" for n in ALL_ZERO) + ("zero-at-last-byte", "only-255")


def _few(n, seed):
    """n bytes of long runs over eight frequent symbols (10..17): every one of them far more frequent than a visitor"""
    return noise_runs(n, seed, alphabet=8, mean_run=40, long_every=13, long_run=700) + 10


@functools.lru_cache(maxsize=None)
def image(name):
    """product path: more than one 1 MiB chunk"""
    if name == "edge-zeros":
        # chunk one ends in three whole tiles (and two bytes) of byte 200, its least frequent symbol: the bucket of 200 is the last one
        # of the rank array, one head and 3 * 4096 + 1 zeros from offset 4095 of a tile to the chunk's end.  Chunk two begins with 200
        tail = 3 * ATILE + 2
        t = np.concatenate((_few(CHUNK - tail, 41), np.full(tail + 2500, 200), _few(1533, 42)))
    elif name == "ragged-1":
        t = np.concatenate((_few(CHUNK - 9000, 43), noise_runs(9000, 44), [77]))
    elif name == "ragged-4097":
        t = np.concatenate((_few(CHUNK - 9000, 45), noise_runs(9000 + ATILE + 1, 46)))
    elif name == "rr-193-split":
        t = np.concatenate((_few(CHUNK - 2 * ATILE - 100, 47), _perm(8)[round_robin(2 * ATILE + 100 + 4000, 193, start=50)]))
    else:
        raise KeyError(name)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    t.setflags(write=False)
    return t


IMAGES = ("edge-zeros", "ragged-1", "ragged-4097", "rr-193-split")
# image -> per chunk (rank-coder events of the chunk's text, RLE0 events of the chunk's rank array) that the chunk must reach
IMAGE_REACH = {
    "edge-zeros": ((("tile-start-repeat", "wave-edge-run", "block-edge-run", "lane0-repeat"), ("ext-chain-3", "run-to-chunk-end", "run-over-tile")),
                   (("lane0-repeat", "partial-last-group"), ("run-over-segment", "last-tile-partial"))),
    "ragged-1": ((("first-in-later-tile", "lane0-repeat"), ("run-over-tile", "run-over-segment")),
                 (("tile-of-one-byte", "partial-last-group"), ("chunk-all-zero", "run-to-chunk-end", "last-tile-partial"))),
    "ragged-4097": ((("first-in-later-tile", "rank-reg1", "rank-reg2"), ("run-over-tile", "run-over-segment")),
                    (("tile-of-one-byte", "rank-reg1", "first-at-64"), ("last-tile-partial", "run-over-segment"))),
    "rr-193-split": ((("rank-q0-reg3", "first-in-later-tile", "first-at-192"), ("run-over-tile",)),
                     (("rank-q0-reg3", "first-at-63", "first-at-64", "first-at-128", "first-at-192", "partial-last-group"), ("last-tile-partial",))),
}

GROUP_IMAGE_LENS = (4095, 4096, 4097, 8192, 3 * 4096 + 1, 70_001)


@functools.lru_cache(maxsize=None)
def group():
    """twelve block texts whose BWT images (n + TRAILER bytes) have the lengths GROUP_IMAGE_LENS: one-valued, then rr-193"""
    out = []
    for m in GROUP_IMAGE_LENS:
        n = m - TRAILER
        for t in (np.full(n, 0x41, dtype=np.uint8), _perm(9)[round_robin(n, 193)]):
            t.setflags(write=False)
            out.append(t)
    return tuple(out)
