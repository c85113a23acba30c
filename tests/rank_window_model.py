"""k_enc_mtf (ans_enc_front.hip) restated in plain Python: the rank of every run head counted in its own window, tile by tile with the
kernel's own tables -- and the crafted inputs that reach its edges.  No GPU code is imported.

enc_front_model.py stays as it is: it restates the SERIAL scheme the kernel had before (one recency list per tile, walked head by head),
which computes the same bytes and still passes on the CPU (test_enc_front_model.py); its hist() and prep() are k_enc_hist and k_enc_prep,
which did not change, and are used here as they are.

The scheme, for one tile, in the index space of its run heads (a repeat has rank 0 and lands right behind its head in the same bucket):
  heads(tile)         head positions, their symbols and run lengths; a tile's first byte is a head whatever stands before it
  sort_by_symbol(hs)  one stable counting sort of the heads by symbol -> P(k), the previous head of head k's symbol (-1: none in the
                      tile), N(j), the next head of head j's symbol (INF: none), and -- a segmented prefix of the run lengths in
                      the sorted order -- the bytes of the symbol in the tile before head k
  in_tile(P, N)       #{ j : P(k) < j < k and N(j) >= k }: each distinct symbol of the window counted once, at its last head there
  carried(...)        only for a symbol's first head in the tile: the symbols s with no head in the tile before k and
                      stamp[s] > stamp[c] (prevlast: -1 = not seen in the chunk, so a symbol new to the chunk gets the number of distinct
                      symbols seen so far, the first-occurrence rule of the reference)
  write position      bstart[c] + tilebase[c] + the bytes of c in the tile before the head
tile_by_sort() is that definition.  tile_by_groups() is how the kernel gets the same numbers without sorting: 64-byte groups, one wave
match per group for the positions and for P (the nearest equal head below in the group, else the table lasth), nx[] filled as the
groups go (nx[k] = INF, nx[P(k)] = k), the window counted in three parts: RW_CAP positions from the head's own lane, the rest in steps of
64 by the wave, first heads by a counter plus the stamp compare.  The test holds the two against each other and against a plain one-list
MTF (plain_rank_encode)."""
import functools

import numpy as np

import enc_front_model as F

ATILE = F.ATILE
WAVE = F.WAVE
RW_CAP = 32
NONE = 0x7FFF                    # lasth: no head of the symbol yet; nx: no later head of the symbol so far
INF = 1 << 30
STALE_RANK = F.STALE_RANK


# ---- the plain algorithm ----------------------------------------------------------------------------------------------------------
def plain_rank_encode(T):
    """one recency list, one pass (rank.cpp:45-90): -> (R, freq).  Buckets in descending frequency, ties -> smaller symbol first"""
    T = np.asarray(T, dtype=np.uint8)
    freq = np.bincount(T, minlength=256)
    order = sorted(range(256), key=lambda s: (-int(freq[s]), s))
    pos = [0] * 256
    at = 0
    for s in order:
        pos[s] = at
        at += int(freq[s])
    R = bytearray(len(T))
    lst = []
    for c in T.tolist():
        if lst and lst[0] == c:
            r = 0
        elif c in lst:
            r = lst.index(c)
            del lst[r]
            lst.insert(0, c)
        else:
            r = len(lst)
            lst.insert(0, c)
        R[pos[c]] = r
        pos[c] += 1
    return np.frombuffer(bytes(R), dtype=np.uint8), freq.astype(np.int32)


# ---- the definition: one stable sort of the tile's heads by symbol ----------------------------------------------------------------------
def heads(tile):
    """-> (positions of the heads, their symbols, their run lengths)"""
    tile = np.asarray(tile, dtype=np.int64)
    h = np.ones(len(tile), dtype=bool)
    h[1:] = tile[1:] != tile[:-1]
    hp = np.flatnonzero(h)
    return hp, tile[hp], np.diff(np.append(hp, len(tile)))


def sort_by_symbol(hs, run):
    """-> (P, N, bytes of the head's symbol in the tile before it)"""
    nh = len(hs)
    order = np.argsort(hs, kind="stable")
    ss = hs[order]
    same = ss[1:] == ss[:-1]                                                   # sorted slot i + 1 continues slot i's symbol
    P = np.full(nh, -1, dtype=np.int64)
    N = np.full(nh, INF, dtype=np.int64)
    P[order[1:][same]] = order[:-1][same]
    N[order[:-1][same]] = order[1:][same]
    rs = run[order]
    excl = np.cumsum(rs) - rs
    seg = np.flatnonzero(np.concatenate(([True], ~same)))                      # first slot of every symbol
    base = np.repeat(excl[seg], np.diff(np.append(seg, nh)))
    before = np.zeros(nh, dtype=np.int64)
    before[order] = excl - base
    return P, N, before


def in_tile(P, N):
    return np.array([int((N[P[k] + 1: k] >= k).sum()) for k in range(len(P))], dtype=np.int64)


def carried(hs, P, stamp):
    """for the heads with P = -1 (else 0): #{ s : no head of s in the tile before k and stamp[s] > stamp[c] }"""
    out = np.zeros(len(hs), dtype=np.int64)
    first = np.full(256, INF, dtype=np.int64)                                  # every symbol's first head in the tile
    fk = np.flatnonzero(P < 0)
    first[hs[fk]] = fk
    for k in fk.tolist():
        out[k] = int(((first > k) & (stamp > stamp[hs[k]])).sum())
    return out


def tile_by_sort(tile, stamp):
    """-> (head positions, run lengths, ranks, bytes-before, window lengths k - P - 1 of the heads that have a P)"""
    hp, hs, run = heads(tile)
    P, N, before = sort_by_symbol(hs, run)
    rank = in_tile(P, N) + carried(hs, P, stamp)
    k = np.arange(len(hs))
    return hp, hs, run, rank, before, (k - P - 1)[P >= 0]


# ---- the kernel's way: 64-byte groups ---------------------------------------------------------------------------------------------------
def tile_by_groups(tile, stamp, pos, log=None):
    """k_enc_mtf on one tile: `pos` (bstart + tilebase of the tile, a list) advances; -> [(write position, rank or 0)] of every byte.
    `log` collects, per head with a window, (positions tested from the own lane, steps of 64 by the wave)"""
    tb = np.asarray(tile, dtype=np.int64).tolist()
    tl = len(tb)
    nx = np.full(ATILE + 64, 0xEEEE, dtype=np.int64)                           # stale until a head writes its slot
    lasth = [NONE] * 256
    last = [int(v) for v in stamp]                                             # the four stamp registers
    out = []
    prevc, hb, nfirst = 256, 0, 0
    for i0 in range(0, tl, WAVE):
        b = tb[i0: i0 + WAVE]
        nvalid = len(b)
        ishead = [b[l] != (prevc if l == 0 else b[l - 1]) for l in range(nvalid)]
        k, P, dp = [0] * nvalid, [0] * nvalid, [0] * nvalid
        lh = [lasth[s] for s in b]                                            # the table as it stands in front of the group
        p0 = [pos[s] for s in b]
        same, below, nheads = {}, {}, 0                                       # per symbol: equal lanes below, the nearest equal head below
        for l in range(nvalid):
            s = b[l]
            dp[l] = p0[l] + same.get(s, 0)                                    # popcount(m & lt)
            same[s] = same.get(s, 0) + 1
            k[l] = hb + nheads                                                # hb + popcount(heads & lt)
            P[l] = below[s] if s in below else (-1 if lh[l] == NONE else lh[l])
            if ishead[l]:
                below[s] = k[l]
                nheads += 1
        for l in range(nvalid):                                               # (ascending lanes: the last lane of each set stays)
            pos[b[l]] = dp[l] + 1
            if ishead[l]:
                lasth[b[l]] = k[l]
        for l in range(nvalid):
            if ishead[l]:
                nx[k[l]] = NONE
        for l in range(nvalid):
            if ishead[l] and P[l] >= 0:
                nx[P[l]] = k[l]
        cnt = [0] * nvalid
        for l in range(nvalid):
            if not (ishead[l] and P[l] >= 0):
                continue
            own = 0
            for s in range(1, RW_CAP + 1):                                    # from the head's own lane
                j = k[l] - s
                if j > P[l]:
                    own += 1
                    cnt[l] += nx[j] >= k[l]
            steps = 0
            hi = k[l] - RW_CAP
            for j0 in range(P[l] + 1, max(hi, P[l] + 1), WAVE):               # the rest, 64 positions a step
                steps += 1
                cnt[l] += int((nx[j0: min(j0 + WAVE, hi)] >= k[l]).sum())     # lanes with j < hi
            if log is not None:
                log.append((own, steps))
        for l in range(nvalid):                                               # first heads, in order
            if ishead[l] and P[l] < 0:
                own = last[b[l]]
                assert own >= -1
                cnt[l] = nfirst + sum(1 for v in last if v > own)
                nfirst += 1
                last[b[l]] = -2
        out += [(dp[l], cnt[l] if ishead[l] else 0) for l in range(nvalid)]
        hb += sum(ishead)
        prevc = b[-1]
    return out


# ---- a chunk ----------------------------------------------------------------------------------------------------------------------------
def rank_window(T, how="groups", stats=None):
    """one chunk through k_enc_hist, k_enc_prep (enc_front_model) and the window scheme: -> (R: the n ranks and behind them whatever landed
    outside, STALE_RANK where nothing was written; freq).  how: "groups" (the kernel's way) or "sort" (the definition)"""
    T = np.asarray(T, dtype=np.uint8)
    n = len(T)
    tilebase, prevlast, freq, bstart = F.prep(*F.hist(T))
    R = bytearray([STALE_RANK]) * (n + ATILE)
    for t in range((n + ATILE - 1) // ATILE):
        tile = T[t * ATILE: (t + 1) * ATILE]
        base = bstart + tilebase[t]
        if how == "sort":
            hp, hs, run, rank, before, win = tile_by_sort(tile, prevlast[t])
            if stats is not None:
                stats.append(win)
            for c, ln, r, bf in zip(hs.tolist(), run.tolist(), rank.tolist(), before.tolist()):
                at = int(base[c]) + bf
                assert 0 <= at and at + ln <= len(R)
                R[at] = r
                R[at + 1: at + ln] = bytes(ln - 1)
        else:
            for at, r in tile_by_groups(tile, prevlast[t], base.tolist(), stats):
                assert 0 <= at < len(R)
                R[at] = r
    return np.frombuffer(bytes(R), dtype=np.uint8), freq.astype(np.int32)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def bwt_like(text):
    """the last column of the sorted rotations of `text` (prefix doubling): runs and short windows, as a BWT image has them"""
    t = np.asarray(text, dtype=np.int64)
    n = len(t)
    rank = t.copy()
    h = 1
    while True:
        key2 = np.roll(rank, -h)
        order = np.lexsort((key2, rank))
        r1, r2 = rank[order], key2[order]
        new = np.zeros(n, dtype=np.int64)
        new[order] = np.cumsum(np.concatenate(([0], (r1[1:] != r1[:-1]) | (r2[1:] != r2[:-1]))))
        rank = new
        if rank.max() == n - 1 or h >= n:
            break
        h *= 2
    sa = np.argsort(rank, kind="stable")
    return t[(sa - 1) % n].astype(np.uint8)


def text(n, seed):
    """English-like filler: words drawn from a small vocabulary with a skewed distribution"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz", dtype=np.uint8)
    vocab = [bytes(rng.choice(letters[: 6 + i % 20], 2 + i % 7)) for i in range(300)]
    w = rng.zipf(1.3, n // 3 + 8) % len(vocab)
    return np.frombuffer(b" ".join(vocab[i] for i in w)[:n], dtype=np.uint8)


LENGTHS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)


def _window_three_tiles():
    """symbol 200 once in tile 0 and again at the last byte of tile 3; between them 70 other symbols without equal neighbours"""
    t = F._filler(4 * ATILE + 100, 51, 200).copy()
    t[1000] = 200
    t[4 * ATILE - 1] = 200
    return t


def _carried_ties():
    """all 256 symbols come in in tile 0; tile 1 touches a hundred of them in a shuffled order; tile 2 opens with all 256 in reverse order (every one a first head
    whose rank comes from the stamps), then runs of a few"""
    t0 = np.arange(ATILE) % 256
    t1 = np.resize(np.random.default_rng(52).permutation(256)[:100], ATILE)
    t2 = np.concatenate((np.arange(255, -1, -1), np.repeat(np.arange(40) * 5 % 256, 96)))
    return np.concatenate((t0, t1, t2))


@functools.lru_cache(maxsize=None)
def case(name):
    """the named text as a read-only uint8 array"""
    if name.startswith("len-"):
        n = int(name[4:])
        t = F.noise_runs(n, 60 + n % 11, alphabet=90)
    elif name == "one-symbol":
        t = np.full(3 * ATILE + 5, 0x41)
    elif name == "alternating":
        t = np.arange(2 * ATILE + 3) % 2 + 7
    elif name == "cycle-256":
        t = np.arange(5 * ATILE) % 256
    elif name == "carried-ties":
        t = _carried_ties()
    elif name == "window-three-tiles":
        t = _window_three_tiles()
    elif name == "lds-worst":
        t = np.arange(2 * ATILE + 1) * 7 % 256
    elif name == "random":
        t = np.random.default_rng(7).integers(0, 256, 3 * ATILE)
    elif name == "runs-at-edges":
        t = F.case("runs-at-edges")
    elif name == "two-chunks":
        t = bwt_like(text(F.CHUNK + ATILE + 1, 3))
    elif name == "bwt-text":
        t = bwt_like(text(64 << 10, 4))
    else:
        raise KeyError(name)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    t.setflags(write=False)
    return t


CASES = (tuple(f"len-{n}" for n in LENGTHS) + ("one-symbol", "alternating", "cycle-256", "carried-ties", "window-three-tiles", "lds-worst",
                                               "random", "runs-at-edges", "bwt-text"))
TWO_CHUNKS = "two-chunks"        # 1 MiB + 4097 bytes: through the product path, where the second chunk's stamps restart
ALPHABETS = (1, 2, 3, 64, 65, 255, 256)


def random_short(i):
    """the i-th random short text: alphabet ALPHABETS[i % 7], every third one up to two tiles and a bit, with and without runs"""
    rng = np.random.default_rng(1000 + i)
    a = ALPHABETS[i % len(ALPHABETS)]
    n = int(rng.integers(1, 300)) if i % 3 else int(rng.integers(300, 2 * ATILE + 200))
    sym = rng.permutation(256)[:a]
    if i % 2:
        t = sym[rng.integers(0, a, n)]
    else:
        t = np.repeat(sym[rng.integers(0, a, n)], rng.geometric(0.4, n))[:n]
    return t.astype(np.uint8)
