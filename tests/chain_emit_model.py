"""The back half of ans_enc_chain.hip restated in plain Python: what k_pairs pads, what k_rans_lanes leaves behind, and how k_emit_count ->
k_emit_prefix -> k_put_payload turn that into the payload bytes -- and the crafted inputs that reach its index edges.  No GPU code is
imported; the functions that need the oracle take it as an argument.

Every index edge of the stage is a function of one number per chunk: rlen, the chunk's count of RLE0 symbols (np = 2 rlen pairs: pair
2 t is symbol t's exponent, pair 2 t + 1 its mantissa; pair j belongs to chain j & 3 and is that chain's step j >> 2).  A text without two
equal neighbouring bytes has rlen == len (only the chunk's first byte has rank 0, and a single zero is one symbol), so rlen is pinned by
construction; test_chain_emit_model.py confirms every one with the oracle.

  emits(pairs)    the sequential walk (four states, last pair first): bytes emitted per pair, the low 16 bits of the state each step started
                  from, the four final states
  layout(np)      per chain: steps, identity steps; steps_pad, batches, nbatch, emit tiles, windows
  place(pairs)    the chain's lane-major leftovers (16-bit states, one mask word per batch of sixteen steps) and the three emit kernels on
                  them -> (csize, payload bytes behind the sixteen state bytes).  Memory nobody wrote holds STALE values, so that a read one
                  past the written words shows.  `mut` names ONE changed token of the scheme (MUTANTS)
  record(lo, fr)  rans_record with 32-bit arithmetic only (numpy uint32, vectorised over fr)
  reach(pairs)    named events of the scheme the pairs reach
  CASES / IMAGES / GROUP   the inputs

Mutants that cannot change a byte (EQUIVALENT, with the reason) are kept: the test asserts that they change none."""
import functools

import numpy as np

CHUNK = 1 << 20
ETILE = 4096                     # pairs per emit tile
RANS_L = 1 << 23
PAD = 256                        # a chain is padded to whole rounds of the sixteen-batch ring
PAD_SPAN = 288                   # identity records k_pairs can write per chain
WINDOW = 64                      # tiles per window of k_emit_prefix
TB = 256
STALE_REC = (0x0BAD, 5)          # (low, freq) of a record nobody wrote
STALE_MASK = 0xFFFFFFFF
STALE_X16 = 0xA5C3
STALE_SUM = 0x00ABCDEF
STALE_BYTE = 0xEE

MUTANTS = (
    "bit-order",                 # k_put_payload: bit step & 15 instead of 15 - (step & 15)
    "bytes-swapped",             # k_put_payload: the two bytes of a two-byte emit in the other order
    "count-live+1", "count-live-1",      # k_emit_count: w < batches + 1 / w < batches - 1
    "put-live+1", "put-live-1",          # k_put_payload: (s0 >> 4) < batches + 1 / - 1
    "tile-test-late",            # both emit kernels return one tile too early: (tile + 1) * ETILE >= np
    "carry-dropped",             # k_emit_prefix: ts[t] = inc - v
    "suffix-inclusive",          # k_emit_prefix: ts[t] = carry + inc
    "first-without-chain",       # k_pairs: first = ((np - 1) >> 2) + 1 for every chain
    "steps-pad-down",            # k_pairs: steps_pad rounded down to a multiple of 256
    "pad-bits-kept",             # the chain's pad steps leave a set bit in the mask word
    # equivalent ones
    "halves-swapped",            # low half "two", high half "one at least"
    "count-tile-test->", "put-tile-test->",      # tile * ETILE > np
)
# mutant -> why no input can tell it from the scheme
EQUIVALENT = {
    "halves-swapped": "k_emit_count takes the population count of the whole word and k_put_payload adds the two bits of a step: neither tells "
                      "the halves apart, whichever side swaps them",
    "count-tile-test->": "the one more tile that runs (np a multiple of 4096) lies inside the launched grid, finds w >= batches in every "
                         "thread and stores a sum of 0 that k_emit_prefix (nt tiles) never reads",
    "put-tile-test->": "the one more tile that runs finds live false in every thread (its first step is 16 * batches) and places nothing",
}


# ---- the reference walk ---------------------------------------------------------------------------------------------------------------
def emits(pairs):
    """pairs: uint32 low | freq << 16 in coding order.  -> (count per pair uint8, low 16 bits of the state the pair's step started from
    uint16, [final state of chain 0..3])"""
    p = np.asarray(pairs, dtype=np.uint32)
    n = len(p)
    lo = (p & 0xFFFF).tolist()
    fr = (p >> 16).tolist()
    cnt = bytearray(n)
    x16 = [0] * n
    R = [RANS_L] * 4
    for j in range(n - 1, -1, -1):
        x = R[j & 3]
        f = fr[j]
        xmax = f << 15
        x16[j] = x & 0xFFFF
        if x >= xmax:
            x >>= 8
            if x >= xmax:
                x >>= 8
                cnt[j] = 2
            else:
                cnt[j] = 1
        R[j & 3] = ((x // f) << 16) + x % f + lo[j]
    return np.frombuffer(bytes(cnt), dtype=np.uint8), np.array(x16, dtype=np.uint16), R


# ---- index scheme ------------------------------------------------------------------------------------------------------------------------
def rans_batches(np_):
    return ((np_ - 1) >> 2) // 16 + 1 if np_ else 0


def layout(np_, mut=None):
    """what k_pairs (first, steps_pad: `mut` applies to these), k_rans_lanes (nbatch) and the emit kernels (batches, tiles) compute from np"""
    steps = [((np_ - 1 - ch) >> 2) + 1 if ch < np_ else 0 for ch in range(4)]
    if mut == "first-without-chain":
        first = [((np_ - 1) >> 2) + 1 if ch < np_ else 0 for ch in range(4)]
    else:
        first = list(steps)
    if np_ == 0:
        steps_pad = PAD
    elif mut == "steps-pad-down":
        steps_pad = (((np_ - 1) >> 2) // PAD) * PAD
    else:
        steps_pad = (((np_ - 1) >> 2) // PAD + 1) * PAD
    nbatch = (rans_batches(np_) + 15) & ~15                                   # k_rans_lanes: whole rounds of the ring
    tiles = (np_ + ETILE - 1) // ETILE
    return {"np": np_, "steps": steps, "first": first, "steps_pad": steps_pad, "identity": [16 * nbatch - s for s in steps],
            "identity_written": [(f, max(f, min(f + PAD_SPAN, steps_pad))) for f in first],
            "batches": rans_batches(np_), "nbatch": nbatch, "tiles": tiles, "windows": (tiles + WINDOW - 1) // WINDOW}


def _walk_chain(recs, x=RANS_L):
    """one chain, highest step first.  recs[k] = (low, freq) or None for an identity record -> (count per step, x16 per step, final state)"""
    cnt, x16 = [0] * len(recs), [0] * len(recs)
    for k in range(len(recs) - 1, -1, -1):
        x16[k] = x & 0xFFFF
        if recs[k] is None:
            continue                                                           # xmax above every state, q * 0 + x + 0
        lo, f = recs[k]
        xmax = f << 15
        if x >= xmax:
            x >>= 8
            cnt[k] = 1
            if x >= xmax:
                x >>= 8
                cnt[k] = 2
        x = (((x // f) << 16) + x % f + lo) & 0xFFFFFFFF
    return cnt, x16, x


def chain_leftovers(pairs, mut=None, em=None):
    """what k_rans_lanes leaves behind: per chain the 16-bit start states of its 16 nbatch steps and nbatch mask words (bit 15 - (step & 15);
    low half: one byte at least, high half: two), in arrays whose unwritten tail is STALE; and the four final states"""
    p = np.asarray(pairs, dtype=np.uint32)
    np_ = len(p)
    lay, wr = layout(np_), layout(np_, mut)
    total = 16 * lay["nbatch"]
    stale = any(not (a <= k < b) for ch in range(4) for (a, b) in [wr["identity_written"][ch]] for k in range(lay["steps"][ch], total))
    nw = WINDOW * (lay["tiles"] + 2)                                           # words per chain in the model's arrays
    x16c = np.full((4, 16 * nw), STALE_X16, dtype=np.uint16)
    cntc = np.zeros((4, 16 * nw), dtype=np.uint8)
    R = [RANS_L] * 4
    if not stale:
        cnt, x16, R = em if em is not None else emits(p)
        for ch in range(4):
            n = lay["steps"][ch]
            x16c[ch, :n] = x16[ch::4]
            cntc[ch, :n] = cnt[ch::4]
            x16c[ch, n:total] = RANS_L & 0xFFFF                                # the pad steps are walked first, from the start state
    else:
        for ch in range(4):
            a, b = wr["identity_written"][ch]
            n = lay["steps"][ch]
            recs = [(int(v) & 0xFFFF, int(v) >> 16) for v in p[ch::4]] + [None if a <= k < b else STALE_REC for k in range(n, total)]
            c, x, R[ch] = _walk_chain(recs)
            x16c[ch, :total] = x
            cntc[ch, :total] = c
    if mut == "pad-bits-kept":
        for ch in range(4):
            cntc[ch, lay["steps"][ch]:total] = 1
    step = np.arange(16 * nw)
    bit = (15 - (step & 15)).astype(np.uint32)
    one, two = (cntc >= 1).astype(np.uint32), (cntc >= 2).astype(np.uint32)
    if mut == "halves-swapped":
        one, two = two, one
    emask = ((one << bit) | (two << (bit + 16))).reshape(4, nw, 16).sum(axis=2, dtype=np.uint32)
    emask[:, lay["nbatch"]:] = STALE_MASK
    return x16c, emask, R


def place(pairs, mut=None, em=None):
    """-> (csize, payload bytes behind the 16 state bytes, final states)"""
    assert mut is None or mut in MUTANTS, mut
    np_ = len(pairs)
    x16c, emask, R = chain_leftovers(pairs, mut, em)
    lay = layout(np_)
    batches, nt = lay["batches"], lay["tiles"]
    etpc = nt + 2                                                              # the grid has the stride's tiles: more than the chunk needs
    popc = np.array([bin(i).count("1") for i in range(65536)], dtype=np.uint32)

    def skipped(kernel, tile):
        if mut == "tile-test-late":
            return (tile + 1) * ETILE >= np_
        if mut == kernel + "-tile-test->":
            return tile * ETILE > np_
        return tile * ETILE >= np_

    # k_emit_count: thread -> chain t >> 6, mask word tile * 64 + (t & 63)
    tsum = np.full(etpc, STALE_SUM, dtype=np.int64)
    lim = batches + (1 if mut == "count-live+1" else -1 if mut == "count-live-1" else 0)
    for tile in range(etpc):
        if skipped("count", tile):
            continue
        w = tile * (ETILE // 64) + np.arange(64)
        words = emask[:, w]
        n = np.where(w[None, :] < lim, popc[words & 0xFFFF] + popc[words >> 16], 0)
        tsum[tile] = int(n.sum())
    # k_emit_prefix: exclusive suffix sum over the tiles, windows of 64, last window first, with a carry
    carry = 0
    hi = nt
    while hi > 0:
        t_idx = hi - 1 - np.arange(WINDOW)                                     # lane 0 = the last tile of the window
        ok = t_idx >= 0
        v = np.where(ok, tsum[np.maximum(t_idx, 0)], 0)
        inc = np.cumsum(v)
        new = inc - v if mut == "carry-dropped" else carry + inc if mut == "suffix-inclusive" else carry + inc - v
        tsum[t_idx[ok]] = new[ok]
        carry += int(inc[-1])
        hi -= WINDOW
    csize = 16 + carry
    # k_put_payload: thread t owns the pairs [16 t, 16 t + 16) of the tile = the steps [s0, s0 + 4) of the four chains
    slack = 2 * np_ + 64
    buf = np.full(2 * slack + max(csize - 16, 0) + 8, STALE_BYTE, dtype=np.uint8)
    end = slack + max(csize - 16, 0)
    lim = batches + (1 if mut == "put-live+1" else -1 if mut == "put-live-1" else 0)
    tiles = [t for t in range(etpc) if not skipped("put", t)]
    if tiles:
        T = np.array(tiles, dtype=np.int64)[:, None]
        s0 = T * (ETILE // 4) + np.arange(TB, dtype=np.int64)[None, :] * 4
        live = (s0 >> 4) < lim
        base = np.where(live, s0, 0)
        step = s0[:, :, None] + np.arange(4)                                   # [tile, thread, q]
        bit = (step & 15) if mut == "bit-order" else 15 - (step & 15)
        cnt = np.zeros(s0.shape + (4, 4), dtype=np.int64)                      # [tile, thread, q, chain]: pair k = 4 q + chain
        xs = np.zeros(s0.shape + (4, 4), dtype=np.int64)
        for ch in range(4):
            mw = np.where(live, emask[ch][base >> 4], 0).astype(np.int64)[:, :, None]
            cnt[:, :, :, ch] = ((mw >> bit) & 1) + ((mw >> (16 + bit)) & 1)
            xs[:, :, :, ch] = x16c[ch][base[:, :, None] + np.arange(4)]
        cnt = cnt.reshape(s0.shape + (16,))
        xs = xs.reshape(s0.shape + (16,))
        n = cnt.sum(axis=2)
        inc = np.cumsum(n, axis=1)
        after0 = tsum[tiles][:, None] + inc[:, -1:] - inc                      # bytes of all pairs after the thread's sixteen
        after = after0[:, :, None] + np.cumsum(cnt[:, :, ::-1], axis=2)[:, :, ::-1]
        pos = np.clip(end - after, 0, len(buf) - 2)
        s1, s2 = cnt == 1, cnt == 2
        buf[pos[s1]] = xs[s1] & 0xFF
        first, second = ((xs[s2] & 0xFF), (xs[s2] >> 8) & 0xFF) if mut == "bytes-swapped" else ((xs[s2] >> 8) & 0xFF, xs[s2] & 0xFF)
        buf[pos[s2]] = first                                                   # the later (lower-address) byte of a step comes first
        buf[pos[s2] + 1] = second
    return csize, buf[end - max(csize - 16, 0): end].tobytes(), R


def payload(pairs, mut=None, em=None):
    """the chunk's payload as the format has it: R0..R3 little endian, then the emitted bytes"""
    csize, body, R = place(pairs, mut, em)
    return b"".join(int(r).to_bytes(4, "little") for r in R) + body


# ---- rans_record ---------------------------------------------------------------------------------------------------------------------
def record(lo, fr):
    """rans_record of ans_enc_chain.hip on numpy uint32 arrays: -> (xmax, rcp, bias, w = (65536 - fr) | shift << 24); 32-bit arithmetic only"""
    lo = np.asarray(lo, dtype=np.uint32)
    fr = np.asarray(fr, dtype=np.uint32)
    big = fr >= 2
    f2 = np.where(big, fr, 2).astype(np.uint32)
    sh = np.zeros(fr.shape, dtype=np.uint32)                                   # 32 - clz(fr - 1)
    v = f2 - np.uint32(1)
    while v.any():
        sh += (v != 0).astype(np.uint32)
        v = v >> np.uint32(1)
    D = f2 << (np.uint32(16) - sh)                                             # in (2^15, 2^16]
    top = np.uint32(0x80000000)
    qh = top // D
    rh = top - qh * D
    ql = (rh << np.uint32(16)) // D
    rem = (rh << np.uint32(16)) - ql * D
    rcp = (qh << np.uint32(16)) + ql + (rem != 0).astype(np.uint32)
    rcp = np.where(big, rcp, np.uint32(0xFFFFFFFF)).astype(np.uint32)
    shift = np.where(big, sh - np.uint32(1), 0).astype(np.uint32)
    bias = np.where(big, lo, lo + np.uint32(65535)).astype(np.uint32)
    return fr << np.uint32(15), rcp, bias, (np.uint32(65536) - fr) | (shift << np.uint32(24))


def record_step(x, rec):
    """the division part of one step on a renormalised state x (rans_step_turn2: v_mul_hi, the shift from w's top byte, v_mad_u32_u24)"""
    xmax, rcp, bias, w = rec
    x = np.asarray(x, dtype=np.uint64)
    q = ((x * rcp.astype(np.uint64)) >> np.uint64(32)) >> (w >> np.uint32(24)).astype(np.uint64)
    return ((q & np.uint64(0xFFFFFF)) * (w & np.uint32(0xFFFFFF)).astype(np.uint64) + x + bias.astype(np.uint64)) & np.uint64(0xFFFFFFFF)


# ---- events --------------------------------------------------------------------------------------------------------------------------
EVENTS = ("pad-0", "pad-255", "pad-256", "chains-unequal", "one-batch", "last-batch-partial", "tile-exact", "tile+1pair", "tile-without-emits",
          "window-exact", "window+1", "three-windows", "eight-windows", "two@bit0", "two@bit15", "two@thread-first", "two@thread-last",
          "two@tile-first", "two@tile-last", "one@tile-first", "one@tile-last", "emit@pair0", "emit@last-pair", "all-16-residues-two",
          "freq-1", "freq-2", "freq-pow2>=4", "freq-pow2+1", "freq>32768")


def reach(pairs, em=None):
    """event -> how often (or whether) the pairs reach it; conditions on the input alone.
    tile+1pair: one symbol behind a whole tile -- np is even, so its two pairs are the least a tile can hold."""
    p = np.asarray(pairs, dtype=np.uint32)
    np_ = len(p)
    cnt, _, _ = em if em is not None else emits(p)
    lay = layout(np_)
    j = np.arange(np_)
    two, one = cnt == 2, cnt == 1
    step = j >> 2
    fr = p >> 16
    pow2 = (fr & (fr - 1)) == 0
    tile_sums = np.bincount(j // ETILE, weights=cnt, minlength=lay["tiles"]) if np_ else np.zeros(0)
    ev = {
        "pad-0": np_ > 0 and max(lay["identity"]) == 0,                            # rlen = 0 (mod 512)
        "pad-255": lay["identity"][0] == 255,                                      # rlen = 1, 2 (mod 512)
        "pad-256": lay["identity"][3] == 256,                                      # rlen = 1 (mod 512): the most k_pairs ever writes
        "chains-unequal": lay["steps"][2] < lay["steps"][0],
        "one-batch": 0 < np_ <= 64,
        "last-batch-partial": lay["steps"][0] % 16 != 0,
        "tile-exact": np_ > 0 and np_ % ETILE == 0,
        "tile+1pair": np_ > ETILE and np_ % ETILE == 2,
        "tile-without-emits": int((tile_sums == 0).sum()),
        "window-exact": lay["tiles"] > 0 and lay["tiles"] % WINDOW == 0,
        "window+1": lay["tiles"] > WINDOW and lay["tiles"] % WINDOW == 1,
        "three-windows": lay["windows"] == 3,
        "eight-windows": lay["windows"] == 8,
        "two@bit0": int((two & ((step & 15) == 15)).sum()),
        "two@bit15": int((two & ((step & 15) == 0)).sum()),
        "two@thread-first": int((two & (j % 16 == 0)).sum()),
        "two@thread-last": int((two & (j % 16 == 15)).sum()),
        "two@tile-first": int((two & (j % ETILE == 0)).sum()),
        "two@tile-last": int((two & (j % ETILE == ETILE - 1)).sum()),
        "one@tile-first": int((one & (j % ETILE == 0)).sum()),
        "one@tile-last": int((one & (j % ETILE == ETILE - 1)).sum()),
        "emit@pair0": np_ > 0 and int(cnt[0]) > 0,
        "emit@last-pair": np_ > 0 and int(cnt[-1]) > 0,
        "all-16-residues-two": len(set((step[two] & 15).tolist())) == 16,
        "freq-1": int((fr == 1).sum()),
        "freq-2": int((fr == 2).sum()),
        "freq-pow2>=4": int((pow2 & (fr >= 4)).sum()),
        "freq-pow2+1": int(((fr >= 5) & (((fr - 1) & (fr - 2)) == 0)).sum()),
        "freq>32768": int((fr > 32768).sum()),
    }
    assert tuple(ev) == EVENTS
    return ev


# ---- the format around the payload ---------------------------------------------------------------------------------------------------
_LEBC = (127, 16510, 2113661, 270549116)


def leb(v):
    n = 1
    while n < 5 and v >= _LEBC[n - 1]:
        n += 1
    if n > 1:
        v -= _LEBC[n - 2]
    b = bytearray((v >> (7 * (n - 1 - k))) & 0x7F for k in range(n))
    b[-1] |= 0x80
    return bytes(b)


def chunks(t):
    t = np.asarray(t, dtype=np.uint8)
    return [t[a: a + CHUNK] for a in range(0, len(t), CHUNK)]


def chunk_pairs(oracle, chunk):
    """(freq table, RLE0 symbols, pairs) of one chunk, from the oracle's stages"""
    r, f = oracle.rank_encode(chunk)
    s = oracle.rle_encode(r)
    return f, s, oracle.model_pairs(s)


def chunk_stream(oracle, chunk, mut=None):
    f, s, pairs = chunk_pairs(oracle, chunk)
    pay = payload(pairs, mut)
    return b"".join(leb(int(v)) for v in f) + leb(len(chunk)) + leb(len(pay)) + leb(len(s)) + pay


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def norepeat(n, seed, alphabet=256):
    """n random bytes below `alphabet`, no two neighbours equal: rlen == n"""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.integers(1, alphabet, n)) % alphabet).astype(np.uint8)


def quiet(n, extra=(), spacing=1500):
    """two alternating bytes (rank 1 throughout: nearly free symbols, whole tiles emit nothing) with a rare visitor every `spacing` bytes
    and the `extra` ones (offset, byte).  rlen == n.  The RLE0 stream is in bucket order: the ranks of the more frequent of the two bytes
    (with visitors at even offsets: the 9s), then the other's, then the visitors'.
    ONE extra visitor in place of the 9 at the odd offset p gives the next 9 rank 2 -- symbol (p + 1) / 2 of the stream, whose mantissa
    (the set bit of an alphabet-2 model that has seen thousands of clear ones: a frequency near 32) is an odd pair; TWO side by side at an
    even offset p give the next 7 and the next 9 rank 3, a class the stream shows nowhere else: their exponents are even pairs of a
    frequency that small"""
    t = np.where(np.arange(n) % 2 == 0, 7, 9).astype(np.uint8)
    pos = np.arange(spacing, n, spacing)
    t[pos] = (20 + (np.arange(len(pos)) * 37) % 200).astype(np.uint8)
    for at, b in extra:
        t[at] = b
    return t


def run_tail(prefix, seed):
    """exactly one chunk: `prefix` no-repeat bytes below 255 and one run of byte 255 to the end of the chunk"""
    t = np.full(CHUNK, 255, dtype=np.uint8)
    t[:prefix] = norepeat(prefix, seed, 255)
    return t


RLENS = (1, 2, 3, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
WINDOW_RLENS = (131071, 131072, 131073, 262145)
# name -> (n, extra visitors).  The offsets were searched: quiet-first has a two-byte emit on pair 4096, the first of tile 1, quiet-last
# one on pair 4095, the last of tile 0 (of 4000 offsets tried with two visitors, none gave the second; see quiet())
QUIET = {
    "quiet-2047": (2047, ()), "quiet-2048": (2048, ()), "quiet-2049": (2049, ()),
    "quiet-first": (8193, ((4096, 231), (4097, 232))),
    "quiet-last": (6143, ((4095, 233),)),
    "quiet-still": (16385, (), 100000),                      # no visitor at all: eight tiles and one symbol
}
# name -> (no-repeat bytes in front of chunk one's run, seed, rlen of chunk one, rlen of chunk two).  The run of 2^20 - prefix bytes is
# 19 or 20 symbols; the prefixes were searched with the oracle
IMAGE_SPECS = {
    "512+513": (492, 11, 512, 513),
    "2048+1": (2029, 12, 2048, 1),
    "2049+2048": (2029, 13, 2049, 2048),
    "131073+512": (131053, 14, 131073, 512),
}
# image -> (events chunk one must reach, events chunk two must reach)
IMAGE_REACH = {
    "512+513": (("pad-0",), ("pad-255", "pad-256", "chains-unequal", "last-batch-partial", "two@bit0", "two@bit15")),
    "2048+1": (("pad-0", "tile-exact", "two@bit0", "two@bit15"), ("pad-256", "one-batch", "tile-without-emits")),
    "2049+2048": (("pad-256", "chains-unequal", "tile+1pair", "one@tile-last"), ("pad-0", "tile-exact", "one@tile-first")),
    "131073+512": (("pad-256", "tile+1pair", "window+1", "all-16-residues-two"), ("pad-0", "two@bit0", "two@bit15")),
}
# lengths of the group's blocks (prefixes of one random stream), searched: the one chunk of each block's BWT image has the rlen below
GROUP_LENS = (151, 152, 153, 600, 1084, 1085, 1086, 1590)
GROUP_RLENS = {151: 511, 152: 512, 153: 513, 1084: 1535, 1085: 1536, 1086: 1537, 1590: 2048}


@functools.lru_cache(maxsize=None)
def case(name):
    """the named input as a read-only uint8 array"""
    kind, _, arg = name.partition("-")
    if kind == "norep":
        n = int(arg)
        t = norepeat(n, n)
    elif kind == "quiet":
        t = quiet(*QUIET[name])
    elif name == "full-chunk":
        t = norepeat(CHUNK, 77)
    elif name == "full-chunk-1":
        t = norepeat(CHUNK - 1, 78)
    else:
        raise KeyError(name)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def image(name):
    prefix, seed, r1, r2 = IMAGE_SPECS[name]
    t = np.concatenate((run_tail(prefix, seed), norepeat(r2, seed + 1)))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def group():
    src = np.random.default_rng(9000).integers(0, 256, 1700, dtype=np.uint8)
    src.setflags(write=False)
    return tuple(src[:n] for n in GROUP_LENS)


CASES = tuple(f"norep-{n}" for n in RLENS) + tuple(QUIET) + tuple(f"norep-{n}" for n in WINDOW_RLENS) + ("full-chunk", "full-chunk-1")
IMAGES = tuple(IMAGE_SPECS)
