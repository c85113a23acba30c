"""The rANS decoder's front restated in plain Python: the scheme of k_dec_headers (ans_dec.hip), k_dec_rans (with its ByteQueue,
ans_dec_rans.hip) and k_dec_rle (ans_dec_rank.hip), and of the batch plumbing around them in ans_dec.hip (cbase, rle_off / out_off, the cleared rank arrays, k_dec_order) -- window by window, symbol by symbol and
pass by pass with the kernels' own intermediate values -- and the crafted inputs that reach their edges.  No GPU code is imported; what
needs the oracle takes it as an argument.

The oracle is the reference ALGORITHM (one byte pointer, one LEB value at a time).  This is the kernels' SCHEME:
  headers(stream, out_cap)      one wave per stream: 64-byte windows from the header's first byte, the ballot of terminators, `before`,
                                vidx, nlead from prevmask or from `since` (continuation bytes the previous window left), the LEB_OFF add,
                                fsum per lane, the 259th terminator found by clearing bits, the acceptance test
                                -> (status, [ChunkInfo], freq, (out bytes, rle symbols))
  ByteQueue                     a = (address + in_off) & 3, the 256-byte windows cur / nxt (lane l = dword l), the roll at di & 63 == 0,
                                the byte-wise load() near in_len, the 64-bit queue, taken()
  rans(stream, info, lead)      one wave per chunk: the exponent model as HI per lane (LO is the row shift), the alphabet-2 pairs in lanes
                                0..3 with qa, classes 2..5 in lanes [2^e, 2^(e+1)), the countdowns `rem` in lanes 0..5 and qexpn in lanes
                                0..3, class 6 in one register and class 7 in three; the gate, the slow block (rebuild or the class 6 / 7
                                arm, then both renormalisations, exponent state first), the tile loop, the tail with its swap, the final
                                check -> (symbols, status bits)
  rle(symbols, info, stale)     one workgroup per chunk: passes of 4096 symbols, 4 per thread, the backward gather with its nb limit,
                                the look-ahead, the scan with carry_s, stores only where val != 0 -> (rank array, status bits)
  decode(oracle, streams, caps) the batch: the count pass, cbase, the arena layout, the clear, the fill pass, k_dec_order beyond 1024
                                chunks, the three stages, the status mapping, then the oracle's rank decode -> [(status, bytes)]
Memory nobody wrote holds STALE values, so that a slot left out, a missing clear or a store beside its place shows.  `mut` names ONE
changed token of the scheme (MUTANTS); `ev` is a dict that counts the named arms the input reaches (EVENTS).

Mutants that cannot change a byte of a valid stream (EQUIVALENT, with the reason) are kept: the test asserts that they change none.
Events no valid stream reaches would go to UNREACHABLE, with the argument; the one there is stands beside its nearest reachable neighbour.

The exponent model is kept for lanes 0..7 only: lanes 8..63 hold HI = 65536 for good (their mix target is 65536), lane 7 does too, and
the lowest lane whose HI is above the range is taken, so no lane behind 7 is ever picked.

The valid inputs are streams the oracle makes from crafted texts; none is mutated.  CASES are one-chunk texts, CHAINS lists of texts
whose streams are concatenated (a valid chain: the test decodes every one with the oracle), BATCH block streams for one batched call.

The refusal side (at the end of the file): REFUSED are streams built field by field and symbol by symbol from the oracle's pieces so
that ONE acceptance test of the scheme refuses each (REASON names it; where the format ties two tests together both are named and the
stream that separates them stands beside it), STILL_ACCEPTED their accepted neighbours, REFUSAL_MUTANTS the scheme with one such test
dropped or moved by one.  Every acceptance test logs a refuse-* event of its own.  run, tot and carry_s of k_dec_rle, the header's
values and fsum are kept in 32 bits as the kernels keep them: two of the streams depend on the wrap.  The model asserts its own bounds
on the way -- every in[p - k] of the header walk inside the chunk's header, every gather step inside the chunk's symbols, every rank
store below olen, the queue's reads clipped to the input as load() clips them: a stream on which verdict() returns has left no buffer
in the scheme, which is the argument test_gpu_dec_refusals.py makes before it hands the stream to a kernel."""
import collections
import functools

import numpy as np

CHUNK = 1 << 20
RANS_L = 1 << 23
LEB_OFF = (127, 16510, 2113661, 270549116)
OK, E_CAPACITY, E_CORRUPT = 0, -2, -3
PASS = 4096                      # symbols per pass of k_dec_rle
PER_THREAD = 4
STALE_SYM = 0xEEEE               # an RLE0 symbol nobody wrote
STALE_RANK = 0xEE                # a rank nobody wrote (the arena before the clear)
STALE_FREQ = -7                  # a frequency nobody wrote
QCAP = 65536
IN_LEADS = (0, 1, 2, 3, 15)

ChunkInfo = collections.namedtuple("ChunkInfo", "in_off clen olen rlen blk out_off rle_off")

HDR_MUTANTS = (
    "since-not-carried",         # k_dec_headers: since = 0 at every window
    "leb-off-nlead",             # LEB_OFF[nlead]
    "end-from-last-terminator",  # pos += 63 - clz(term) + 1
    "before-counts-own-lane",    # before = popc(term & ((2 << l) - 1))
    "fsum-vidx-le-256",          # vidx <= 256 goes to the frequency arm
    "rp-plus-olen",              # rp += olen
    "since-limit-5",             # since > 5
)
QUEUE_MUTANTS = (
    "skip-not-dropped",          # ByteQueue::init without buf >>= 8 a
    "roll-at-63",                # (di & 63) == 63
    "no-prefetch",               # init without nxt = load(1)
    "tail-dword-zero",           # load(): a dword that crosses in_len reads as 0
    "load-g-negative-unchecked",  # load() without g >= 0
)
RANS_MUTANTS = (
    "tail-no-swap",              # the tail without the swap of the state pairs
    "tile-bound-lt",             # t + 64 < rlen
    "renorm-x-single-byte", "renorm-x2-single-byte",       # JPK_RENORM2 without the second take
    "renorm-mantissa-first",     # JPK_RENORM2(x2, x)
    "rem-starts-8",              # rem = 8 in lanes 0..3
    "rem-ex1",                   # rem = ex1
    "cap-32768",                 # the cap of expn
    "remainder-lane0",           # the rounding remainder of classes 2..5 added in lane 0
    "reg2-wrong-lane",           # f7[2] += (l == 1) ? 16 : 0
    "tgt-swapped",               # tgt = (sym & 1) ? 65535 : 1
    "gate-x-only",               # gate = due ? 0 : x
    "rem6-not-reset",            # class 6 arm without rem = (l == 4) ? 1 : rem
    "exp-mix-le",                # below = l <= e
    "seen7-ge",                  # ++seen7 >= expn7
)
RLE_MUTANTS = (
    "gather-stops-at-b0",        # k_dec_rle: u >= b0
    "gather-past-chunk-start",   # the gather without u >= 0
    "lookahead-unguarded",       # src[t + 1] > 1 without t + 1 >= rlen
    "nb-limit-lower",            # nb > 19
    "carry-not-added",           # run = inc - s
    "gather-limit-22",           # nb <= 22 in the gather's loop
)
BATCH_MUTANTS = ("no-rank-clear",)      # jpk_ans_decode_batch without the memset of the rank arrays
# one acceptance test dropped, or moved by one: told apart by a refused stream (REFUSED) or by an accepted neighbour
REFUSAL_MUTANTS = (
    "no-nlead-limit",            # k_dec_headers without nlead > 4
    "no-since-limit",            # without since > 4
    "no-freq-limit",             # without x > ANS_CHUNK on a frequency
    "no-olen-limit", "olen-ge-chunk",       # without olen > ANS_CHUNK; olen >= ANS_CHUNK
    "no-rlen-limit",             # without rlen > olen
    "no-clen-fit",               # without clen > len - ip
    "no-clen-min", "clen-lt-15",            # without clen < 16; clen < 15
    "no-total-check",            # without total != olen
    "no-states-check",           # k_dec_rans without the four R != RANS_L
    "no-taken-check", "taken-ge-clen",      # without bq.taken() > clen; taken() >= clen
    "no-nb-limit", "nb-limit-21",           # k_dec_rle without nb > 20; nb > 21
    "no-store-flag", "run-le-olen",         # without the else atomicOr behind run < olen; run <= olen
    "no-carry-check",            # without carry_s != olen
)
MUTANTS = HDR_MUTANTS + QUEUE_MUTANTS + RANS_MUTANTS + RLE_MUTANTS + BATCH_MUTANTS + REFUSAL_MUTANTS
# mutant -> why no stream, valid or not, can tell it from the scheme (the test runs them on every refused stream too)
_SINCE = ("`since` only ends the walk early.  Without it the walk goes on to the next window with nval < 259, so the first terminator "
          "there is a header value: its nlead = l + since >= since > 4 and `nlead > 4` refuses it; with no terminator in that window "
          "since grows by 64, and the windows end at pos >= len, which refuses too.  Either way the chunk is refused and nothing of it "
          "is listed.  On a malformed header the limit decides which test refuses, never whether")
EQUIVALENT = {
    "since-limit-5": "a LEB128 value has at most five bytes, four of them continuation bytes: in a valid header `since` never exceeds 4, "
                     "so neither limit is ever met.  " + _SINCE,
    "no-since-limit": _SINCE,
    "load-g-negative-unchecked": "g = gbase + 4 (64 w + l) >= gbase = in_off - a, and a chunk's payload starts behind its header of at least "
                                 "259 bytes, so in_off - a >= 256 > 0: the test guards streams that begin with a payload, which the format "
                                 "does not have",
    "tile-bound-lt": "it only sends a last tile of exactly 64 symbols through the tail, which decodes the same symbols one at a time: the swap "
                     "of the state pairs gives symbol j the pair (R0, R1) for even j and (R2, R3) for odd j, as the tile loop does, lanes "
                     "0..63 are all below `left` = 64 and are all stored, and the final check looks at all four states",
    "gather-limit-22": "the loop's limit only bounds the walk over a malformed group; a valid chunk decodes to at most 2^20 bytes, so a group "
                       "has at most 20 digits, the walk ends on a non-digit or the chunk's start with nb <= 20 and `nb > 20` is never true.  "
                       "On a malformed group of 21 digits or more the walk ends with nb = 21 or 22 under one limit and 21, 22 or 23 under "
                       "the other: all above 20, so the group is refused and its count is never formed",
}
# event -> why no stream the encoder makes reaches it
UNREACHABLE = {
    "rle-no-zero": "the rank coder's list starts in first-appearance order (rank.cpp:45-90), so the first byte of every chunk is at list position 0 "
                   "and codes as rank 0: every non-empty chunk's rank array holds at least one zero, the head of its first symbol's bucket.  "
                   "`rle-one-zero` names the nearest thing a stream has: that zero and no other",
    "refuse-max-chunks": "nch >= max_chunks needs len / 275 + 2 accepted chunks inside len bytes.  An accepted chunk has 259 header values "
                         "of at least one byte each and clen >= 16, so it takes 275 bytes or more, and n accepted chunks end at "
                         "ip >= 275 n; the loop runs only while ip < len, so n < len / 275 + 1 when the test is made",
    "refuse-ip-past-len": "ip is the byte behind the header's last terminator, and a terminator is a lane with p < len (the ballot tests it): "
                          "ip <= len for every header the walk completes",
    "refuse-rle-symbol-over-256": "k_dec_rans forms a symbol as the lane of classes 0..5 (0..63), 64 + m with m <= 63 or 128 + m with "
                                  "m <= 128: at most 256 whatever the payload holds, and k_dec_rle reads only what k_dec_rans stored "
                                  "(t < rlen, the look-ahead and the gather stay inside the chunk)",
}

_FIELDS = ("freq", "olen", "clen", "rlen")
HDR_EVENTS = (tuple(f"hdr-{f}-since{k}" for f in _FIELDS for k in (1, 2)) +
              ("hdr-end-lane63", "hdr-end-lane0", "hdr-surplus-terminators", "hdr-5-windows", "hdr-more-than-5-windows", "hdr-window-past-len") +
              tuple(f"hdr-start-mod4-{k}" for k in range(4)) + tuple(f"hdr-start-mod64-{k}" for k in (0, 1, 63)) +
              ("hdr-freq-3-bytes", "hdr-chunk-of-one-byte-275", "hdr-chain-over-64"))
QUEUE_EVENTS = (tuple(f"queue-a{k}" for k in range(4)) +
                ("queue-roll-1", "queue-roll-2", "queue-roll-after-4-byte-symbol", "queue-tail-partial-dword", "queue-dword-past-end",
                 "queue-payload-ends-at-in-len", "queue-taken-equals-clen"))
_RLENS = (1, 2, 3, 63, 64, 65, 128)
_PATTERNS = ("01", "10", "11", "02", "20", "12", "21", "22")
RANS_EVENTS = (tuple(f"rlen-{n}" for n in _RLENS) + tuple(f"rlen-above-64-mod4-{k}" for k in (1, 2, 3)) + tuple(f"class-{e}" for e in range(8)) +
               tuple(f"bytes-{p}" for p in _PATTERNS) + ("slow-due-only", "slow-bytes-only", "slow-due-and-bytes") +
               tuple(f"rebuild-class-{e}" for e in range(2, 8)) + ("lg-0", "lg-1", "lg-ge-2", "lg-5", "expn-cap", "expn-cap-twice",
                                                                  "class7-reg0", "class7-reg1", "class7-sym129", "pair0-high", "pair0-low",
                                                                  "pair1-high", "pair1-low", "exp-floor-used", "tail-odd"))
RLE_EVENTS = ("rle-group-over-thread-edge", "rle-group-over-pass-edge", "rle-lookahead-over-pass-edge", "rle-group-at-chunk-start",
              "rle-group-at-chunk-end", "rle-digits-end-then-digits-start", "rle-group-1-digits", "rle-group-2-digits", "rle-group-19-digits",
              "rle-group-20-digits", "rle-store-at-olen-1", "rle-pass-with-carry", "rle-no-zero", "rle-one-zero", "rle-only-zeros")
BATCH_EVENTS = ("batch-block-offsets-nonzero", "batch-zero-over-dense", "batch-order-not-identity")
# the three acceptance tests no stream reaches (UNREACHABLE); the refusal side has its own lists, REFUSE_EVENTS and INPUT_EVENTS, beside
# the streams that reach the others
DEAD_REFUSALS = ("refuse-max-chunks", "refuse-ip-past-len", "refuse-rle-symbol-over-256")
EVENTS = HDR_EVENTS + QUEUE_EVENTS + RANS_EVENTS + RLE_EVENTS + BATCH_EVENTS + DEAD_REFUSALS


def _log(ev, name, n=1):
    if ev is not None and n:
        ev[name] = ev.get(name, 0) + n


def uniform_cdf(A, i):
    if i <= 0:
        return 0
    scale = 65536 // A
    return i * scale + (65536 - scale * A)


# ---- k_dec_headers -----------------------------------------------------------------------------------------------------------------------
def headers(stream, out_cap, mut=None, ev=None, blk=0):
    """-> (status, [ChunkInfo], [freq[256]], (out bytes, rle symbols)) of one stream; the chunks in front of a refused one stay listed"""
    assert mut is None or mut in MUTANTS, mut
    s = bytes(stream)
    ln = len(s)
    max_chunks = ln // 275 + 2
    ip = op = rp = 0
    status = OK
    infos, freqs = [], []
    leb_off = LEB_OFF + (0,) * 64
    while ip < ln and status == OK:
        if len(infos) >= max_chunks:
            _log(ev, "refuse-max-chunks")
            status = E_CORRUPT
            break
        _log(ev, f"hdr-start-mod4-{ip % 4}")
        if ip % 64 in (0, 1, 63):
            _log(ev, f"hdr-start-mod64-{ip % 64}")
        start = ip
        nval, pos = 0, ip
        fields = [0, 0, 0]                     # olen, clen, rlen: each decoded by the lane that holds its terminator, summed over the wave
        fsum = [0] * 64
        freq = [STALE_FREQ] * 256
        bad = False
        since = 0
        nwin = 0
        fsum_mask = 0xffffffff                 # fsum and its wave sum are 32-bit registers
        while nval < 259:
            if pos >= ln:
                _log(ev, "refuse-header-truncated")
                bad = True
                break
            nwin += 1
            win = s[pos: pos + 64]             # lanes past len read 0 and are no terminators
            if pos + 64 > ln:
                _log(ev, "hdr-window-past-len")
            term = 0
            for l, b in enumerate(win):
                if b & 0x80:
                    term |= 1 << l
            t = term
            while t:
                l = (t & -t).bit_length() - 1
                t &= t - 1
                own = 1 if mut == "before-counts-own-lane" else 0
                vidx = nval + bin(term & ((1 << (l + own)) - 1)).count("1")
                if vidx >= 259:
                    continue
                prevmask = term & ((1 << l) - 1)
                nlead = l - (prevmask.bit_length() - 1) - 1 if prevmask else l + since
                if nlead > 4 and mut != "no-nlead-limit":
                    _log(ev, "refuse-nlead-over-4")
                    bad = True
                    continue
                p = pos + l
                x = 0
                for k in range(nlead, 0, -1):
                    assert ip <= p - k < ln, "k_dec_headers reads in[p - k] outside the chunk's header"
                    x = ((x << 7) | s[p - k]) & 0xffffffff
                x = ((x << 7) | (win[l] & 0x7f)) & 0xffffffff
                if nlead > 0:
                    x = (x + leb_off[nlead if mut == "leb-off-nlead" else nlead - 1]) & 0xffffffff
                    _log(ev, "hdr-5-byte-value-wraps", nlead == 4 and s[p - 4] >> 4 != 0)
                field = _FIELDS[max(vidx - 255, 0)]
                if not prevmask and since in (1, 2):
                    _log(ev, f"hdr-{field}-since{since}")
                if vidx < 256 or (vidx == 256 and mut == "fsum-vidx-le-256"):
                    if x > CHUNK and mut != "no-freq-limit":
                        _log(ev, "refuse-freq-over-chunk")
                        bad = True
                    if vidx < 256:
                        freq[vidx] = x
                        if nlead == 2:
                            _log(ev, "hdr-freq-3-bytes")
                    fsum[l] = (fsum[l] + x) & fsum_mask
                else:
                    fields[vidx - 256] += x
            nt = bin(term).count("1")
            if nval + nt >= 259:
                tt = term
                for _ in range(259 - nval - 1):
                    tt &= tt - 1
                end = (tt & -tt).bit_length() - 1
                if mut == "end-from-last-terminator":
                    end = term.bit_length() - 1
                if end in (0, 63):
                    _log(ev, f"hdr-end-lane{end}")
                if nt > 259 - nval:
                    _log(ev, "hdr-surplus-terminators")
                pos += end + 1
                nval = 259
            else:
                since = (64 - term.bit_length()) if nt else since + 64
                if mut == "since-not-carried":
                    since = 0
                if since > (5 if mut == "since-limit-5" else 4) and mut != "no-since-limit":
                    _log(ev, "refuse-since-over-window" if nt else "refuse-window-without-terminator")
                    bad = True
                    break
                nval += nt
                pos += 64
        olen, clen, rlen = (f & 0xffffffff for f in fields)
        total = sum(fsum) & fsum_mask
        ip = pos
        # the acceptance test, term by term: a walk that stopped inside the header (nval < 259) has no fields to test
        tests = () if nval < 259 else (
            ("refuse-olen-over-chunk", (olen >= CHUNK if mut == "olen-ge-chunk" else olen > CHUNK) and mut != "no-olen-limit"),
            ("refuse-rlen-over-olen", rlen > olen and mut != "no-rlen-limit"),
            ("refuse-ip-past-len", ip > ln),
            ("refuse-clen-past-len", clen > ln - ip and mut != "no-clen-fit"),
            ("refuse-clen-below-16", clen < (15 if mut == "clen-lt-15" else 16) and mut != "no-clen-min"),
            ("refuse-total-ne-olen", total != olen and mut != "no-total-check"))
        for name, fired in tests:
            _log(ev, name, fired)
            bad = bad or fired
        if bad:
            status = E_CORRUPT
            break
        if op + olen > out_cap:
            _log(ev, f"refuse-capacity-at-chunk-{len(infos) + 1}" if len(infos) < 2 else "refuse-capacity-later")
            status = E_CAPACITY
            break
        _log(ev, "hdr-5-windows", nwin == 5)
        _log(ev, "hdr-more-than-5-windows", nwin > 5)
        _log(ev, "hdr-chunk-of-one-byte-275", olen == 1 and ip + clen - start == 275)
        infos.append(ChunkInfo(ip, clen, olen, rlen, blk, op, rp))
        freqs.append(freq)
        ip += clen
        op += olen
        rp += olen if mut == "rp-plus-olen" else rlen
    _log(ev, "hdr-chain-over-64", len(infos) > 64)
    return status, infos, freqs, (op, rp)


# ---- ByteQueue ---------------------------------------------------------------------------------------------------------------------------
class ByteQueue:
    def __init__(self, s, in_off, lead, mut=None, ev=None):
        self.s, self.in_len, self.mut, self.ev = s, len(s), mut, ev
        a = (lead + in_off) & 3            # the stream starts `lead` bytes behind an aligned address
        self.gbase = in_off - a
        self.cur = self.load(0)
        self.nxt = [0] * 64 if mut == "no-prefetch" else self.load(1)
        self.di, self.buf, self.nb, self.skip = 0, 0, 0, a
        self.taken4 = False                # the symbol before this refill took four bytes
        _log(ev, f"queue-a{a}")
        self.refill()
        if mut != "skip-not-dropped":
            self.buf >>= 8 * a
        self.nb -= a
        self.refill()

    def load(self, w):
        """lane l's dword of window w: whole where it lies inside the input, byte by byte (0 past in_len) otherwise"""
        g0 = self.gbase + w * 256
        out = []
        for l in range(64):
            g = g0 + 4 * l
            if g < 0:                      # in front of the input: the guarded load takes the bytes that exist, the unguarded one whatever lies there
                out.append(0xEEEEEEEE if self.mut == "load-g-negative-unchecked" else sum(self.s[g + k] << (8 * k) for k in range(4) if g + k >= 0))
                continue
            d = self.s[g: g + 4]
            out.append(0 if self.mut == "tail-dword-zero" and 0 < len(d) < 4 else int.from_bytes(d, "little"))
        return out

    def refill(self):
        di = self.di
        if (di & 63) == (63 if self.mut == "roll-at-63" else 0) and di != 0:
            self.cur = self.nxt
            self.nxt = self.load((di >> 6) + 1)
            if self.ev is not None:
                _log(self.ev, "queue-roll-1", di >> 6 == 1)
                _log(self.ev, "queue-roll-2", di >> 6 == 2)
                _log(self.ev, "queue-roll-after-4-byte-symbol", self.taken4)
        if self.ev is not None:
            g = self.gbase + 4 * di
            _log(self.ev, "queue-dword-past-end", g >= self.in_len)
            _log(self.ev, "queue-tail-partial-dword", g < self.in_len < g + 4)
        self.buf |= self.cur[di & 63] << (8 * self.nb)
        self.nb += 4
        self.di = di + 1

    def take(self):
        b = self.buf & 0xff
        self.buf >>= 8
        self.nb -= 1
        return b

    def taken(self):
        return 4 * self.di - self.skip - self.nb


def _quasi_rebuild(F, A, to_first, ev):
    """QuasiModel rebuild (model.cpp:160-204) of the A counts F, already in the model's units -> (the A widths, what lies in front of the
    class).  to_first: the rounding remainder goes to the class's first symbol; otherwise to a lane in front of the class"""
    tot = sum(F)
    lg = 0
    while (tot >> lg) + A > 65536:
        lg += 1
    _log(ev, "lg-0", lg == 0)
    _log(ev, "lg-1", lg == 1)
    _log(ev, "lg-ge-2", lg >= 2)
    _log(ev, "lg-5", lg == 5)
    F = [(f >> lg) + 1 for f in F]
    t2 = sum(F)
    F = [((65536 * f) & 0xffffffff) // t2 for f in F]
    rest = 65536 - sum(F)
    if to_first:
        F[0] += rest
        return F, 0
    return F, rest                        # the remainder went to a lane in front of the class: every bound of the class moves up by it


# ---- k_dec_rans --------------------------------------------------------------------------------------------------------------------------
def rans(stream, info, lead=0, mut=None, ev=None):
    """one chunk -> (rlen symbols, STALE_SYM where nothing was stored; status bits: 1 = the final check failed)"""
    assert mut is None or mut in MUTANTS, mut
    s = bytes(stream)
    clen, rlen = info.clen, info.rlen
    bq = ByteQueue(s, info.in_off, lead, mut, ev)
    _log(ev, "queue-payload-ends-at-in-len", info.in_off + clen == len(s))
    ehi = [uniform_cdf(8, l + 1) for l in range(8)]                    # lane j: HI = cdf[j + 1]; LO is lane j - 1's HI (row shift)
    qhi, qlo, qf = [0] * 64, [0] * 64, [0] * 64
    for l in range(64):
        cls = 0 if l < 2 else l.bit_length() - 1
        A = 2 if l < 4 else 1 << cls
        i = (l & 1) if l < 4 else l - A
        qlo[l], qhi[l] = uniform_cdf(A, i), uniform_cdf(A, i + 1)
    qfr = [h - lo for h, lo in zip(qhi, qlo)]
    qa = [32768] * 4
    hi6 = [uniform_cdf(64, l + 1) for l in range(64)]
    lo6 = [uniform_cdf(64, l) for l in range(64)]
    f6 = [0] * 64
    seen6, expn6 = 0, 8
    # class 7: symbol i = lane i % 64 of register i // 64; kept as three registers of 64 lanes
    hi7 = [[uniform_cdf(129, l + 64 * j + 1) if l + 64 * j < 129 else 65536 for l in range(64)] for j in range(3)]
    lo7 = [[uniform_cdf(129, l + 64 * j) if l + 64 * j < 129 else 65536 for l in range(64)] for j in range(3)]
    f7 = [[0] * 64 for _ in range(3)]
    seen7, expn7 = 0, 8
    qexpn = [8] * 4
    rem = [8 if mut == "rem-starts-8" else 9] * 4 + [1, 1]
    R = []
    for k in range(4):
        b = []
        for _ in range(4):
            b.append(bq.take())
            if bq.nb < 4:
                bq.refill()
        R.append(b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24)
    mysym = [0] * 64
    out = [STALE_SYM] * rlen
    cap = 32768 if mut == "cap-32768" else QCAP
    tracking = ev is not None

    def symbol(ra, rb, lanei):
        nonlocal seen6, expn6, seen7, expn7
        RA, RB = R[ra], R[rb]
        rng = RA & 0xffff
        e = 0
        while rng >= ehi[e]:
            e += 1
        elo = ehi[e - 1] if e else 0
        efr = ehi[e] - elo
        x = efr * (RA >> 16) + rng - elo
        if tracking:
            _log(ev, f"class-{e}")
            _log(ev, "exp-floor-used", efr <= 32)
        for j in range(7):                                            # AdaptiveModel update: entry j + 1 lives in lane j
            below = j <= e if mut == "exp-mix-le" else j < e
            ehi[j] += ((j + 1 if below else j + 1 + 65536 - 8) - ehi[j]) >> 5
        if e >= 2:
            rem[e - 2] -= 1
        due = 0 in rem
        rngm, xs = RB & 0xffff, RB >> 16
        if e < 6:
            sym = 2 * e if e < 2 else 1 << e
            last = sym + 1 if e < 2 else 2 * sym - 1
            while sym <= last and rngm >= qhi[sym]:
                sym += 1
            if sym > last:                                            # no lane of the class is above the range: s_ff1 gives -1, lane 63 is read
                sym = -1
                x2 = qfr[63] * xs + rngm - qlo[63]
            else:
                x2 = qfr[sym] * xs + rngm - qlo[sym]
                qf[sym] += 1
            if e < 2:
                tgt = 1 if (sym & 1) != (mut == "tgt-swapped") else 65535
                l0 = 2 * e
                d = (tgt - qa[l0]) >> 5
                qa[l0] += d
                qa[l0 + 1] += d
                qhi[l0] += d                                          # even lane: [0, a)
                qfr[l0] += d
                qlo[l0 + 1] += d                                      # odd lane: [a, 65536)
                qfr[l0 + 1] -= d
                if tracking:
                    _log(ev, f"pair{e}-high", qa[l0] >= 65504)
                    _log(ev, f"pair{e}-low", qa[l0] <= 32)
        else:
            sym, x2 = -1, 0                                           # no lane of classes 6, 7: the slow block redoes both
        gate = 0 if due else (x if mut == "gate-x-only" else min(x, x2))
        if gate < RANS_L:
            if due:
                if e == 6:
                    m = 0
                    while m < 63 and rngm >= hi6[m]:
                        m += 1
                    x2 = (hi6[m] - lo6[m]) * xs + rngm - lo6[m]
                    f6[m] += 16
                    sym = 64 + m
                    seen6 += 1
                    if seen6 > expn6:
                        _log(ev, "rebuild-class-6")
                        F, _ = _quasi_rebuild(f6, 64, True, ev)
                        acc = 0
                        for l in range(64):
                            lo6[l] = acc
                            acc += F[l]
                            hi6[l] = acc
                            f6[l] = 0
                        expn6 = expn6 << 1 if expn6 < 65536 else 65536
                        seen6 = 0
                    if mut != "rem6-not-reset":
                        rem[4] = 1
                elif e == 7:
                    if rngm < hi7[0][63]:
                        j, m = 0, 0
                        while rngm >= hi7[0][m]:
                            m += 1
                        _log(ev, "class7-reg0")
                    elif rngm < hi7[1][63]:
                        j, m = 1, 0
                        while rngm >= hi7[1][m]:
                            m += 1
                        _log(ev, "class7-reg1")
                    else:
                        j, m = 2, 0                                   # the 129th symbol: lane 0 of the third register
                        _log(ev, "class7-sym129")
                    x2 = (hi7[j][m] - lo7[j][m]) * xs + rngm - lo7[j][m]
                    f7[j][1 if j == 2 and mut == "reg2-wrong-lane" else m] += 16
                    sym = 128 + 64 * j + m
                    seen7 += 1
                    if (seen7 >= expn7) if mut == "seen7-ge" else (seen7 > expn7):
                        _log(ev, "rebuild-class-7")
                        F, _ = _quasi_rebuild(f7[0] + f7[1] + f7[2][:1], 129, True, ev)      # lanes with i >= 129 count as 0
                        acc = 0
                        for i in range(192):
                            jj, l = i >> 6, i & 63
                            w = F[i] if i < 129 else 0
                            lo7[jj][l] = acc
                            acc += w
                            hi7[jj][l] = acc
                            f7[jj][l] = 0
                        expn7 = expn7 << 1 if expn7 < 65536 else 65536
                        seen7 = 0
                    rem[5] = 1
                else:
                    kl, A = e - 2, 1 << e
                    _log(ev, f"rebuild-class-{e}")
                    F, ahead = _quasi_rebuild([f << 4 for f in qf[A: 2 * A]], A, mut != "remainder-lane0", ev)
                    acc = ahead
                    for i in range(A):
                        qlo[A + i] = acc
                        acc += F[i]
                        qhi[A + i] = acc
                        qfr[A + i] = F[i]
                        qf[A + i] = 0
                    ex0 = qexpn[kl]
                    ex1 = ex0 << 1 if ex0 < cap else cap
                    if tracking:
                        _log(ev, "expn-cap", ex1 == QCAP)
                        _log(ev, "expn-cap-twice", ex0 == QCAP)
                    qexpn[kl] = ex1
                    rem[kl] = ex1 if mut == "rem-ex1" else ex1 + 1
            # JPK_RENORM2: both states, the exponent state first, then one refill
            n1 = n2 = 0
            first = mut != "renorm-mantissa-first"
            for which in ((0, 1) if first else (1, 0)):
                v = x if which == 0 else x2
                n = 0
                if v < RANS_L:
                    v = ((v << 8) | bq.take()) & 0xffffffff
                    n = 1
                    if v < RANS_L and mut != ("renorm-x-single-byte", "renorm-x2-single-byte")[which]:
                        v = ((v << 8) | bq.take()) & 0xffffffff
                        n = 2
                if which == 0:
                    x, n1 = v, n
                else:
                    x2, n2 = v, n
            if tracking:
                if n1 + n2:
                    _log(ev, f"bytes-{n1}{n2}")
                _log(ev, "slow-due-only", due and not n1 + n2)
                _log(ev, "slow-bytes-only", not due and n1 + n2 > 0)
                _log(ev, "slow-due-and-bytes", due and n1 + n2 > 0)
            bq.taken4 = n1 + n2 == 4
            if bq.nb < 4:
                bq.refill()
            bq.taken4 = False
        R[ra], R[rb] = x & 0xffffffff, x2 & 0xffffffff
        mysym[lanei] = sym & 0xffff

    t = 0
    while (t + 64 < rlen) if mut == "tile-bound-lt" else (t + 64 <= rlen):
        for j in range(0, 64, 2):
            symbol(0, 1, j)
            symbol(2, 3, j + 1)
        out[t: t + 64] = mysym
        t += 64
    left = rlen - t
    for j in range(left):
        symbol(0, 1, j)
        if mut != "tail-no-swap":
            R[0], R[2] = R[2], R[0]
            R[1], R[3] = R[3], R[1]
    out[t: t + left] = mysym[:left]
    if tracking:
        _log(ev, f"rlen-{rlen}", rlen in _RLENS)
        _log(ev, f"rlen-above-64-mod4-{rlen % 4}", rlen > 64 and rlen % 4 != 0)
        _log(ev, "tail-odd", left % 2 == 1)
        _log(ev, "queue-taken-equals-clen", bq.taken() == clen)
    states = any(r != RANS_L for r in R) and mut != "no-states-check"
    over = ((bq.taken() >= clen) if mut == "taken-ge-clen" else (bq.taken() > clen)) and mut != "no-taken-check"
    _log(ev, "refuse-states", states)
    _log(ev, "refuse-taken-over-clen", over)
    assert mut is not None or all(0 <= x <= 256 for x in out), "k_dec_rans emits 0..256 only, whatever the payload holds"
    return out, (1 if states or over else 0)


# ---- k_dec_rle ---------------------------------------------------------------------------------------------------------------------------
def rle(symbols, info, stale=None, mut=None, ev=None):
    """symbols: the packed RLE0 symbols of the chunk's BLOCK (the chunk's own start at info.rle_off; what lies behind the block's last
    symbol is STALE_SYM).  stale: what the chunk's rank array holds before the kernel runs -- None: the host cleared it.
    -> (the olen ranks, status bits: 2 = "rle mismatch")"""
    assert mut is None or mut in MUTANTS, mut
    base, rlen, olen = info.rle_off, info.rlen, info.olen
    nsym = len(symbols)

    def src(u):
        return int(symbols[base + u]) if 0 <= base + u < nsym else STALE_SYM

    dst = bytearray(olen) if stale is None else bytearray(stale[:olen])
    assert len(dst) == olen
    carry_s, bad_s = 0, 0
    tracking = ev is not None
    seen_zero = seen_other = False
    zeros = true_total = 0
    for b0 in range(0, rlen, PASS):
        if tracking:
            _log(ev, "rle-pass-with-carry", b0 > 0 and carry_s != 0)
        run = 0 if mut == "carry-not-added" else carry_s               # exclusive scan over the threads, in thread order
        tot = 0
        for t in range(b0, min(b0 + PASS, rlen)):
            sy = src(t)
            cnt = val = 0
            if sy > 256:
                _log(ev, "refuse-rle-symbol-over-256")
                bad_s |= 1
            if sy > 1:
                cnt, val = 1, sy - 1
                seen_other = True
                true_total += 1
            elif (t + 1 >= rlen and mut != "lookahead-unguarded") or src(t + 1) > 1:
                bits = nb = 0
                u = t
                floor = b0 if mut == "gather-stops-at-b0" else (-base if mut == "gather-past-chunk-start" else 0)
                while u >= floor and src(u) <= 1 and nb <= (22 if mut == "gather-limit-22" else 21):
                    assert mut is not None or 0 <= u < rlen, "k_dec_rle gathers outside the chunk's symbols"
                    bits = (bits | src(u) << nb) & 0xffffffff
                    nb += 1
                    u -= 1
                if nb > {"nb-limit-lower": 19, "nb-limit-21": 21}.get(mut, 20) and mut != "no-nb-limit":
                    _log(ev, "refuse-rle-21-digits")
                    bad_s |= 1
                else:
                    cnt = (((1 << nb) | bits) - 1) & 0xffffffff
                seen_zero = True
                zeros += cnt
                true_total += cnt
                if tracking:
                    first = u + 1
                    _log(ev, "rle-group-over-thread-edge", first // PER_THREAD != t // PER_THREAD)
                    _log(ev, "rle-group-over-pass-edge", first < b0)
                    _log(ev, "rle-group-at-chunk-start", first == 0)
                    _log(ev, "rle-group-at-chunk-end", t + 1 == rlen)
                    _log(ev, "rle-digits-end-then-digits-start", t + 1 == rlen and base + rlen < nsym and src(rlen) <= 1)
                    _log(ev, f"rle-group-{nb}-digits", nb in (1, 2, 19, 20))
            elif tracking:
                _log(ev, "rle-lookahead-over-pass-edge", (t + 1) % PASS == 0)
            if val:
                if (run <= olen) if mut == "run-le-olen" else (run < olen):
                    assert 0 <= run < olen, "k_dec_rle stores outside the chunk's rank array"
                    dst[run] = val & 0xff
                    if tracking:
                        _log(ev, "rle-store-at-olen-1", run == olen - 1)
                elif mut != "no-store-flag":
                    _log(ev, "refuse-rle-store-at-olen")
                    bad_s |= 1
            run = (run + cnt) & 0xffffffff                              # run, tot and carry_s are 32-bit registers
            tot = (tot + cnt) & 0xffffffff
        carry_s = (carry_s + tot) & 0xffffffff
    if tracking:
        _log(ev, "rle-no-zero", rlen > 0 and not seen_zero)
        _log(ev, "rle-one-zero", zeros == 1 and seen_other)
        _log(ev, "rle-only-zeros", rlen > 0 and not seen_other)
    mismatch = carry_s != olen and mut != "no-carry-check"
    _log(ev, "refuse-rle-short", mismatch and carry_s < olen)
    _log(ev, "refuse-rle-long", mismatch and carry_s > olen)
    _log(ev, "rle-count-wraps", true_total >> 32 != 0)
    return bytes(dst), (2 if mismatch or bad_s else 0)


# ---- the batch ---------------------------------------------------------------------------------------------------------------------------
def _align(x):
    return (x + 255) // 256 * 256


def dec_order(infos):
    """k_dec_order: 4096 buckets of 256 symbols, longest bucket first, arrival order inside a bucket (any order is a valid launch order)"""
    def bucket(rlen):
        return 4095 - min(rlen >> 8, 4095)
    return sorted(range(len(infos)), key=lambda c: (bucket(infos[c].rlen), c))


def _rank_decode_any(R, freq):
    """rank.cpp:96-151 on any byte array (the walk of the oracle's decoder, with a list long enough for every rank)"""
    order = sorted((s for s in range(256) if freq[s] > 0), key=lambda s: (-freq[s], s))
    lst = [0] * 257
    bpos, bend, pos = {}, {}, 0
    for s in order:
        lst[R[pos]] = s
        bpos[s], bend[s] = pos + 1, pos + freq[s]
        pos += freq[s]
    uniq = len(order)
    out = bytearray()
    sym = lst[0]
    for _ in range(len(R)):
        out.append(sym)
        if bpos.get(sym, 0) < bend.get(sym, 0):
            r = R[bpos[sym]]
            bpos[sym] += 1
            if r > 0:
                lst[:r] = lst[1: r + 1]
                lst[r] = sym
                sym = lst[0]
        elif uniq > 0:
            uniq -= 1
            lst[:max(uniq, 1)] = lst[1: max(uniq, 1) + 1]
            sym = lst[0]
    return bytes(out)


def decode(oracle, streams, caps, leads=None, mut=None, ev=None, arena=None):
    """jpk_ans_decode_batch of `streams` into capacities `caps` -> [(status, decoded bytes)].  arena: a bytearray that stands for the
    context's arena and is kept between calls (None: a fresh one, every byte STALE_RANK)"""
    assert mut is None or mut in MUTANTS, mut
    nblk = len(streams)
    leads = leads or [0] * nblk
    arena = bytearray() if arena is None else arena
    status = [OK] * nblk
    walked = [headers(s, cap, mut, None, b) for b, (s, cap) in enumerate(zip(streams, caps))]      # pass 1: counts and totals only
    cbase, nch_total = [], 0
    for b, (st, infos, _, _) in enumerate(walked):
        cbase.append(nch_total)
        if st != OK:
            status[b] = st
        else:
            nch_total += len(infos)
    out = [(status[b], b"") for b in range(nblk)]
    if nch_total == 0:
        return out
    off = _align(nblk * 56 + 64) + _align(nblk * 32 + 64)
    for bytes_ in (nblk * 4, nch_total * 40, nch_total * 1024, nch_total * 4):
        off += _align(bytes_ + 64)
    o_rle, o_ranks = [], []
    for b, (st, _, _, (tot_out, tot_rle)) in enumerate(walked):
        live = st == OK
        o_rle.append(off)
        off += _align((tot_rle if live else 0) * 2 + 64)
        o_ranks.append(off)
        off += _align((tot_out if live else 0) + 64)
    if len(arena) < off + 4096:
        arena.extend(bytes([STALE_RANK]) * (off + 4096 - len(arena)))
    before = bytes(arena)
    if mut != "no-rank-clear":
        arena[o_ranks[0]: off] = bytes(off - o_ranks[0])
    # pass 2 fills the chunk table at the block's global chunk base
    table = [None] * nch_total
    freq = [None] * nch_total
    for b, s in enumerate(streams):
        if status[b] != OK:
            continue
        st, infos, freqs, _ = headers(s, caps[b], mut, ev, b)
        assert st == OK and len(infos) == len(walked[b][1])
        table[cbase[b]: cbase[b] + len(infos)] = infos
        freq[cbase[b]: cbase[b] + len(infos)] = freqs
        _log(ev, "batch-block-offsets-nonzero", any(cbase[b] and ci.rle_off and ci.out_off for ci in infos))
    order = dec_order(table) if nch_total > 1024 else list(range(nch_total))
    _log(ev, "batch-order-not-identity", order != list(range(nch_total)))
    hs = [0] * nblk
    syms = [[STALE_SYM] * walked[b][3][1] if status[b] == OK else [] for b in range(nblk)]
    for c in order:
        ci = table[c]
        got, bits = rans(streams[ci.blk], ci, leads[ci.blk], mut, ev)
        syms[ci.blk][ci.rle_off: ci.rle_off + ci.rlen] = got
        hs[ci.blk] |= bits
    for b in range(nblk):
        if status[b] == OK:
            raw = np.array(syms[b], dtype="<u2").tobytes()
            arena[o_rle[b]: o_rle[b] + len(raw)] = raw
    for c in range(nch_total):
        ci = table[c]
        at = o_ranks[ci.blk] + ci.out_off
        ranks, bits = rle(syms[ci.blk], ci, arena[at: at + ci.olen], mut, ev)
        if ev is not None:
            was = np.frombuffer(before[at: at + ci.olen], dtype=np.uint8)
            _log(ev, "batch-zero-over-dense", int(((was != 0) & (was != STALE_RANK) & (np.frombuffer(ranks, dtype=np.uint8) == 0)).sum()))
        arena[at: at + ci.olen] = ranks
        hs[ci.blk] |= bits
    for b in range(nblk):
        if status[b] != OK:
            continue
        if hs[b]:
            out[b] = (E_CORRUPT, b"")
            continue
        parts = []
        for c in range(cbase[b], cbase[b] + len(walked[b][1])):
            ci = table[c]
            at = o_ranks[b] + ci.out_off
            r = np.frombuffer(bytes(arena[at: at + ci.olen]), dtype=np.uint8)
            f = np.array(freq[c], dtype=np.int32)
            if int(f.sum()) != ci.olen or (f < 0).any():
                parts = None
                break
            # a mutant's rank array need not be one: the oracle's decoder, like the reference's, trusts its input
            parts.append(oracle.rank_decode(r, f).tobytes() if mut is None else _rank_decode_any(r.tolist(), f.tolist()))
        out[b] = (OK, b"".join(parts)) if parts is not None else (E_CORRUPT, b"")
    return out


def front(stream, lead=0, mut=None, ev=None):
    """everything in front of the rank decoder for one stream at exact capacity: (status, infos, freq, totals, [symbols], [ranks], bits)
    -- what DETECTS compares"""
    status, infos, freqs, totals = headers(stream, 1 << 40, mut, ev)
    syms, ranks, bits = [STALE_SYM] * totals[1], [], 0
    if status == OK:
        for ci in infos:
            got, b = rans(stream, ci, lead, mut, ev)
            syms[ci.rle_off: ci.rle_off + ci.rlen] = got
            bits |= b
        for ci in infos:
            r, b = rle(syms, ci, None, mut, ev)
            ranks.append(r)
            bits |= b
    return status, infos, freqs, totals, syms, ranks, bits


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def text_of_ranks(ranks, seed=0):
    """the text whose move-to-front ranks over a list of all 256 byte values are `ranks`: pop the rank, reinsert in front (the coder's
    list starts in first-appearance order, so the first ranks it finds differ; the oracle's rank array is what the tests look at)"""
    lst = np.random.default_rng(seed).permutation(256).tolist()
    out = bytearray()
    for r in ranks:
        c = lst.pop(r)
        lst.insert(0, c)
        out.append(c)
    return np.frombuffer(bytes(out), dtype=np.uint8)


def runs_text(pairs):
    """a^k1 b^j1 a^k2 ...: `pairs` = (byte, count), ..."""
    return np.concatenate([np.full(n, b, dtype=np.uint8) for b, n in pairs])


def histogram_text(counts, seed):
    """a seeded shuffle of the multiset with counts[s] copies of byte s: the header's LEB lengths are the histogram's"""
    t = np.repeat(np.arange(256), counts).astype(np.uint8)
    np.random.default_rng(seed).shuffle(t)
    return t


def _two_byte_counts(n2, total=20000):
    """n2 counts of 127 (two LEB bytes), the others share the rest and stay below 127 (one byte): 256 + n2 frequency bytes"""
    c = np.zeros(256, dtype=np.int64)
    c[:n2] = 127
    rest, m = total - 127 * n2, 256 - n2
    c[n2:] = rest // m
    c[n2: n2 + rest % m] += 1
    assert c.sum() == total and c[n2:].max() < 127 and c.min() >= 1
    return c


# frequency bytes mod 64 -> what the three 3-byte length fields behind them do at the window's edge
HDR_EDGE = {62: "olen-since2", 63: "olen-since1", 59: "clen-since2", 60: "clen-since1", 56: "rlen-since2", 57: "rlen-since1", 55: "end-lane63"}
RLEN_TEXTS = (1, 2, 3, 63, 64, 65, 128, 129, 130, 131)


def _no_repeats(n, k=0):
    """n bytes over 11 symbols without two equal neighbours: no zero rank behind a symbol's first, so rlen = n"""
    return ((np.arange(n) * 7 + k) % 11 + 40 + k % 5).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    """the named one-chunk text as a read-only uint8 array"""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("rlen-"):
        t = _no_repeats(int(name[5:]))
    elif name == "class7":
        t = text_of_ranks(rng.integers(127, 256, 20000).tolist(), 1)
    elif name == "classes":
        # every class, rebuilds of classes 2..6: the class drawn evenly, the rank evenly inside it; ranks of zero come in runs
        e = rng.integers(0, 8, 20000)
        lo = np.array([0, 1, 3, 7, 15, 31, 63, 127])[e]
        hi = np.array([1, 3, 7, 15, 31, 63, 127, 256])[e]
        t = text_of_ranks((lo + rng.integers(0, 1 << 30, 20000) % (hi - lo)).tolist(), 2)
    elif name == "cap":
        r = np.full(282011, 3)
        r[rng.integers(0, 282011, 60)] = rng.integers(0, 256, 60)
        r[281000:] = rng.integers(0, 256, 1011)                       # the exponent entries of the other classes are at their floor by now
        t = text_of_ranks(r.tolist(), 3)
    elif name == "zeros-1MiB":
        t = np.full(CHUNK, 0x5A, dtype=np.uint8)
    elif name == "pairs":
        # the digit 0 (runs of one zero), the digit 1 (runs of two), rank 1 and rank 2, each 400 times on end
        t = np.concatenate((np.tile(np.array([1, 1, 2, 2], dtype=np.uint8), 400), np.tile(np.array([1, 1, 1, 2, 2, 2], dtype=np.uint8), 400),
                            np.tile(np.array([3, 4], dtype=np.uint8), 400), np.tile(np.array([5, 6, 7], dtype=np.uint8), 400)))
    elif name.startswith("hdr-"):
        b = {v: k for k, v in HDR_EDGE.items()}[name[4:]]
        t = histogram_text(_two_byte_counts(b), b)
    elif name == "freq-straddle":
        # value bytes 62..64 and 127..129 are 3-byte frequencies (two and one byte in the window before), 191..192 a 2-byte one
        c = np.ones(256, dtype=np.int64)
        c[62] = c[125] = 16510 + 5
        c[187] = 127
        t = runs_text([(s, int(c[s])) for s in range(256)])
    elif name == "digit-groups":
        # zero runs that put digit groups over thread and pass edges, from the chunk's start to its end; more than one pass
        parts = []
        for i in range(2600):
            parts += [(1, 2 + i % 7), (2, 1 + i % 3)]
        t = runs_text([(1, 5)] + parts + [(3, 1), (4, 1), (3, 70000), (4, 3)])
    elif name == "pass-edge":
        # two symbols: the more frequent one's bucket is 0 0 then 1500 times (rank 1, 0, 0, 0), in RLE0 symbols `0 0` then (2, 0, 0) on
        # end: the 1365th of these digit pairs lies at symbols 4095 and 4096, over the edge of the first pass
        t = runs_text([(1, 3)] + [(2, 1), (1, 4)] * 1500)
    elif name == "zeros-512KiB":
        t = np.full(CHUNK // 2, 0xC3, dtype=np.uint8)                 # 2^19 zeros: L = 2^19 + 1, the shortest chunk with a group of 19 digits
    elif name == "roll-after-22":
        # four symbols, 35 periods of: 190 rounds of three (rank 2: the pair model of class 1 goes to its low end), 320 rounds of four
        # (rank 3: the exponent entries of class 1 go to their floor), then two symbols at rank 1 -- two bytes for either state.  Of the
        # 36 such symbols one is followed by the refill that rolls the window, with the stream 0 or 3 bytes behind an aligned address
        t = np.tile(np.array([10, 20, 30] * 190 + [10, 20, 30, 40] * 320 + [30, 40], dtype=np.uint8), 35)
    elif name == "dense-5000":
        t = rng.integers(0, 256, 5000).astype(np.uint8)
    elif name == "zero-heavy-6000":
        t = runs_text([(7, 3000), (9, 2990), (7, 10)])
    else:
        raise KeyError(name)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    t.setflags(write=False)
    return t


CASES = (tuple(f"rlen-{n}" for n in RLEN_TEXTS) + ("class7", "classes", "cap", "zeros-1MiB", "pairs") + tuple(f"hdr-{v}" for v in HDR_EDGE.values()) +
         ("freq-straddle", "digit-groups", "pass-edge", "zeros-512KiB", "roll-after-22", "dense-5000", "zero-heavy-6000"))

# chain -> the texts whose streams are concatenated
CHAINS = {
    "chain-rlens": tuple(f"rlen-{n}" for n in RLEN_TEXTS),
    "chain-two": ("rlen-65", "dense-5000"),
    # a chunk whose rank array ends in zeros (the least frequent symbol's bucket: a head and a repeat), then one that starts with zeros
    "chain-digits": ("@ends-in-digits", "@starts-with-digits", "@ends-in-digits", "rlen-3"),
    "chain-70": tuple(f"@small-{n}" for n in range(1, 71)),
    "chain-63": ("@pad-50", "rlen-3"),                                # a stream of 319 bytes in front: the second header starts at 63 mod 64
}
BIG_CHAIN = tuple(f"@small-{1 + (n * 37) % 97 + (500 if n % 9 == 4 else 0)}" for n in range(1100))
BATCH = ("dense-5000", "chain-digits", "zero-heavy-6000", "chain-rlens", "rlen-1")


@functools.lru_cache(maxsize=None)
def part(name):
    if not name.startswith("@"):
        return case(name)
    if name == "@ends-in-digits":
        t = runs_text([(1, 9), (2, 4), (3, 2)])
    elif name == "@starts-with-digits":
        t = runs_text([(1, 6), (2, 1), (1, 2)])
    elif name.startswith("@pad-"):
        n = int(name[5:])
        t = (np.arange(n) * 13 + n) % 251
    elif name.startswith("@small-"):
        n = int(name[7:])
        t = _no_repeats(n, n) if n % 3 else runs_text([(n % 200 + 1, (n + 1) // 2), (n % 50 + 201, n // 2)]) if n > 1 else _no_repeats(1, 1)
    else:
        raise KeyError(name)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    t.setflags(write=False)
    return t


_streams = {}


def stream(oracle, name):
    """(the valid stream of a case, a chain or "big-chain", the text it decodes to): computed once, shared, left unchanged"""
    if name not in _streams:
        names = CHAINS[name] if name in CHAINS else (BIG_CHAIN if name == "big-chain" else (name,))
        texts = [part(n) for n in names]
        enc = {}
        for n, t in zip(names, texts):
            if n not in enc:
                enc[n] = oracle.ans_encode(t)
        s = np.concatenate([enc[n] for n in names])
        t = np.concatenate(texts)
        s.setflags(write=False)
        t.setflags(write=False)
        _streams[name] = (s, t)
    return _streams[name]


# ---- refused streams ---------------------------------------------------------------------------------------------------------------------
# Built field by field from the oracle's own pieces (leb_encode, model_pairs, rans_encode_pairs): for a valid text the result is the
# oracle's stream byte for byte (test_the_pieces_rebuild_the_oracles_stream), so any header field and any RLE0 symbol sequence can stand in
# an otherwise well-formed stream.  REFUSED: name -> builder(oracle) -> (stream bytes, out_cap); REASON: name -> the refuse-* events that
# fire on it (one, wherever the format lets one acceptance test fire alone).  STILL_ACCEPTED: the neighbours both model and oracle decode.
REFUSE_EVENTS = ("refuse-nlead-over-4", "refuse-since-over-window", "refuse-window-without-terminator", "refuse-header-truncated",
                 "refuse-freq-over-chunk", "refuse-olen-over-chunk", "refuse-rlen-over-olen", "refuse-clen-past-len", "refuse-clen-below-16",
                 "refuse-total-ne-olen", "refuse-capacity-at-chunk-1", "refuse-capacity-at-chunk-2", "refuse-capacity-later",
                 "refuse-states", "refuse-taken-over-clen", "refuse-rle-21-digits", "refuse-rle-store-at-olen", "refuse-rle-short",
                 "refuse-rle-long", "refuse-max-chunks", "refuse-ip-past-len", "refuse-rle-symbol-over-256")
INPUT_EVENTS = ("hdr-5-byte-value-wraps", "rle-count-wraps")          # what a crafted input is, not why it is refused
HEADER_REFUSALS = REFUSE_EVENTS[:13]
T0_LEN = 300


def base_text():
    """300 bytes over the values 0..22, no two neighbours equal: every count is one LEB byte, values 23..255 have count 0 (one byte
    0x80 each), and the text holds a zero byte"""
    return ((np.arange(T0_LEN) * 7) % 23).astype(np.uint8)


def side_text():
    return _no_repeats(40)


def leb5(v, extra=0):
    """the five-byte form of the 32-bit value v; extra: bits 32..34 of the 35 the five bytes hold, which a 32-bit register drops"""
    raw = (v - LEB_OFF[3]) & 0xffffffff
    return bytes([(raw >> 28) | (extra << 4), (raw >> 21) & 0x7f, (raw >> 14) & 0x7f, (raw >> 7) & 0x7f, (raw & 0x7f) | 0x80])


def payload_of(oracle, syms):
    """the rANS payload of an RLE0 symbol sequence (any sequence over 0..256)"""
    return oracle.rans_encode_pairs(oracle.model_pairs(np.asarray(syms, dtype=np.uint16))).tobytes()


def fields_of(oracle, freq, olen, clen, rlen):
    """the header's 259 values, one bytes object each"""
    return [oracle.leb_encode(int(v)) for v in list(freq) + [olen, clen, rlen]]


def chunk_of_symbols(oracle, freq, olen, syms):
    pay = payload_of(oracle, syms)
    return fields_of(oracle, freq, olen, len(pay), len(syms)), pay


def chunk_of_text(oracle, text):
    """(fields, payload, freq) of the chunk the oracle's encoder makes of a text of at most 2^20 bytes"""
    r, f = oracle.rank_encode(text)
    fields, pay = chunk_of_symbols(oracle, f, len(text), oracle.rle_encode(r))
    return fields, pay, f


def _join(fields, pay):
    return b"".join(fields) + bytes(pay)


def digits(v):
    """the RLE0 digit group of a run of v zeros: v + 1 in binary without its leading one"""
    return [int(c) for c in bin(v + 1)[3:]]


def _base(oracle):
    fields, pay, f = chunk_of_text(oracle, base_text())
    assert all(len(x) == 1 for x in fields[:256]) and not f[23:].any() and f[0] > 0
    return fields, pay, f


def _side(oracle):
    return oracle.ans_encode(side_text()).tobytes()


def _placed(oracle, bad, k, ends, olen=T0_LEN):
    """`bad` as chunk k (1 or 3) of a chain of four with valid neighbours; ends: nothing can follow it (the stream is cut in it)"""
    v = _side(oracle)
    n = (k - 1) + (0 if ends else 4 - k)
    return v * (k - 1) + bad + (b"" if ends else v * (4 - k)), n * len(side_text()) + olen


def _rle_freq(olen):
    f = [0] * 256
    f[0], f[65], f[66] = 1, olen - 2, 1
    return f


def _hdr_case(edit, ends=False):
    """edit(oracle, fields, pay, freq) -> the bad chunk's bytes, from the base chunk's pieces"""
    def at(k):
        def build(oracle):
            fields, pay, f = _base(oracle)
            return _placed(oracle, edit(oracle, list(fields), pay, f.tolist()), k, ends)
        return build
    return at


def _set(i, value):
    def edit(oracle, fields, pay, f):
        fields[i] = value(oracle, fields, pay, f) if callable(value) else value
        return _join(fields, pay)
    return edit


def _refreq(changes, olen=None):
    def edit(oracle, fields, pay, f):
        for s, v in changes.items():
            fields[s] = leb5(v) if v >= 1 << 31 else oracle.leb_encode(v)
        if olen is not None:
            fields[256] = oracle.leb_encode(olen)
        return _join(fields, pay)
    return edit


def _rlen_plus_1(oracle, fields, pay, f):
    fields, pay = chunk_of_symbols(oracle, f, T0_LEN, [2] * (T0_LEN + 1))
    return _join(fields, pay)


def _empty_chunk(oracle, clen=16):
    return _join(fields_of(oracle, [0] * 256, 0, clen, 0), RANS_L.to_bytes(4, "little") * 4)


# name -> (edit of the base chunk, the stream ends in it, the events that fire)
_HDR = {
    "nlead-6-bytes-in-window": (_set(30, bytes(5) + b"\x80"), False, ("refuse-nlead-over-4",)),
    "since-5-at-window-edge": (_set(59, bytes(5) + b"\x80"), False, ("refuse-since-over-window",)),
    "window-of-64-continuation-bytes": (_set(64, bytes(64) + b"\x80"), False, ("refuse-window-without-terminator",)),
    "cut-at-window-edge": (lambda o, fields, pay, f: _join(fields, pay)[:128], True, ("refuse-header-truncated",)),
    # the one byte of the last window is a terminator; the 63 lanes behind it read as 0, continuation bytes
    "cut-one-byte-past-window-edge": (lambda o, fields, pay, f: _join(fields, pay)[:129], True, ("refuse-since-over-window",)),
    "freq-chunk-plus-1": (_refreq({30: CHUNK + 1}), False, ("refuse-freq-over-chunk", "refuse-total-ne-olen")),
    # two counts of 2^31: their 32-bit sum is 0, `total` is olen again and only the limit on a single count refuses
    "freq-two-of-2^31": (_refreq({30: 1 << 31, 31: 1 << 31}), False, ("refuse-freq-over-chunk",)),
    "olen-chunk-plus-1": (_refreq({30: CHUNK - T0_LEN, 31: 1}, CHUNK + 1), False, ("refuse-olen-over-chunk",)),
    "rlen-olen-plus-1": (_rlen_plus_1, False, ("refuse-rlen-over-olen",)),
    # five bytes whose 35 bits wrap onto a value with bit 31 set: above olen as the kernel reads it, below zero as the oracle does
    "rlen-top-bit-set": (_set(258, lambda o, fields, pay, f: leb5(0x80000000 | 3, 5)), False, ("refuse-rlen-over-olen",)),
    "clen-past-len": (_set(257, lambda o, fields, pay, f: o.leb_encode(len(pay) + 1)), True, ("refuse-clen-past-len",)),
    "total-olen-minus-1": (_set(0, lambda o, fields, pay, f: o.leb_encode(f[0] - 1)), False, ("refuse-total-ne-olen",)),
    "total-olen-plus-1": (_set(0, lambda o, fields, pay, f: o.leb_encode(f[0] + 1)), False, ("refuse-total-ne-olen",)),
}


def _clen_15(k):
    def build(oracle):
        return _placed(oracle, _empty_chunk(oracle, 15)[:-1], k, True, 0)
    return build


def _capacity(nvalid):
    def build(oracle):
        fields, pay, _ = _base(oracle)
        return _side(oracle) * nvalid + _join(fields, pay), nvalid * len(side_text()) + T0_LEN - 1
    return build


def _flipped(oracle):
    """one bit of one payload byte behind the 16 state bytes: the last such bit, counted from the payload's end, under which the final
    states miss RANS_L and no byte beyond clen is taken (a flip may also send the decoder for more bytes than the chunk has; the model
    says which flips do)"""
    fields, pay, _ = _base(oracle)
    for at in range(len(pay) - 1, 15, -1):
        for bit in range(8):
            s = _join(fields, pay[:at] + bytes([pay[at] ^ (1 << bit)]) + pay[at + 1:])
            if verdict(s, T0_LEN)[1] == ("refuse-states",):
                return s, T0_LEN
    raise AssertionError("no flip isolates the states check")


def _truncated(oracle):
    fields, pay, _ = _base(oracle)
    fields[257] = oracle.leb_encode(len(pay) - 1)
    return _join(fields, pay[:-1]), T0_LEN


def second_text_for(last):
    """a text whose header starts with the byte `last`: that byte is the LEB form of its count of zero bytes, or the first of two"""
    zeros = (last & 0x7f) if last & 0x80 else (last << 7) + 127
    return np.concatenate((np.zeros(zeros, dtype=np.uint8), _no_repeats(30)))


def _taken_over_clen(oracle):
    """A, B with A's clen one short and B's first header byte lent to A as its last payload byte: every state of A ends at RANS_L and
    only taken() > clen refuses it; the oracle refuses through p >= end"""
    fields, pay, _ = _base(oracle)
    b = second_text_for(pay[-1])
    enc_b = oracle.ans_encode(b).tobytes()
    assert enc_b[0] == pay[-1]
    fields[257] = oracle.leb_encode(len(pay) - 1)
    return _join(fields, pay) + enc_b[1:], T0_LEN + len(b)


def _rle_case(make):
    """make() -> (symbols, olen): under a valid header whose counts sum to olen"""
    def build(oracle):
        syms, olen = make()
        fields, pay = chunk_of_symbols(oracle, _rle_freq(olen), olen, syms)
        return _join(fields, pay), olen
    return build


_G = [1] * 6                                                          # a group of six digits: 126 zeros, so that rlen stays below olen


def _n2(n):
    return [2] * n                                                    # n ranks of 1, one byte each


def _wraps():
    """2048 x (2^21 - 2 zeros, a separator) and a last group of 2^20 + 2048 zeros: 2^32 + 2^20 in all, which a 32-bit register holds as
    2^20 = olen.  Every separator lands at run >= olen; only their refused stores tell"""
    syms = ([1] * 20 + [2]) * 2048 + digits((1 << 20) + 2048)
    assert len(syms) == 43028
    return syms, CHUNK


REFUSED = collections.OrderedDict()
REASON = {}
for _n, (_edit, _ends, _why) in _HDR.items():
    for _k in (1, 3):
        REFUSED[f"{_n}@{_k}"] = _hdr_case(_edit, _ends)(_k)
        REASON[f"{_n}@{_k}"] = _why
for _k in (1, 3):
    REFUSED[f"clen-15@{_k}"] = _clen_15(_k)
    REASON[f"clen-15@{_k}"] = ("refuse-clen-below-16",)
for _n, _b, _why in (
        ("capacity-at-chunk-1", _capacity(0), ("refuse-capacity-at-chunk-1",)),
        ("capacity-at-chunk-2", _capacity(1), ("refuse-capacity-at-chunk-2",)),
        ("capacity-at-chunk-4", _capacity(3), ("refuse-capacity-later",)),
        ("rans-last-byte-flipped", _flipped, ("refuse-states",)),
        # the queue's byte-wise load() gives 0 for the missing byte: the states miss RANS_L and one byte more than clen was taken
        ("rans-payload-truncated", _truncated, ("refuse-states", "refuse-taken-over-clen")),
        ("rans-taken-over-clen", _taken_over_clen, ("refuse-taken-over-clen",)),
        ("rle-21-digits-at-start", _rle_case(lambda: ([0] * 21 + _n2(50) + _G + _n2(50), 226)), ("refuse-rle-21-digits",)),
        ("rle-21-digits-in-the-middle", _rle_case(lambda: (_n2(50) + _G + _n2(25) + [0, 1] * 10 + [1] + _n2(25), 226)), ("refuse-rle-21-digits",)),
        ("rle-21-digits-over-pass-edge", _rle_case(lambda: (_G + _n2(4085) + [1] * 21 + _n2(50), 126 + 4135)), ("refuse-rle-21-digits",)),
        ("rle-21-digits-at-end", _rle_case(lambda: (_n2(50) + _G + _n2(50) + [0] * 21, 226)), ("refuse-rle-21-digits",)),
        ("rle-25-digits", _rle_case(lambda: (_n2(50) + _G + _n2(25) + [1, 0] * 12 + [1] + _n2(25), 226)), ("refuse-rle-21-digits",)),
        # the last rank lands at run == olen: its store is refused, and with it the count is olen + 1
        ("rle-store-at-olen", _rle_case(lambda: (_n2(50) + _G + _n2(50), 225)), ("refuse-rle-store-at-olen", "refuse-rle-long")),
        ("rle-short", _rle_case(lambda: (_n2(50) + _G + _n2(50), 227)), ("refuse-rle-short",)),
        ("rle-long-by-digits", _rle_case(lambda: (_n2(50) + digits(10), 59)), ("refuse-rle-long",)),
        ("rle-count-wraps", _rle_case(_wraps), ("refuse-rle-store-at-olen",))):
    REFUSED[_n] = _b
    REASON[_n] = _why


def _surplus(k):
    def build(oracle):
        fields, pay, _ = _base(oracle)
        fields[257] = oracle.leb_encode(len(pay) + k)
        return _join(fields, pay + bytes([0x5A, 0x80, 0xFF, 0x00][:k])), T0_LEN
    return build


def _with_empty(where):
    def build(oracle):
        v, e = _side(oracle), _empty_chunk(oracle)
        return {"alone": e, "first": e + v + v, "middle": v + e + v, "last": v + v + e}[where], 0 if where == "alone" else 2 * len(side_text())
    return build


def _wrapped_olen(oracle):
    fields, pay, _ = _base(oracle)
    fields[256] = leb5(T0_LEN, 7)
    return _join(fields, pay), T0_LEN


MOVED = (2, 7)                                                        # the counts moved by +1 and -1


def moved_text():
    return np.random.default_rng(0).integers(0, 23, T0_LEN).astype(np.uint8)


def _freq_two_moved(oracle):
    """the sum is right, two counts are not: the header accepts, the ranks are the valid ones, and the bytes are whatever the rank
    decoder makes of buckets that start one place off.  rank_rows_model says when that is defined: the text holds a zero byte, and no
    two buckets name the same start position -- the base text cannot serve, every rank behind a first one is 22 there, and for two
    buckets that name one position the kernel's winner and the reference's differ by design (the test asserts that this text and this
    pair are inside the scope)"""
    fields, pay, f = chunk_of_text(oracle, moved_text())
    fields[MOVED[0]], fields[MOVED[1]] = oracle.leb_encode(int(f[MOVED[0]]) + 1), oracle.leb_encode(int(f[MOVED[1]]) - 1)
    return _join(fields, pay), T0_LEN


def _valid_base(oracle):
    fields, pay, _ = _base(oracle)
    return _join(fields, pay), T0_LEN


STILL_ACCEPTED = collections.OrderedDict(
    [("valid-base", _valid_base)] + [(f"surplus-payload-{k}", _surplus(k)) for k in (1, 3, 4)] +
    [(f"empty-chunk-{w}", _with_empty(w)) for w in ("alone", "first", "middle", "last")] +
    [("olen-5-bytes-wrapped", _wrapped_olen), ("freq-equals-chunk", lambda oracle: (stream(oracle, "zeros-1MiB")[0].tobytes(), CHUNK)),
     ("freq-two-moved", _freq_two_moved)])

_built = {}


def crafted(oracle, name):
    """(stream as a read-only uint8 array, out_cap) of a REFUSED or STILL_ACCEPTED name: built once, shared, left unchanged"""
    if name not in _built:
        s, cap = (REFUSED.get(name) or STILL_ACCEPTED[name])(oracle)
        a = np.frombuffer(bytes(s), dtype=np.uint8)
        _built[name] = (a, cap)
    return _built[name]


def verdict(stream, out_cap, lead=0, mut=None):
    """-> (status, the refuse-* and input events that fired, the stage that refused: "headers", "payload" or None).  The model's bounds
    assertions run on the way: this is the walk every stream takes before a kernel sees it"""
    ev = {}
    status, infos, _, totals = headers(stream, out_cap, mut, ev)
    stage = "headers" if status != OK else None
    if status == OK:
        syms, bits = [STALE_SYM] * totals[1], 0
        for ci in infos:
            got, b = rans(stream, ci, lead, mut, ev)
            syms[ci.rle_off: ci.rle_off + ci.rlen] = got
            bits |= b
        for ci in infos:
            bits |= rle(syms, ci, None, mut, ev)[1]
        if bits:
            status, stage = E_CORRUPT, "payload"
    return status, tuple(sorted(e for e in ev if e in REFUSE_EVENTS)), stage, {e: ev[e] for e in ev if e in INPUT_EVENTS}
