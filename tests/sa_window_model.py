"""Plain-Python restatement of what the doubling rounds of the forward BWT's suffix sort (jampack_amd/csrc/bwt_fwd_rounds.hip) see of an
input: the active list of a round as a sequence of group sizes, and where those groups lie against the 1024-slot windows (SEG_TILE,
bwt_fwd.hpp) the kernels cut the list into.  No GPU, no library: the crafted texts of test_sa_window_model.py and test_gpu_sa_windows.py
are built here, and this model says which routes of the kernels they reach.

What the model rests on.  With plain byte keys (JPK_KEY_BITS=8) round 0 sorts on the first DEPTH = 7 bytes of every suffix, zero padded.
If the text has no zero byte, no run of 7 or more equal bytes (no run members, RUNF) and ends in h distinct bytes that occur nowhere
else, every suffix whose h-byte prefix would run off the text, or would hold one of the ending's bytes, is alone with its prefix.  The
list a round starts with is then the suffixes whose h-byte prefix occurs more than once, grouped by that prefix, the groups in
lexicographic order of the prefix: h = 7 for round 1, h = 14 for round 2 (round 1 splits every group by the rank of the suffix 7
further on, which is the rank of ITS 7-byte prefix).  Window geometry depends on nothing but the sizes of the groups in that order.
"""
import functools
from collections import Counter

import numpy as np

WIN = 1024          # slots per window of the active list (SEG_TILE); a group above WIN members is a large group
DEPTH = 7           # bytes per key of round 0 with plain byte keys
KB = 7              # bytes packed into one 64-bit word of a prefix key
UNIT = 120          # the forward BWT sorts len - len % 120 bytes (JPK_BWT_UNITS)

# byte values: who may use what (the two builders share the plan)
STEM_LO, STEM_HI = 1, 40                # stem bytes of scattered(); prescribed() keeps [1, 19] for its leading pairs
LEAD1 = tuple(range(1, 9))              # prescribed(): first byte of a stem, the smallest bytes of the text
LEAD2 = tuple(range(9, 20))             # prescribed(): second byte of a stem
PSTEM_LO = 20
DIGIT0, BASE = 50, 200                  # tail digits: bytes 50..249
REC_END = 0xFF                          # last byte of every record, the text's largest byte
ENDING = tuple(range(41, 50)) + tuple(range(250, 255))      # 14 distinct bytes used nowhere else
SEPS = (60, 61, 62, 63, 64, 65)

KINDS = (
    # groups of at most WIN members: sorted in LDS by the window they start in (k_seg_round)
    "small-inside", "small-straddle", "1024-aligned", "1024-straddle",
    # groups above WIN members: cut into pieces (win_geometry / k_win_count / k_win_pieces), sorted by k_lg_*
    "large-1025", "large-2-windows", "large-3-windows", "large-4-or-more-windows", "large-starts-at-slot-0", "large-starts-at-last-slot",
    "large-ends-on-edge", "large-ends-list",
    # windows
    "window-inside-large", "A+B", "A+small+B", "small-tail+B",
    # the list's end
    "last-window-ragged", "list-multiple-of-1024", "last-window-single-slot",
)


def bits_for(v):
    """jpk_bits_for (common.hpp)"""
    return int(v).bit_length()


def lg_digit_bits(n):
    """(passes, digit width) of the large groups' radix sort for a block of n sorted bytes: lg_digit_bits of bwt_fwd_rounds.hip"""
    kbits = bits_for(3 * n)
    npass = max((kbits + 7) // 8, 1)
    return npass, max((kbits + npass - 1) // npass, 4)


def longest_run(t):
    t = np.asarray(t, dtype=np.uint8)
    if len(t) == 0:
        return 0
    edges = np.flatnonzero(np.concatenate(([True], t[1:] != t[:-1], [True])))
    return int(np.diff(edges).max())


def _prefix_words(t, h):
    """the h-byte prefixes at positions 0 .. len(t) - h as 64-bit words of 7 bytes each, big endian, most significant word first"""
    n = len(t) - h + 1
    words = []
    for w0 in range(0, h, KB):
        w = np.zeros(n, dtype=np.uint64)
        for k in range(w0, min(w0 + KB, h)):
            w = (w << np.uint64(8)) | t[k: k + n].astype(np.uint64)
        words.append(w)
    return words


def layout(t, h):
    """sizes of the groups of two or more suffixes that share their first h bytes, in the order of that prefix: the list of the round
    that compares at distance h"""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    n = len(t)
    assert n >= 2 * h
    assert not (t == 0).any(), "premise: no zero byte"
    assert longest_run(t) < DEPTH, "premise: no run of 7 or more equal bytes"
    end = t[n - h:]
    assert len(set(end.tolist())) == h and not np.isin(t[: n - h], end).any(), "premise: the last h bytes are distinct and occur nowhere else"
    words = _prefix_words(t, h)
    order = np.lexsort(words[::-1])
    new = np.zeros(len(order), dtype=bool)
    new[0] = True
    for w in words:
        ws = w[order]
        new[1:] |= ws[1:] != ws[:-1]
    sizes = np.diff(np.concatenate((np.flatnonzero(new), [len(order)])))
    return sizes[sizes > 1].astype(np.int64)


def large_members(sizes):
    """members of groups above WIN: what k_win_count adds up in SaState::lc"""
    sizes = np.asarray(sizes, dtype=np.int64)
    return int(sizes[sizes > WIN].sum())


def kind_counts(sizes):
    """how often a list of these group sizes shows every geometry kind of KINDS"""
    sizes = np.asarray(sizes, dtype=np.int64)
    c = Counter()
    if len(sizes) == 0:
        return c
    ends = np.cumsum(sizes)
    starts = ends - sizes
    m = int(ends[-1])
    for gs, ge, sz in zip(starts.tolist(), ends.tolist(), sizes.tolist()):
        crosses = gs // WIN != (ge - 1) // WIN
        if sz <= WIN:
            c["small-straddle" if crosses else "small-inside"] += 1
            if sz == WIN:
                c["1024-straddle" if gs % WIN else "1024-aligned"] += 1
            continue
        nt = (ge - 1) // WIN - gs // WIN + 1                       # pieces of the group: Piece::nt
        c["large-1025"] += sz == WIN + 1
        c["large-2-windows" if nt == 2 else "large-3-windows" if nt == 3 else "large-4-or-more-windows"] += 1
        c["large-starts-at-slot-0"] += gs % WIN == 0
        c["large-starts-at-last-slot"] += gs % WIN == WIN - 1
        c["large-ends-on-edge"] += ge % WIN == 0
        c["large-ends-list"] += ge == m
    for base in range(0, m, WIN):
        wend = min(base + WIN, m)
        gi = int(np.searchsorted(starts, base, side="right")) - 1          # the group that holds the window's first slot
        gl = int(np.searchsorted(starts, wend - 1, side="right")) - 1      # the window's last group
        spill = starts[gi] < base
        if gi == gl:
            c["window-inside-large"] += bool(spill and sizes[gi] > WIN)     # no head in the window
            continue
        has_b = sizes[gl] > WIN
        if spill and sizes[gi] > WIN and has_b:
            c["A+B" if gl == gi + 1 else "A+small+B"] += 1
        if spill and sizes[gi] <= WIN and has_b:
            c["small-tail+B"] += 1
    c["last-window-ragged"] += m % WIN != 0
    c["list-multiple-of-1024"] += m % WIN == 0
    c["last-window-single-slot"] += m % WIN == 1
    return Counter({k: int(v) for k, v in c.items() if v})


def kinds(sizes):
    return set(kind_counts(sizes))


# ---- builders --------------------------------------------------------------------------------------------------------------------
def _chain(rng, rows, length, lo, hi):
    """rows x length random bytes of [lo, hi], no two equal neighbours in a row"""
    span = hi - lo + 1
    out = np.empty((rows, length), dtype=np.int64)
    out[:, 0] = rng.integers(0, span, rows)
    for k in range(1, length):
        out[:, k] = (out[:, k - 1] + rng.integers(1, span, rows)) % span
    return (out + lo).astype(np.uint8)


def _records(rng, stems, counts):
    """one record per copy of every stem -- the stem, the copy number in base 200 (little endian, bytes 50..249), 0xFF -- shuffled"""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.max() < BASE ** 3
    stem_of = np.repeat(np.arange(len(counts)), counts)
    copy = np.concatenate([np.arange(c) for c in counts])
    rec = np.empty((len(stem_of), stems.shape[1] + 4), dtype=np.uint8)
    rec[:, : stems.shape[1]] = stems[stem_of]
    for k in range(3):
        rec[:, stems.shape[1] + k] = DIGIT0 + (copy // BASE ** k) % BASE
    rec[:, -1] = REC_END
    return rec[rng.permutation(len(rec))]


def _pad(rng, length, lo):
    """random bytes that bring a text of `length` bytes to a multiple of 120: the forward BWT sorts whole units of 120 bytes and copies
    the rest (bwt.cpp:29-33), and every crafted text is to be sorted to its end"""
    return _chain(rng, 1, UNIT - 1, lo, STEM_HI)[0][: -length % UNIT]


def scattered(seed, counts, stem_len=DEPTH):
    """counts[i] copies of stem i (stem_len bytes of 1..40) wherever the shuffle puts them.  The stems' groups lie where chance puts
    them; stem_len > 7 gives deep stems whose groups survive into round 2."""
    rng = np.random.default_rng(seed)
    stems = _chain(rng, len(counts), stem_len, STEM_LO, STEM_HI)
    body = _records(rng, stems, counts).reshape(-1)
    return np.concatenate((body, _pad(rng, len(body) + len(ENDING), STEM_LO), np.array(ENDING, dtype=np.uint8)))


def prescribed(seed, sizes, stem_len=DEPTH, list_mod=None):
    """The round-1 list starts with groups of exactly `sizes`, in that order, and ends with them once more.  Stem i starts with the pair
    (LEAD1[i // 11], LEAD2[i % 11]): bytes that occur nowhere else, below every other byte, rising with i -- so the stems themselves
    are the list's first groups.  Every record ends in 0xFF, the largest byte, and so does the two-byte opening: 0xFF + the first six
    bytes of stem i are the list's last groups.  list_mod: two or three copies of random strings are added in front of the ending so
    that the list's length is list_mod modulo 1024 (a string of L + 6 bytes that occurs k times adds L groups of k).  Random bytes that
    repeat nothing bring the length to a multiple of 120."""
    assert len(sizes) <= len(LEAD1) * len(LEAD2) and stem_len >= DEPTH
    rng = np.random.default_rng(seed)
    i = np.arange(len(sizes))
    lead = np.stack((np.array(LEAD1)[i // len(LEAD2)], np.array(LEAD2)[i % len(LEAD2)]), axis=1).astype(np.uint8)
    stems = np.concatenate((lead, _chain(rng, len(sizes), stem_len - 2, PSTEM_LO, STEM_HI)), axis=1)
    body = np.concatenate((np.array([DIGIT0, REC_END], dtype=np.uint8), _records(rng, stems, sizes).reshape(-1)))
    fill = _chain(rng, 2, WIN + 8, PSTEM_LO, STEM_HI)
    pad = _chain(rng, 1, UNIT - 1, PSTEM_LO, STEM_HI)[0]
    ending = np.array(ENDING, dtype=np.uint8)

    def text(la, lb):
        parts, sep = [body], iter(SEPS)
        for u, length, copies in ((fill[0], la, 2), (fill[1], lb, 3)):
            for _ in range(copies if length else 0):
                parts += [u[: length + DEPTH - 1], np.array([next(sep)], dtype=np.uint8)]
        length = sum(len(p) for p in parts) + len(ending)
        return np.concatenate(parts + [pad[: -length % UNIT], ending])

    if list_mod is None:
        return text(0, 0)
    need = (list_mod - int(layout(text(0, 0), DEPTH).sum())) % WIN
    if need == 1:
        need += WIN
    lb = need % 2
    t = text((need - 3 * lb) // 2, lb)
    assert int(layout(t, DEPTH).sum()) % WIN == list_mod
    return t


# ---- the crafted texts -------------------------------------------------------------------------------------------------------------
COUNTS = (2, 3, 5, 40, 300, 1000, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 3100, 5000)
DEEP_COUNTS = (2, 3, 40, 300, 1000, 1024, 1025, 1100, 2049, 3100)
DEEP_STEM = 16
# slot of every leading group:      0     1024  2047  3072  5120  6145  7169  10169 15169 15179 17179 18179 (ends 19379)
EDGE_SIZES = (1024, 1023, 1025, 2048, 1025, 1024, 3000, 5000, 10, 2000, 1000, 1200)
TEXTS = ("period-2", "one-large", "edges-56k", "edges-213k", "scatter-650k", "scatter-866k", "deep", "deeper")
DEEP = ("deep", "deeper")               # stems of 14 bytes and more: their groups are still there in round 2


@functools.lru_cache(maxsize=None)
def crafted(name):
    """the crafted texts by name (read-only: share, do not change)"""
    t = {
        # two groups of about 2090 and nothing else, in a block short enough for two radix passes of 7 bits
        "period-2": lambda: np.concatenate((np.tile(np.array([30, 31], dtype=np.uint8), 2093), np.array(ENDING, dtype=np.uint8))),
        "one-large": lambda: prescribed(11, (600, 1025), list_mod=1),
        "edges-56k": lambda: prescribed(12, (1023, 1025, 1024, 2047)),
        "edges-213k": lambda: prescribed(13, EDGE_SIZES, list_mod=0),
        "scatter-650k": lambda: scattered(1, COUNTS * 3),
        "scatter-866k": lambda: scattered(2, COUNTS * 4),
        "deep": lambda: scattered(3, DEEP_COUNTS * 2, DEEP_STEM),
        # stems longer than the variable-length keys of the default build reach: large groups in its round 1 too
        "deeper": lambda: scattered(4, DEEP_COUNTS, 3 * DEEP_STEM),
    }[name]()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def crafted_layout(name, h):
    s = layout(crafted(name), h)
    s.setflags(write=False)
    return s
