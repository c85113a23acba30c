"""Plain-Python restatement of how the encoder's adaptive-model kernels (k_adapt_* in jampack_amd/csrc/ans_enc_model.hip) cut the nine
recurrences of a chunk into 4096-item segments and what becomes of every segment.  No GPU, no library: the crafted streams of
test_adapt_segment_model.py and test_gpu_adapt_merge.py are built here, and this model says which routes of the kernels they reach.

One step of a recurrence is x += (mix - x) >> 5 with mix = i if i <= sym else i + 65536 - A (an arithmetic shift: floor).  The step
is monotone in x, so a segment can be walked from the two extreme states: where the two ends have met, every start state has.
"""
import numpy as np

SEG = 4096          # items per segment (ATILE)
WARM = 320          # items walked in front of a segment with the two extreme states (AD_WARM_DEFAULT)
EXPO = (0, 2, 4, 8, 16, 32, 64, 128, 257)       # class e covers the symbols [EXPO[e], EXPO[e + 1])
KINDS = ("first", "resolved", "identity", "merge", "plateau-merge", "table")


def step(x, i, sym, A):
    mix = i if i <= sym else i + 65536 - A
    return x + ((mix - x) >> 5)


def sym_class(s):
    if s < 2:
        return 0
    if s >= 128:
        return 7
    return int(s).bit_length() - 1


def uniform_cdf(A, i):
    scale = 65536 // A
    return i * scale + (65536 - scale * A)


def recurrences(symbols):
    """The nine item streams of one chunk: (name, i, A, items).  Seven exponent entries over the class of every symbol, two mantissa
    models over the low bit of the class-0 and the class-1 symbols in class order."""
    cls = [sym_class(int(s)) for s in symbols]
    out = [("exp%d" % i, i, 8, cls) for i in range(1, 8)]
    for c in (0, 1):
        out.append(("mant%d" % c, 1, 2, [int(s) & 1 for s, e in zip(symbols, cls) if e == c]))
    return out


def classify(i, A, items, exp):
    """One dict per segment: kind, and for the merged kinds `merge` = items of the segment after which the two ends are equal (every
    output from that item on is exact whatever the start state was); for a plateau lane also `reach` = index in the segment of the
    first symbol that reaches the entry (in front of it the entry does not move)."""
    smin, smax = i, i + 65536 - A
    segs = []
    for k in range((len(items) + SEG - 1) // SEG):
        t0, t1 = k * SEG, min((k + 1) * SEG, len(items))
        if k == 0:
            segs.append({"kind": "first"})
            continue
        lo, hi = smin, smax
        for t in range(t0 - WARM, t0):
            lo, hi = step(lo, i, items[t], A), step(hi, i, items[t], A)
        assert hi - lo <= 31, "the warm-up leaves at most 32 candidate start states"
        if lo == hi:
            segs.append({"kind": "resolved"})
            continue
        plateau = exp and hi == smax and lo == smax - 31
        reach = next((t - t0 for t in range(t0, t1) if items[t] >= i), None) if plateau else None
        if plateau and reach is None:
            segs.append({"kind": "identity"})
            continue
        merge = None
        for t in range(t0, t1):
            lo, hi = step(lo, i, items[t], A), step(hi, i, items[t], A)
            if lo == hi:
                merge = t - t0 + 1
                break
        if merge is None:
            segs.append({"kind": "table", "reach": reach})
        elif plateau:
            segs.append({"kind": "plateau-merge", "merge": merge, "reach": reach})
        else:
            segs.append({"kind": "merge", "merge": merge})
    return segs


def classify_chunk(symbols):
    """{recurrence name: [segment dict, ...]} for the symbols of one chunk."""
    return {name: classify(i, A, items, name.startswith("exp")) for name, i, A, items in recurrences(symbols)}


def exact_states(i, A, items):
    """The sequential reference: the entry's value in front of every item."""
    x, out = uniform_cdf(A, i), []
    for s in items:
        out.append(x)
        x = step(x, i, s, A)
    return out


# ---- the crafted streams ------------------------------------------------------------------------------------------------------
CLASS_P = (.30, .40, .10, .07, .05, .04, .03, .01)


def mixed(rng, n):
    """classes 0..7 with the probabilities CLASS_P, a uniform symbol inside the class's range"""
    cls = rng.choice(8, size=n, p=CLASS_P)
    lo = np.asarray(EXPO[:8])[cls]
    hi = np.asarray(EXPO[1:])[cls]
    return (lo + np.floor(rng.random(n) * (hi - lo)).astype(np.int64)).astype(np.uint16)


def bits(rng, n):
    return rng.integers(0, 2, size=n).astype(np.uint16)


def z(rng, n):
    return np.zeros(n, np.uint16)


def stream1(seed):
    rng = np.random.default_rng(seed)
    parts = [mixed(rng, 6000), z(rng, 5000), bits(rng, 6000), mixed(rng, 9000), z(rng, 2500), mixed(rng, 4113)]
    return np.concatenate(parts)          # 32 613 symbols


def stream2(seed):
    rng = np.random.default_rng(seed)
    parts = [mixed(rng, 4096), z(rng, 4096), mixed(rng, 4096), z(rng, 9000), mixed(rng, 3000), z(rng, 1)]
    return np.concatenate(parts)          # 24 289 symbols
