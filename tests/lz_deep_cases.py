"""Token streams for the tests of the deep LZ77 expander (the deep rule of jampack_amd/csrc/lz_expand.hpp, k_lzd_plan / k_lzd_copy,
jpk_dev_blocks_lz77_expand_deep): the model of the rule and the crafted streams that the rule test (test_lz_deep_rule_host.py), the
device test (test_gpu_lz77_expand_deep.py) and the staged reader's test (test_gpu_jam_staged_deep.py) run.  The token writer is
lz_expand_cases.py's.

limits = (H, bytes_per_record, slack) as jampack_amd.lz77_deep_limits() gives them (32, 128, 4).  A case is (name, stream, out_cap or
None, path) as in lz_expand_cases.py; the path is worked out by deep_path_of, never written down by hand.
"""
import numpy as np

from lz_expand_cases import END, LEB_OFF, shape, tok

LIMITS = (32, 128, 4)               # what the tests expect jpk_debug_lz77_deep_limits to say; the GPU tests read it from the library


def _rnd(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def prefixes(stream):
    """(records, output bytes) behind every token of a VALID stream, the end token included, by a token walk of its own"""
    s = bytes(stream)

    def rd(pos):
        d, x = 0, 0
        while not s[pos + d] & 0x80:
            x = (x << 7) | s[pos + d]
            d += 1
        x = (x << 7) | (s[pos + d] & 0x7F)
        return x + (LEB_OFF[d - 1] if d else 0), pos + d + 1

    out, pos, nrec, op = [], 0, 0, 0
    while pos < len(s):
        t = s[pos]
        off, pos = rd(pos + 1)
        ln, lit = t >> 3, t & 7
        if ln == 31:
            e, pos = rd(pos)
            ln += e
        if lit == 7:
            e, pos = rd(pos)
            lit += e
        if off == 0:
            rest = len(s) - pos
            out.append((nrec + (1 if rest else 0), op + rest))
            break
        nrec += (1 if lit else 0) + 1
        op += lit + ln + 4
        pos += lit
        out.append((nrec, op))
    return out


def deep_path_of(stream, limits=LIMITS) -> str:
    """the model of the deep rule on a VALID stream: serial when behind some token records > op // bytes_per_record + slack, or when a
    byte is more than H matches from its literal"""
    hops, per, slack = limits
    if any(nrec > op // per + slack for nrec, op in prefixes(stream)):
        return "serial"
    return "parallel" if shape(stream)[1] <= hops else "serial"


def deep_chase(d: int) -> bytes:
    """256 literals, then d matches of 256 bytes at distance 256, each a copy of the one in front, then 1 KiB of literals: d hops deep and
    two records per 512 bytes at the worst, inside the budget"""
    s = tok(256, _rnd(256, 700 + d), 256)
    for _ in range(d - 1):
        s += tok(256, b"", 256)
    return s + END + _rnd(1024, 701)


def generations(depth: int) -> bytes:
    """generation 0 is 4 KiB of literals, generation k = 1..depth a match of 4032 bytes at distance 4096 and 64 fresh literals (file B
    copies A, C copies B, ...): a byte of the last generation's match is `depth` hops deep"""
    s, lits = b"", _rnd(4096, 710)
    for k in range(1, depth + 1):
        s += tok(4032, lits, 4096)
        lits = _rnd(64, 710 + k)
    return s + END + lits


def overlaps(period: int, depth: int, length: int = 300) -> bytes:
    """`depth` matches of `length` bytes at a short distance `period`, one behind the other and behind 256 literals: every match repeats
    the last `period` bytes of the one in front of it, a 16-byte word hardly ever stays inside one period, and every byte of match k is
    k hops deep: the per-byte chase at its worst"""
    s = tok(length, _rnd(256, 720 + period), period)
    for _ in range(depth - 1):
        s += tok(length, b"", period)
    return s + END + _rnd(40, 721)


def budget(over: bool) -> bytes:
    """two tokens of one literal and a match of 4: 4 records for 10 bytes, exactly 10 // 128 + 4.  over: a match alone behind them makes it
    5 for 14 bytes.  A long match and 1100 literals bring both streams back far inside the budget, which does not help the second one"""
    s = tok(4, b"A", 1) + tok(4, b"B", 1)
    if over:
        s += tok(4, b"", 1)
    return s + tok(300, b"", 2) + END + _rnd(1100, 730)


def short_input(tokens: int = 390) -> bytes:
    """what a short period makes of a block: 300 literals and `tokens` matches of 300 bytes that all read the literals -- about 4 input
    bytes per token, far more records than in_len / 64 + 4 and one hop deep"""
    s = tok(300, _rnd(300, 740), 300)
    for k in range(1, tokens):
        s += tok(300, b"", 300 * (k + 1))
    return s + END


def record_edge(at: int) -> bytes:
    """a literal record that ends at byte `at` of the output, a match that ends at byte 3 * at + 40 and one more of each"""
    return tok(2 * at + 40, _rnd(at, 750 + at), 5) + tok(at + 13, _rnd(at, 760 + at), 2 * at) + END + _rnd(at, 770 + at)


def short_records() -> bytes:
    """4 KiB of literals pay for 32 records; behind them 12 tokens of one to three literals and a match of 4 to 8 bytes at distance 1 or
    2: every 16-byte word there lies across two or more records"""
    s = tok(8, _rnd(4096, 790), 3)
    s += b"".join(tok(4 + i % 5, _rnd(1 + i % 3, 791 + i), 1 + i % 2) for i in range(12))
    return s + END + _rnd(100, 789)


def tiny(n: int) -> bytes:
    """n bytes of output; from 5 bytes on, one literal and a match"""
    return END + _rnd(n, 780 + n) if n < 5 else tok(n - 1, b"z", 1) + END


def valid_cases(limits=LIMITS):
    from lz_expand_cases import chase
    hops = limits[0]
    named = [(f"deep chase {d}", deep_chase(d)) for d in (9, 15, hops, hops + 1)]
    named += [(f"generations {d}", generations(d)) for d in (9, 15, hops, hops + 1, hops + 2)]
    named += [(f"period {p} depth {hops}", overlaps(p, hops)) for p in (3, 17)]
    named += [("chase 7 of 64 bytes", chase(7)), ("chase 8 of 64 bytes", chase(8))]
    named += [("records at the budget", budget(False)), ("one record over the budget", budget(True))]
    named += [("short input", short_input()), ("short records", short_records())]
    named += [(f"record edge {at}", record_edge(at)) for at in (15, 16, 17)]
    named += [(f"tiny {n}", tiny(n)) for n in (0, 1, 15, 16, 17)]
    return [(name, s, None, deep_path_of(s, limits)) for name, s in named]


def expected_paths(limits=LIMITS):
    """the paths the issue names, for the tests to hold deep_path_of against"""
    hops = limits[0]
    want = {f"deep chase {d}": "parallel" for d in (9, 15, hops)}
    want[f"deep chase {hops + 1}"] = "serial"
    want.update({f"generations {d}": "parallel" for d in (9, 15, hops)})
    want.update({f"generations {d}": "serial" for d in (hops + 1, hops + 2)})
    want.update({f"period {p} depth {hops}": "parallel" for p in (3, 17)})
    want.update({"chase 7 of 64 bytes": "parallel", "chase 8 of 64 bytes": "serial", "records at the budget": "parallel",
                 "one record over the budget": "serial", "short input": "parallel", "short records": "parallel"})
    want.update({f"record edge {at}": "parallel" for at in (15, 16, 17)})
    want.update({f"tiny {n}": "parallel" for n in (0, 1, 15, 16, 17)})
    return want
