"""Token streams of the first LZ77 stage for the tests of the parallel expander (jampack_amd/csrc/lz_expand.hpp, k_lzx_plan /
k_lzx_copy): a small token writer in the format of Lz77::WriteToken (lz77.cpp:53-70) and the crafted streams both the rule test
(test_lz_expand_rule_host.py) and the device test (test_gpu_lz77_expand.py) run.

A case is (name, stream bytes, out_cap or None, path): out_cap None = exactly what the stream decodes to; path is "parallel" when the
rule decodes the block from its records, "serial" when it must hand it to the serial decoder (a failed check, more records than
in_len / 64 + 4, or a byte more than 8 matches away from its literal).
"""
import struct

import numpy as np

END = bytes([0x04, 0x80])
LEB_OFF = (127, 16510, 2113661, 270549116)
MAX_CHASE = 8


def leb(v: int) -> bytes:
    """Utils::EncodeLeb128 (utils.cpp:22-60) as pre::leb_write has it"""
    if v < LEB_OFF[0]:
        return bytes([v | 0x80])
    for d in range(1, 5):
        if d == 4 or v < LEB_OFF[d]:
            x = v - LEB_OFF[d - 1]
            return bytes([(x >> (7 * (d - k))) & 0x7F for k in range(d)] + [0x80 | (x & 0x7F)])
    raise ValueError(v)


def tok(length: int, lits: bytes, off: int) -> bytes:
    """one token: `lits` literal bytes, then a match of `length` >= 4 bytes at distance off"""
    assert length >= 4
    lc, nl = min(length - 4, 31), min(len(lits), 7)
    b = bytes([(lc << 3) | nl]) + leb(off)
    if lc == 31:
        b += leb(length - 4 - 31)
    if nl == 7:
        b += leb(len(lits) - 7)
    return b + bytes(lits)


def seg_cap(in_len: int) -> int:
    return in_len // 64 + 4


def _rnd(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def chase(depth: int) -> bytes:
    """64 literals, then `depth` matches of 64 bytes at distance 64, each a copy of the one in front of it: a byte of the last match is
    `depth` hops from its literal.  1 KiB of trailing literals keeps the record cap out of the way (depth + 2 records, cap 20 and more)."""
    s = tok(64, _rnd(64, 900 + depth), 64)
    for _ in range(depth - 1):
        s += tok(64, b"", 64)
    return s + END + _rnd(1024, 901)


def records(tokens: int, extra_single: int) -> bytes:
    """`tokens` tokens of one literal and a match of 4 (two records each), `extra_single` tokens of a match alone (one record), the end
    token and 1100 literals (one record): 2 * tokens + extra_single + 1 records"""
    s = b"".join(tok(4, bytes([65 + i % 26]), 1) for i in range(tokens))
    s += b"".join(tok(4, b"", 1) for _ in range(extra_single))
    return s + END + _rnd(1100, 902)


def valid_cases():
    cases = [("empty", END, None, "parallel")]
    for n in (1, 15, 16, 17, 65_537):
        cases.append((f"literals {n}", END + _rnd(n, n), None, "parallel"))
    cases.append(("match off>len", tok(10, _rnd(40, 1), 30) + END + _rnd(9, 2), None, "parallel"))
    cases.append(("match off==len", tok(20, _rnd(40, 3), 20) + END + _rnd(5, 4), None, "parallel"))
    for period in (1, 3, 64, 255):
        cases.append((f"match period {period}", tok(1000, _rnd(300, 10 + period), period) + END + _rnd(33, 5), None, "parallel"))
    # sources that straddle a literal|match border (B reads the last 6 literals of A and its match), match|match and match|literal (C)
    s = tok(12, _rnd(32, 6), 7) + tok(20, b"", 18) + tok(30, _rnd(3, 7), 25) + tok(200, b"", 90) + END + _rnd(600, 8)
    cases.append(("straddling sources", s, None, "parallel"))
    # many short records: every 16-byte output word straddles two or more of them
    s = b"".join(tok(4 + i % 5, _rnd(1 + i % 3, 100 + i), 1 + i % 2) for i in range(12)) + END + _rnd(2000, 9)
    cases.append(("words across records", s, None, "parallel"))
    for depth in (1, 2, MAX_CHASE):
        cases.append((f"chase depth {depth}", chase(depth), None, "parallel"))
    cases.append((f"chase depth {MAX_CHASE + 1}", chase(MAX_CHASE + 1), None, "serial"))
    at_cap, over_cap = records(10, 0), records(10, 1)
    assert 2 * 10 + 1 == seg_cap(len(at_cap)) and 2 * 10 + 2 == seg_cap(len(over_cap)) + 1
    cases.append(("records at the cap", at_cap, None, "parallel"))
    cases.append(("one record over the cap", over_cap, None, "serial"))
    cases.append(("no end token", tok(40, _rnd(100, 11), 50), None, "parallel"))
    return cases


def corrupt_cases():
    """(name, stream, out_cap, "serial"): each fails a check of Lz77::Decompress; `short` streams are valid and one byte over out_cap"""
    body = tok(10, _rnd(40, 12), 30) + END + _rnd(100, 13)
    return [
        ("offset beyond the output", tok(8, _rnd(4, 14), 10) + END, 64, "serial"),
        ("offset beyond the output, late", tok(10, _rnd(40, 15), 30) + tok(8, b"abc", 54) + END, 200, "serial"),
        ("truncated token", tok(10, _rnd(40, 16), 30) + bytes([0xF9]) + leb(3), 4096, "serial"),
        ("truncated leb", tok(10, _rnd(40, 17), 30) + bytes([0x08, 0x01]), 4096, "serial"),
        ("literals beyond the input", bytes([0x0F]) + leb(5) + leb(100) + _rnd(10, 18), 4096, "serial"),
        ("one byte over out_cap, rest behind a match", body, 40 + 10 + 100 - 1, "serial"),
        ("one byte over out_cap, token", tok(10, _rnd(40, 19), 30), 49, "serial"),
        ("one byte over out_cap, rest", END + _rnd(77, 20), 76, "serial"),
    ]


def shape(stream) -> tuple:
    """(records, deepest byte) of a VALID stream by a token walk of its own: what decides its path (records <= seg_cap(len(stream)) and
    depth <= MAX_CHASE: parallel)"""
    s = bytes(stream)

    def rd(pos):
        d, x = 0, 0
        while not s[pos + d] & 0x80:
            x = (x << 7) | s[pos + d]
            d += 1
        x = (x << 7) | (s[pos + d] & 0x7F)
        return x + (LEB_OFF[d - 1] if d else 0), pos + d + 1

    depth, pos, nrec, deepest = np.zeros(0, dtype=np.int32), 0, 0, 0
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
            return nrec + (1 if pos < len(s) else 0), deepest
        ln += 4
        nrec += (1 if lit else 0) + 1
        depth = np.concatenate([depth, np.zeros(lit, dtype=np.int32)])
        pos += lit
        src = depth[len(depth) - off:]
        new = np.resize(src, ln) + 1                                   # the period repeats: byte k reads byte k mod off of the source
        deepest = max(deepest, int(new.max()))
        depth = np.concatenate([depth, new])
    return nrec, deepest


def path_of(stream) -> str:
    nrec, deepest = shape(stream)
    return "parallel" if nrec <= seg_cap(len(stream)) and deepest <= MAX_CHASE else "serial"


def pack(cases) -> bytes:
    """the cases as the rule test's program reads them: count, then per case in_len, out_cap (-1: exact), serial flag, the stream"""
    out = struct.pack("<i", len(cases))
    for _, s, cap, path in cases:
        out += struct.pack("<iii", len(s), -1 if cap is None else cap, 1 if path == "serial" else 0) + s
    return out
