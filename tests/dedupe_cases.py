"""Inputs of the dedupe tests (tests/test_dedupe_host.py, tests/test_gpu_dedupe.py): name -> block, built once per process."""
import functools

import numpy as np

MiB = 1 << 20
XS = (255, 256, 257, 511, 512, 4096, 70_000)
YS = (0, 1, 63, 64, 65, 1000)
LITS = (0, 6, 7, 134, 135, 16_518)            # literal runs in front of a match: the classes of the token's literal extension
SMALL = (0, 1, 63, 64, 255, 256)
PATHOLOGICAL = ("zero", "runs", "repeat4k", "tile300", "tile100")


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def tile(period, n, seed):
    rng = np.random.default_rng(seed)
    return np.tile(_rnd(rng, period), n // period + 1)[:n].copy()


@functools.lru_cache(maxsize=None)
def cases():
    from jampack_amd import corpus
    rng = np.random.default_rng(2024)
    out = {}
    for nx in XS:
        for ny in YS:
            x, y = _rnd(rng, nx), _rnd(rng, ny)
            out[f"xyx/{nx}/{ny}"] = np.concatenate([x, y, x])
    x = _rnd(rng, 4096)
    out["xxxx"] = np.tile(x, 4)
    x, y = _rnd(rng, 3000), _rnd(rng, 777)
    out["ends_at_last_byte"] = np.concatenate([y, x, y, x])            # the second x ends the block
    out["source_at_byte_0"] = np.concatenate([x, y, x, y[:100]])
    a, b = _rnd(rng, 1500), _rnd(rng, 2100)
    out["abab"] = np.concatenate([a, b, a, b])
    x = _rnd(rng, 2_300_000)                                           # match extension 2 300 000 - 35 >= 2 113 661: four bytes
    out["copy_2.2MiB"] = np.concatenate([x, x])
    # b | b | (lit literals) | a-copy ...: the token of every later match has `lit` literals in front of it; lit = 0: two tokens back to back
    a, b = _rnd(rng, 600), _rnd(rng, 700)
    for lit in LITS:
        out[f"lit/{lit}"] = np.concatenate([a, b, b, _rnd(rng, lit), a, _rnd(rng, 50)])
    out["zero"] = corpus.make("zero", MiB, 1)
    out["runs"] = corpus.make("runs", MiB, 7)
    out["repeat4k"] = corpus.make("repeat4k", MiB, 7)
    out["tile300"] = tile(300, MiB, 8)
    out["tile100"] = tile(100, MiB, 9)
    out["text"] = corpus.make("text", 300_000, 11)
    out["random"] = corpus.make("random", 300_000, 12)
    for n in SMALL:
        out[f"n/{n}"] = _rnd(rng, n)
    return out


def tokens(s1):
    """the (literals, match length, offset) tokens of an LZ77 stream in front of its end token, by the format's own rules"""
    C = (127, 16510, 2113661, 270549116)

    def leb(pos):
        d, x = 0, 0
        while not s1[pos + d] & 0x80:
            x = (x << 7) | int(s1[pos + d])
            d += 1
        x = (x << 7) | (int(s1[pos + d]) & 0x7F)
        return x + (C[d - 1] if d else 0), pos + d + 1

    out, pos = [], 0
    while True:
        tok = int(s1[pos])
        off, pos = leb(pos + 1)
        ln, lit = tok >> 3, tok & 7
        if ln == 31:
            e, pos = leb(pos)
            ln += e
        if lit == 7:
            e, pos = leb(pos)
            lit += e
        if off == 0:
            return out
        out.append((lit, ln + 4, off))
        pos += lit
