"""Inputs for the tests of the writer's filter choice (test_filters_encode_host.py, test_gpu_filters_encode.py): sampled and
record-shaped data whose channels a delta filter separates, and mixes of them with data that stays raw."""
import numpy as np

MiB = 1 << 20
FBS = 65_536
ROUND_TRIP_LENS = (0, 1, 2, 31, 32, 33, 65_535, 65_536, 65_537, 131_072, 131_073, 196_613)
REC_WIDTHS = (1, 2, 3, 7, 29, 31, 32)
STORED_KINDS = ("text", "text_wide", "random", "dna", "zero", "geometric", "repeat4k")


def _corpus():
    import jampack_amd
    return jampack_amd.corpus


def stereo16(n: int = MiB) -> np.ndarray:
    """two samples16 streams (seeds 1 and 2) interleaved as 16-bit pairs: a 4-byte frame"""
    c = _corpus()
    a, b = c.samples16(n // 2, 1).view(np.uint16), c.samples16(n // 2, 2).view(np.uint16)
    return np.stack([a, b], axis=1).reshape(-1).view(np.uint8)[:n].copy()


def rgb(n: int = MiB, seed: int = 1) -> np.ndarray:
    """three byte channels, each a random walk with steps -3..3"""
    steps = np.random.default_rng(seed).integers(-3, 4, (n // 3 + 1, 3))
    return (np.cumsum(steps, 0) & 255).astype(np.uint8).reshape(-1)[:n].copy()


def structs12(n: int = MiB, seed: int = 1) -> np.ndarray:
    """12-byte records: a counter, a slowly growing u32, four small bytes"""
    rng = np.random.default_rng(seed)
    k = n // 12 + 1
    rows = np.zeros((k, 12), dtype=np.uint8)
    rows[:, 0:4] = (np.arange(k, dtype=np.int64) + 1000).astype("<u4").view(np.uint8).reshape(k, 4)
    rows[:, 4:8] = np.cumsum(rng.integers(0, 50, k)).astype("<u4").view(np.uint8).reshape(k, 4)
    rows[:, 8:12] = rng.integers(0, 4, (k, 4)).astype(np.uint8)
    return rows.reshape(-1)[:n].copy()


def rec(n: int, w: int, seed: int = 1) -> np.ndarray:
    """records of w bytes, every byte column a random walk with steps -2..2 from a start of its own"""
    rng = np.random.default_rng(seed)
    k = n // w + 1
    start = rng.integers(0, 256, w)
    return ((start + np.cumsum(rng.integers(-2, 3, (k, w)), 0)) & 255).astype(np.uint8).reshape(-1)[:n].copy()


def mixed() -> dict:
    """pieces of different kinds back to back, so that neighbouring 64 KiB pieces choose differently; the odd cuts move the record
    phase against the piece grid, and the last piece of each input is short"""
    c = _corpus()
    return {
        "text|rgb|stereo|random|structs": np.concatenate([c.make("text", FBS, 7), rgb(FBS, 2), stereo16(FBS), c.make("random", FBS, 9), structs12(FBS + 1001, 3)]),
        "rec7|text|rec29|rec32|zero": np.concatenate([rec(FBS + 5, 7, 4), c.make("text", FBS - 5, 8), rec(FBS, 29, 5), rec(FBS, 32, 6), np.zeros(3000, np.uint8)]),
        "samples16|rec3|geometric|rec2": np.concatenate([c.make("samples16", FBS, 3), rec(2 * FBS + 77, 3, 7), c.make("geometric", FBS - 77, 4), rec(40_001, 2, 8)]),
    }


def round_trip_inputs():
    """(name, bytes) at every round-trip length: rec at the widths where len % width != 0 and the top width both run, text, random"""
    c = _corpus()
    for n in ROUND_TRIP_LENS:
        for w in REC_WIDTHS:
            yield f"rec{w}/{n}", rec(n, w, 11 + w)
        yield f"text/{n}", c.make("text", n, 5)
        yield f"random/{n}", c.make("random", n, 6)


def pieces(x: np.ndarray):
    """the 64 KiB pieces of S1 = x: all full but the last"""
    return [x[o: o + FBS] for o in range(0, len(x), FBS)]


def headers(s2: np.ndarray, n: int):
    """(type, width) of every piece of an S2 made of n bytes of S1"""
    return [(int(s2[j * (FBS + 2)]), int(s2[j * (FBS + 2) + 1])) for j in range(-(-n // FBS))]
