"""What the host test (test_jam_staged_host.py) and the device test (test_gpu_jam_staged.py) of staged frames share: the inputs of the
one-frame tests, the stored form of S2 and the header fields."""
import struct

import numpy as np

import dedupe_cases
import filter_cases

MiB = 1 << 20
STAGED = 1 << 30
FLAGS = (0, 1, 4, 5)
FBS = 65_536
DEDUPE_NAMES = ("xyx/256/0", "xyx/70000/1000", "xxxx", "abab", "lit/135", "tile300", "text", "n/0", "n/1")


def inputs():
    """name -> raw block: the dedupe's cases (lengths 0 and 1 among them) and blocks the filter choice has something to find in"""
    d = dedupe_cases.cases()
    out = {name: d[name] for name in DEDUPE_NAMES}
    out["stereo16"] = filter_cases.stereo16(200_000)
    out["rec7"] = filter_cases.rec(131_073, 7)
    out["mixed"] = filter_cases.mixed()["text|rgb|stereo|random|structs"]
    assert len(out["n/0"]) == 0 and len(out["n/1"]) == 1
    return out


def s2_stored(r):
    """S2 of flags 0 (DESIGN 4.7 "Writing"): S1 = 04 80 | R, every 64 KiB piece of it behind 00 00"""
    s1 = np.concatenate([np.array([0x04, 0x80], dtype=np.uint8), np.asarray(r, dtype=np.uint8)])
    return np.concatenate([np.concatenate([np.zeros(2, dtype=np.uint8), s1[o: o + FBS]]) for o in range(0, len(s1), FBS)])


def header(f):
    """(magic, crc, payload size, BlockSize field) of the frame at the start of f"""
    return struct.unpack("<3sIii", bytes(f[:15]))
