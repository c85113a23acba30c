"""Guarded device buffers for the contract tests of the jpk_dev_* entries (test_gpu_stage_contracts.py, test_gpu_primitives.py).

A guarded buffer is one device allocation filled with a sentinel byte.  The payload region [off, off + cap) starts `lead` bytes behind
a 256-byte-aligned ADDRESS (the allocation's own base address is looked at, not assumed), with at least GUARD sentinel bytes in front of
it and behind it: a stray store of a whole tile still lands in the test's own allocation, where `violations` finds it.

The checking itself is plain numpy on a host copy of the whole allocation, so it is tested without a GPU (test_stage_guard_host.py).
"""
import numpy as np

SENT = 0xA5
GUARD = 4096
ALIGN = 256


def payload_offset(base_addr: int, lead: int, guard: int = GUARD, align: int = ALIGN) -> int:
    """offset, inside an allocation that starts at address base_addr, of the first byte that has >= guard bytes in front of it and lies
    `lead` bytes behind an align-aligned address"""
    first = base_addr + guard
    return (first + align - 1) // align * align + lead - base_addr


def alloc_bytes(lead: int, cap: int, guard: int = GUARD, align: int = ALIGN) -> int:
    """bytes to allocate so that payload_offset(...) + cap + guard fits whatever the base address is"""
    return guard + align + lead + cap + guard


def violations(img: np.ndarray, off: int, cap: int, used=None, sent: int = SENT):
    """img: host copy of a whole guarded allocation after a call whose output region was [off, off + cap).  Returns a list of
    (region, index of the first changed byte relative to the region's start, number of changed bytes):
      "front"  [0, off)                    the guard in front of the output
      "spare"  [off + used, off + cap)     capacity the call reported it did not use (only with used is not None)
      "back"   [off + cap, len(img))       the guard behind the output: index 0 is the first byte past out_cap"""
    regions = [("front", 0, off), ("back", off + cap, len(img))]
    if used is not None:
        assert 0 <= used <= cap, (used, cap)
        regions.insert(1, ("spare", off + used, off + cap))
    out = []
    for name, a, b in regions:
        bad = np.flatnonzero(img[a:b] != sent)
        if bad.size:
            out.append((name, int(bad[0]), int(bad.size)))
    return out


def first_diff(a: np.ndarray, b: np.ndarray) -> str:
    n = min(len(a), len(b))
    d = np.flatnonzero(a[:n] != b[:n])
    return f"len {len(a)} vs {len(b)}, {d.size} bytes differ, first at {d[:4].tolist()}"


def bit_range_order(keys: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """the permutation a stable sort on key bits [lo, hi) applies (hi == lo: the identity)"""
    keys = np.asarray(keys, dtype=np.uint64)
    w = hi - lo
    if w == 0:
        return np.arange(len(keys), dtype=np.int64)
    mask = np.uint64((1 << w) - 1)
    return np.argsort((keys >> np.uint64(lo)) & mask, kind="stable")


class Guarded:
    """one guarded device allocation; `ptr` is the payload's device address (an int: what the Context methods take)"""

    def __init__(self, torch, payload, lead: int, cap=None):
        a = np.ascontiguousarray(payload).view(np.uint8).reshape(-1) if payload is not None else np.zeros(0, np.uint8)
        self.cap = len(a) if cap is None else int(cap)
        assert len(a) <= self.cap and 0 <= lead < ALIGN
        self.buf = torch.full((alloc_bytes(lead, self.cap),), SENT, dtype=torch.uint8, device="cuda")
        self.off = payload_offset(self.buf.data_ptr(), lead)
        assert self.off >= GUARD and self.off + self.cap + GUARD <= self.buf.numel()
        self.ptr = self.buf.data_ptr() + self.off
        assert (self.ptr - lead) % ALIGN == 0
        self.before = np.full(self.buf.numel(), SENT, dtype=np.uint8)          # what the allocation holds before the call
        self.before[self.off: self.off + len(a)] = a
        if len(a):
            self.buf[self.off: self.off + len(a)] = torch.from_numpy(a).to("cuda")

    def host(self) -> np.ndarray:
        return self.buf.cpu().numpy()

    def check_output(self, expect, used=None, what=""):
        """(a) the first len(expect) bytes of the region equal expect, (b) both guards hold the sentinel, (c) so do the bytes from `used`
        (default len(expect)) up to the capacity.  Returns the host copy."""
        img = self.host()
        expect = np.ascontiguousarray(expect).view(np.uint8).reshape(-1)
        used = len(expect) if used is None else used
        v = violations(img, self.off, self.cap, used)
        assert not v, f"{what}: wrote outside its output (region, first index, bytes): {v}"
        got = img[self.off: self.off + len(expect)]
        assert np.array_equal(got, expect), f"{what}: {first_diff(got, expect)}"
        return img

    def check_guards(self, what=""):
        """after a call that failed: nothing outside [ptr, ptr + cap) was written"""
        v = violations(self.host(), self.off, self.cap, None)
        assert not v, f"{what}: wrote outside its output (region, first index, bytes): {v}"

    def check_unchanged(self, what=""):
        """(d) a const input: payload and guards are what they were"""
        img = self.host()
        d = np.flatnonzero(img != self.before)
        assert d.size == 0, f"{what}: const input changed, {d.size} bytes, first at payload offset {int(d[0]) - self.off}"
