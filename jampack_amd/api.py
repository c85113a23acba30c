"""Python mirror of the reference's operator interface for the block hot path, on top of the C ABI.

Reference interface mirrored (same names and argument meaning; errors raise JampackError instead of exit(-1)):
  BlockSort::Bwt::ForwardBwt / InverseBwt   bwt.hpp:13-18
  Ans::Encode / Ans::Decode                 ans.hpp:32-33
  Postcoder::Encode / Decode                rank.hpp:12-13
Host-buffer calls take/return numpy uint8 arrays; `Context` exposes the device-buffer entry points for data that
already lives in HBM (torch CUDA tensors or raw device pointers).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CHUNK, TRAILER, JampackError, Stats, lib


def _np_u8(a) -> np.ndarray:
    return np.ascontiguousarray(np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray, memoryview)) else a, dtype=np.uint8)


def _ptr(a: np.ndarray):
    return a.ctypes.data if a.size else None


def _chk(rc: int, what: str):
    if rc != 0:
        raise JampackError(rc, what)


def ans_capacity(n: int) -> int:
    """generous output bound for Ans::Encode of n bytes (the reference gives 1.05 x BlockSize, jampack.cpp:74)"""
    return int(n * 1.25) + 4096 + 1400 * (n // CHUNK + 1)


def init(device_mask: int = 0) -> int:
    """jpk_init: devices the host-buffer entry points may use (bit d = device d, 0 = all); returns how many were selected"""
    n = lib().jpk_init(device_mask)
    if n < 0:
        raise JampackError(n, "jpk_init")
    return n


def shutdown() -> None:
    lib().jpk_shutdown()


def release_idle() -> int:
    """destroys the batch entries' idle worker contexts and the multi-device slabs; returns the contexts destroyed"""
    return int(lib().jpk_release_idle())


def thread_device() -> int:
    """device the calling thread's pooled context lives on"""
    d = lib().jpk_thread_device()
    if d < 0:
        raise JampackError(d, "jpk_thread_device")
    return d


def ans_decoded_size(stream):
    """(decoded bytes, chunks) declared by the chunk headers of an Ans stream (host-side header walk)"""
    c = _np_u8(stream)
    n, k = C.c_int64(0), C.c_int32(0)
    _chk(lib().jpk_ans_decoded_size(_ptr(c), len(c), C.byref(n), C.byref(k)), "jpk_ans_decoded_size")
    return n.value, k.value


class Bwt:
    """BlockSort::Bwt (bwt.hpp:13-18)."""

    def ForwardBwt(self, block, out: np.ndarray | None = None) -> np.ndarray:
        t = _np_u8(block)
        if out is None:
            out = np.zeros(len(t) + TRAILER, dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_bwt_forward(_ptr(t), len(t), out.ctypes.data, len(out), C.byref(n)), "ForwardBwt")
        return out[: n.value]

    def InverseBwt(self, bwt, threads: int = 1, gpu: bool = True) -> np.ndarray:
        b = _np_u8(bwt)
        out = np.zeros(max(len(b), 1), dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_bwt_inverse(_ptr(b), len(b), out.ctypes.data, len(out), C.byref(n), threads, int(gpu)), "InverseBwt")
        return out[: n.value]


class Ans:
    """Ans (ans.hpp:15-45)."""

    def Encode(self, data, cap: int | None = None) -> np.ndarray:
        x = np.array(_np_u8(data), copy=True)       # the ABI may clobber its input like the reference (rank.cpp:88)
        cap = ans_capacity(len(x)) if cap is None else cap
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_ans_encode(_ptr(x), len(x), out.ctypes.data, cap, C.byref(n)), "Ans::Encode")
        return out[: n.value]

    def Decode(self, data, cap: int, threads: int = 1) -> np.ndarray:
        c = _np_u8(data)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_ans_decode(_ptr(c), len(c), out.ctypes.data, cap, C.byref(n), threads), "Ans::Decode")
        return out[: n.value]


class Postcoder:
    """Postcoder (rank.hpp:9-16)."""

    def Encode(self, t):
        r = np.array(_np_u8(t), copy=True)
        f = np.zeros(256, dtype=np.int32)
        _chk(lib().jpk_rank_encode(_ptr(r), f.ctypes.data, len(r)), "Postcoder::Encode")
        return r, f

    def Decode(self, ranks, freq) -> np.ndarray:
        r = np.array(_np_u8(ranks), copy=True)
        f = np.ascontiguousarray(freq, dtype=np.int32)
        _chk(lib().jpk_rank_decode(_ptr(r), f.ctypes.data, len(r)), "Postcoder::Decode")
        return r


def block_compress(block, cap: int | None = None) -> np.ndarray:
    """ForwardBwt + Ans::Encode (jampack.cpp:40-41) with the BWT image kept in HBM."""
    t = _np_u8(block)
    cap = ans_capacity(len(t) + TRAILER) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_int32(0)
    _chk(lib().jpk_block_compress(_ptr(t), len(t), out.ctypes.data, cap, C.byref(n)), "block_compress")
    return out[: n.value]


def block_decompress(comp, cap: int) -> np.ndarray:
    """Ans::Decode + InverseBwt (jampack.cpp:49-50)."""
    c = _np_u8(comp)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_int32(0)
    _chk(lib().jpk_block_decompress(_ptr(c), len(c), out.ctypes.data, cap, C.byref(n)), "block_decompress")
    return out[: n.value]


JAM_HEADER = 15
MIN_BLOCKSIZE = 1 << 20        # format.hpp:21
MAX_BLOCKSIZE = 1000 << 20     # format.hpp:22


class Checksum:
    """Mirror of `class Checksum` (checksum.hpp:12-16)."""

    def IntegrityCheck(self, buf) -> int:
        t = _np_u8(buf)
        crc = C.c_uint32(0)
        _chk(lib().jpk_checksum(_ptr(t), len(t), C.byref(crc)), "Checksum::IntegrityCheck")
        return crc.value


def jam_block_write(block, block_size: int, cap: int | None = None) -> np.ndarray:
    """One framed block: crc (jampack.cpp:31) + the 15-byte header of CompWriteBlock (jampack.cpp:122-135) +
    the block_compress payload."""
    t = _np_u8(block)
    cap = JAM_HEADER + ans_capacity(len(t) + TRAILER) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_int32(0)
    _chk(lib().jpk_jam_block_write(_ptr(t), len(t), block_size, out.ctypes.data, cap, C.byref(n)), "jam_block_write")
    return out[: n.value]


def jam_block_read(stream, cap: int):
    """DecompReadBlock + Decomp (jampack.cpp:140-164, 47-60) for the frame at the start of `stream`.
    Returns (block bytes, bytes consumed); raises JampackError(CORRUPT) on a bad header or crc."""
    c = _np_u8(stream)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n, used = C.c_int32(0), C.c_int32(0)
    _chk(lib().jpk_jam_block_read(_ptr(c), len(c), out.ctypes.data, cap, C.byref(n), C.byref(used)), "jam_block_read")
    return out[: n.value], used.value


def jam_compress_bound(n: int, block_size: int = 8 << 20) -> int:
    """jpk_jam_compress_bound: the largest archive n input bytes can give with this block size"""
    b = int(lib().jpk_jam_compress_bound(n, block_size))
    _chk(b if b < 0 else 0, "jpk_jam_compress_bound")
    return b


def jam_compress(data, block_size: int = 8 << 20) -> np.ndarray:
    """Jampack::Compress's block loop (jampack.cpp:186-254) over an in-memory buffer: consecutive frames of
    block_size input bytes (DEFAULT_BLOCKSIZE 8 MiB, format.hpp:20), made by one jpk_jam_compress call (the batch engine)."""
    t = _np_u8(data)
    out = np.empty(max(jam_compress_bound(len(t), block_size), 1), dtype=np.uint8)
    n = C.c_int64(0)
    _chk(lib().jpk_jam_compress(_ptr(t), len(t), block_size, out.ctypes.data, len(out), C.byref(n), 0), "jam_compress")
    return out[: n.value]


def jam_frames(stream):
    """jpk_jam_frames: host walk of an archive -> (frames, raw bytes, bad frame or -1) of the frames in front of the first bad one"""
    c = _np_u8(stream)
    k, raw, bad = C.c_int32(0), C.c_int64(0), C.c_int32(-1)
    rc = lib().jpk_jam_frames(_ptr(c), len(c), C.byref(k), C.byref(raw), C.byref(bad))
    if rc not in (0, -3):
        raise JampackError(rc, "jpk_jam_frames")
    return k.value, raw.value, bad.value


def jam_decompress(stream) -> np.ndarray:
    """Jampack::Decompress's block loop (jampack.cpp:262-336): frames until the stream ends, decoded by one jpk_jam_decompress call.
    Raises JampackError(-3) on the first corrupt frame."""
    c = _np_u8(stream)
    k, raw, bad = jam_frames(c)
    if bad >= 0:
        raise JampackError(-3, f"jam_decompress: corrupt frame {bad}")
    out = np.empty(max(raw, 1), dtype=np.uint8)
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
    _chk(lib().jpk_jam_decompress(_ptr(c), len(c), out.ctypes.data, raw, C.byref(n), C.byref(nf), C.byref(bf)), "jam_decompress")
    return out[: n.value]


JAM_INDEX_PLAIN, JAM_INDEX_CLI, JAM_INDEX_STAGED = 0, 1, 2    # JPK_JAM_INDEX_*: the kinds of an index (and, for kind 2, of its frames)
JAM_GAP_NOFRAME, JAM_GAP_STAGE = 0, 1                         # JPK_JAM_GAP_*: why a recovered index skipped archive bytes


class JamIndex:
    """jpk_jam_index: the frame table of one archive -- `frames`, `raw_len`, `archive_len`, `bad_frame` (-1: the whole archive is
    indexed; otherwise the index covers the frames in front of that one), `kind` (0: a plain archive, 1: an archive of the stock CLI,
    indexed by decoding it, 2: an archive of plain and staged frames, a staged frame sized by the token walk of its first stage or by a
    decode), `frame(k)` and `frame_kind(k)`; `gaps`, the archive bytes a recovered index (jam_recover_index) skipped, a list of
    (archive_off, archive_len, frame, why) -- empty for every other index.  Keeps no reference to the archive."""

    def __init__(self, handle, bad_frame: int):
        self._h = handle
        k, raw, alen = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _chk(lib().jpk_jam_index_info(self._h, C.byref(k), C.byref(raw), C.byref(alen)), "jpk_jam_index_info")
        self.frames, self.raw_len, self.archive_len, self.bad_frame = k.value, raw.value, alen.value, int(bad_frame)
        self.kind = int(lib().jpk_jam_index_kind(self._h))
        self.gaps = []
        for g in range(int(lib().jpk_jam_index_gaps(self._h))):
            o, n, f, w = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
            _chk(lib().jpk_jam_index_gap(self._h, g, C.byref(o), C.byref(n), C.byref(f), C.byref(w)), "jpk_jam_index_gap")
            self.gaps.append((o.value, n.value, f.value, w.value))

    def frame(self, k: int):
        """(raw offset, raw size, payload offset, payload size) of frame k"""
        ro, raw, po, ps = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _chk(lib().jpk_jam_index_frame(self._h, k, C.byref(ro), C.byref(raw), C.byref(po), C.byref(ps)), "jpk_jam_index_frame")
        return ro.value, raw.value, po.value, ps.value

    def frame_kind(self, k: int) -> int:
        """jpk_jam_index_frame_kind: 0 (plain) or 2 (staged) for frame k of an index of kind 2, the index's kind otherwise"""
        rc = int(lib().jpk_jam_index_frame_kind(self._h, k))
        _chk(min(rc, 0), "jpk_jam_index_frame_kind")
        return rc

    def close(self):
        if self._h:
            lib().jpk_jam_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def jam_index(stream) -> JamIndex:
    """jpk_jam_index_create: the index of an archive in host memory (no device call)"""
    c = _np_u8(stream)
    h, bad = C.c_void_p(), C.c_int32(-1)
    _chk(lib().jpk_jam_index_create(_ptr(c), len(c), C.byref(h), C.byref(bad)), "jpk_jam_index_create")
    return JamIndex(h, bad.value)


def jam_cli_index(stream) -> JamIndex:
    """jpk_jam_cli_index_create: the index of a stock-CLI archive in host memory, made by decoding it once on the device (a frame's
    raw size is known only behind its last stage); jam_read takes it like a plain index"""
    c = _np_u8(stream)
    h, bad = C.c_void_p(), C.c_int32(-1)
    _chk(lib().jpk_jam_cli_index_create(_ptr(c), len(c), C.byref(h), C.byref(bad)), "jpk_jam_cli_index_create")
    return JamIndex(h, bad.value)


def jam_staged_index(stream, verify: bool = False) -> JamIndex:
    """jpk_jam_staged_index_create: the index (kind 2) of an archive of plain and staged frames in host memory.  A staged frame's raw size
    comes from the token walk of its first stage on the device -- no expansion and no checksum; verify=True decodes and checks every
    staged frame instead.  An archive without a staged frame is indexed on the host alone.  jam_read takes it like a plain index."""
    c = _np_u8(stream)
    h, bad = C.c_void_p(), C.c_int32(-1)
    _chk(lib().jpk_jam_staged_index_create(_ptr(c), len(c), int(verify), C.byref(h), C.byref(bad)), "jpk_jam_staged_index_create")
    return JamIndex(h, bad.value)


def _recover_verify(kind: int, verify) -> int:
    """verify=None is the kind's own value: 1 for a stock-CLI index, whose every frame is decoded, 0 otherwise"""
    return int(kind == JAM_INDEX_CLI) if verify is None else int(verify)


def jam_recover_index(stream, kind: int = JAM_INDEX_PLAIN, verify: bool | None = None) -> JamIndex:
    """jpk_jam_index_recover: the index of a damaged archive in host memory -- the walk goes on behind a bad frame at the next offset
    where a structurally valid frame starts, and what it skipped is in `gaps`.  kind 0: plain frames, no device call; kind 2: plain and
    staged frames, a staged frame sized (verify=True: decoded and checked) on the device, one its stages refuse becomes a gap; kind 1:
    frames of the stock CLI, every structurally valid one decoded and checked on the device (verify must be True), one that fails
    becomes a gap.  verify=None is the kind's own value: True for kind 1, False otherwise."""
    c = _np_u8(stream)
    h, g = C.c_void_p(), C.c_int32(0)
    _chk(lib().jpk_jam_index_recover(_ptr(c), len(c), int(kind), _recover_verify(kind, verify), C.byref(h), C.byref(g)), "jpk_jam_index_recover")
    return JamIndex(h, -1)


def jam_salvage(stream, index: JamIndex | None = None, kind: int = JAM_INDEX_PLAIN):
    """jpk_jam_salvage: everything recoverable of an archive in host memory -> (bytes, frame_status).  Frame k of the index lies at its
    raw offset; a frame that fails its decode or its crc has status -3 and zeros in its place.  Without an index the archive is
    recovered first (jam_recover_index(stream, kind))."""
    c = _np_u8(stream)
    ix = index if index is not None else jam_recover_index(c, kind)
    try:
        out = np.zeros(max(ix.raw_len, 1), dtype=np.uint8)
        st = (C.c_int32 * max(ix.frames, 1))()
        n, failed = C.c_int64(0), C.c_int32(0)
        _chk(lib().jpk_jam_salvage(ix._h, _ptr(c), len(c), out.ctypes.data, ix.raw_len, C.byref(n), st, C.byref(failed)), "jpk_jam_salvage")
        return out[: n.value], list(st)[: ix.frames]
    finally:
        if index is None:
            ix.close()


def _frame_status(index: JamIndex, frame_status):
    """the frame_status argument of the repair entries: NULL, or one int32 per frame of the index"""
    if frame_status is None:
        return None
    if len(frame_status) != index.frames:
        raise ValueError("frame_status needs one entry per frame of the index")
    return (C.c_int32 * max(index.frames, 1))(*[int(s) for s in frame_status])


def jam_repair(stream, index: JamIndex, frame_status=None) -> np.ndarray:
    """jpk_jam_repair: the archive that holds exactly the kept frames of the index -- every frame, or with frame_status (a salvage's) the
    ones whose status is 0 --, headers and payloads copied unchanged, back to back.  Host code; no frame is decoded.  The result of a
    recovered index is an archive every whole-archive decoder reads to its end."""
    c = _np_u8(stream)
    st = _frame_status(index, frame_status)
    out = np.empty(max(len(c), 1), dtype=np.uint8)
    n, k = C.c_int64(0), C.c_int32(0)
    _chk(lib().jpk_jam_repair(index._h, _ptr(c), len(c), st, out.ctypes.data, len(c), C.byref(n), C.byref(k)), "jpk_jam_repair")
    return out[: n.value].copy()


def _writes(writes):
    """the (off, len, src) arrays of the update entries from [(raw offset, bytes), ...]; the numpy sources are returned to keep them alive"""
    srcs = [_np_u8(s) for _, s in writes]
    n = len(srcs)
    L, P = C.c_int64 * max(n, 1), C.c_void_p * max(n, 1)
    return n, L(*[int(o) for o, _ in writes]), L(*[len(s) for s in srcs]), P(*[_ptr(s) for s in srcs]), srcs


def jam_update_bound(index: JamIndex, writes, tail_len: int = 0, block_size: int = 8 << 20) -> int:
    """jpk_jam_update_bound: an output capacity that always suffices for jam_update(…, writes [(raw offset, length or bytes), ...], a tail
    of tail_len bytes); raises JampackError(-1) for writes the update would refuse"""
    n = len(writes)
    L = C.c_int64 * max(n, 1)
    lens = [int(s) if isinstance(s, (int, np.integer)) else len(_np_u8(s)) for _, s in writes]
    b = lib().jpk_jam_update_bound(index._h, n, L(*[int(o) for o, _ in writes]), L(*lens), tail_len, block_size)
    if b < 0:
        raise JampackError(int(b), "jpk_jam_update_bound")
    return int(b)


def jam_update(stream, writes, index: JamIndex | None = None, tail=None, block_size: int = 8 << 20, dedupe: bool = False, filters: bool = False,
               flags: int | None = None):
    """jpk_jam_update: the archive in host memory with the writes [(raw offset, bytes), ...] applied and `tail` appended as new frames of
    block_size -> (archive, JamIndex of it).  Only the frames a write touches are encoded again -- each keeps its raw size, its BlockSize
    and its kind; dedupe / filters (or flags) are those of the stock-CLI and the staged writers --, every other frame is copied as it is.
    Writes must be disjoint and inside the archive's raw bytes.  Without an index the archive is taken for a plain one; a stock-CLI
    archive is updated through the index of jam_cli_index, one with staged frames through that of jam_staged_index.  A partly covered
    frame that fails its decode or its crc raises JampackError(-3)."""
    c = _np_u8(stream)
    ix = index if index is not None else jam_index(c)
    try:
        n, off, ln, ptrs, keep = _writes(writes)
        t = _np_u8(tail) if tail is not None else np.zeros(0, dtype=np.uint8)
        fl = _cli_flags(dedupe, filters) if flags is None else flags
        cap = lib().jpk_jam_update_bound(ix._h, n, off, ln, len(t), block_size)
        _chk(min(int(cap), 0), "jpk_jam_update_bound")
        out = np.empty(max(int(cap), 1), dtype=np.uint8)
        m, h, rw, bad = C.c_int64(0), C.c_void_p(), C.c_int32(0), C.c_int32(-1)
        rc = lib().jpk_jam_update(ix._h, _ptr(c), len(c), n, off, ln, ptrs, _ptr(t), len(t), block_size, fl, 0, out.ctypes.data, int(cap), C.byref(m), C.byref(h),
                                  C.byref(rw), C.byref(bad))
        _chk(rc, f"jpk_jam_update: frame {bad.value}" if bad.value >= 0 else "jpk_jam_update")
        del keep
        return out[: m.value].copy(), JamIndex(h, -1)
    finally:
        if index is None:
            ix.close()


def lz77_size(stream, cap: int) -> int:
    """jpk_lz77_size: what Lz77().Decompress(stream, cap) would be long, from the tokens alone (host code, no output buffer); raises
    JampackError with the status Decompress would raise"""
    t = _np_u8(stream)
    n = C.c_int32(0)
    _chk(lib().jpk_lz77_size(_ptr(t), len(t), cap, C.byref(n)), "jpk_lz77_size")
    return n.value


def lz77_deep_limits():
    """jpk_debug_lz77_deep_limits -> (hop cap H, output bytes per record, records of slack) of the deep expander's rule (host code)"""
    h, b, k = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _chk(lib().jpk_debug_lz77_deep_limits(C.byref(h), C.byref(b), C.byref(k)), "jpk_debug_lz77_deep_limits")
    return h.value, b.value, k.value


def _ranges(ranges):
    n = len(ranges)
    L = C.c_int64 * max(n, 1)
    return n, L(*[int(o) for o, _ in ranges]), L(*[int(l) for _, l in ranges])


def jam_read(stream, ranges, index: JamIndex | None = None):
    """jpk_jam_read: the byte ranges [(raw offset, length), ...] of an archive in host memory -> list of numpy arrays.  Only the frames
    the ranges touch are staged and decoded.  Raises JampackError with the first failing range's status.  Without an index the archive
    is taken for a plain one; a stock-CLI archive is read through the index of jam_cli_index, an archive with staged frames through
    the index of jam_staged_index."""
    c = _np_u8(stream)
    ix = index if index is not None else jam_index(c)
    try:
        n, off, ln = _ranges(ranges)
        outs = [np.empty(max(int(l), 0), dtype=np.uint8) for _, l in ranges]
        P = C.c_void_p * max(n, 1)
        bad = C.c_int32(-1)
        _chk(lib().jpk_jam_read(ix._h, _ptr(c), len(c), n, off, ln, P(*[o.ctypes.data for o in outs]), None, C.byref(bad)), "jpk_jam_read")
        return outs
    finally:
        if index is None:
            ix.close()


class Lz77:
    """Decoder side of `class Lz77` (lz77.hpp:21-22); host code."""

    def Decompress(self, buf, cap: int) -> np.ndarray:
        t = _np_u8(buf)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_lz77_decompress(_ptr(t), len(t), out.ctypes.data, cap, C.byref(n)), "Lz77::Decompress")
        return out[: n.value]

    def dedupe(self, buf, cap: int | None = None) -> np.ndarray:
        """jpk_lz77_dedupe: repeats of >= 256 bytes inside the block as tokens of the first LZ77 stage, the rest as literals (at most
        len + 2 bytes; 04 80 | block when nothing repeats).  Decompress() gives the block back."""
        t = _np_u8(buf)
        cap = len(t) + 2 if cap is None else cap
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_lz77_dedupe(_ptr(t), len(t), out.ctypes.data, cap, C.byref(n)), "jpk_lz77_dedupe")
        return out[: n.value]


class Lpx:
    """`class Lpx` (lpx.hpp:31-32); host code."""

    def Encode(self, buf) -> np.ndarray:
        t = _np_u8(buf)
        out = np.zeros(max(len(t), 1), dtype=np.uint8)
        _chk(lib().jpk_lpx_encode(_ptr(t), len(t), out.ctypes.data), "Lpx::Encode")
        return out[: len(t)]

    encode = Encode

    def Decode(self, buf) -> np.ndarray:
        t = _np_u8(buf)
        out = np.zeros(max(len(t), 1), dtype=np.uint8)
        _chk(lib().jpk_lpx_decode(_ptr(t), len(t), out.ctypes.data), "Lpx::Decode")
        return out[: len(t)]


class Filters:
    """`class Filters` (filters.hpp:43-44); host code.  Encode picks a delta filter per 64 KiB piece by this library's own integer cost
    ("Filters"), not by the reference's heuristic; every decoder of the format reads what it writes."""

    def Encode(self, buf) -> np.ndarray:
        t = _np_u8(buf)
        cap = len(t) + 2 * -(-len(t) // 65_536)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_filters_encode(_ptr(t), len(t), out.ctypes.data, cap, C.byref(n)), "Filters::Encode")
        return out[: n.value]

    encode = Encode

    def Decode(self, buf, cap: int) -> np.ndarray:
        t = _np_u8(buf)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_int32(0)
        _chk(lib().jpk_filters_decode(_ptr(t), len(t), out.ctypes.data, cap, C.byref(n)), "Filters::Decode")
        return out[: n.value]


def filters_cost(piece, type: int, width: int) -> int:
    """jpk_filters_cost: the writer's cost (1/4096 bit) of one filter candidate for one piece of 1..65536 bytes; width 0 = raw"""
    t = _np_u8(piece)
    c = C.c_int64(0)
    _chk(lib().jpk_filters_cost(_ptr(t), len(t), type, width, C.byref(c)), "jpk_filters_cost")
    return c.value


def checksum_host(buf) -> int:
    t = _np_u8(buf)
    return int(lib().jpk_checksum_host(_ptr(t), len(t)))


def jam_cli_block_read(stream, cap: int):
    """One frame written by an unmodified `jampack c`: the whole Jampack::Decomp() (jampack.cpp:47-60), entropy decode and
    inverse BWT on the GPU, the pre-stage decoders on the host.  Returns (block bytes, bytes consumed)."""
    c = _np_u8(stream)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n, used = C.c_int32(0), C.c_int32(0)
    _chk(lib().jpk_jam_cli_block_read(_ptr(c), len(c), out.ctypes.data, cap, C.byref(n), C.byref(used)), "jam_cli_block_read")
    return out[: n.value], used.value


def cli_stages_bound(n: int) -> int:
    """jpk_cli_stages_bound: the bytes the stored-form stage chain makes of an n-byte block (what goes into the BWT)"""
    b = int(lib().jpk_cli_stages_bound(n))
    _chk(b if b < 0 else 0, "jpk_cli_stages_bound")
    return b


CLI_DEDUPE = 1        # JPK_CLI_DEDUPE
CLI_FILTERS = 4       # JPK_CLI_FILTERS (bit 2: the values 2 and 3 stay refused)


def _cli_flags(dedupe: bool, filters: bool) -> int:
    return (CLI_DEDUPE if dedupe else 0) | (CLI_FILTERS if filters else 0)


def cli_stages_encode(block, cap: int | None = None, dedupe: bool = False, filters: bool = False) -> np.ndarray:
    """jpk_cli_stages_encode_ex: end token | Lpx::Encode(raw filter pieces of (end token | block)) -- what the stock decoder's four
    pre-stage decoders turn back into `block`; host code.  dedupe: Lz77().dedupe(block) in place of (end token | block).  filters:
    Filters().Encode in place of the raw pieces."""
    t = _np_u8(block)
    cap = cli_stages_bound(len(t)) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_int32(0)
    _chk(lib().jpk_cli_stages_encode_ex(_ptr(t), len(t), out.ctypes.data, cap, C.byref(n), _cli_flags(dedupe, filters)), "jpk_cli_stages_encode_ex")
    return out[: n.value]


def jam_cli_block_write(block, block_size: int, cap: int | None = None, dedupe: bool = False, filters: bool = False) -> np.ndarray:
    """One frame an unmodified `jampack d` decodes: the header of jam_block_write + block_compress of the stage chain of `block`
    (dedupe: with long repeats taken out first, filters: with a delta filter chosen per 64 KiB piece; cli_stages_encode)."""
    t = _np_u8(block)
    cap = JAM_HEADER + ans_capacity(cli_stages_bound(len(t)) + TRAILER) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_int32(0)
    _chk(lib().jpk_jam_cli_block_write_ex(_ptr(t), len(t), block_size, out.ctypes.data, cap, C.byref(n), _cli_flags(dedupe, filters)), "jam_cli_block_write")
    return out[: n.value]


def jam_cli_compress_bound(n: int, block_size: int = 8 << 20) -> int:
    """jpk_jam_cli_compress_bound: the largest stock-CLI archive n input bytes can give with this block size"""
    b = int(lib().jpk_jam_cli_compress_bound(n, block_size))
    _chk(b if b < 0 else 0, "jpk_jam_cli_compress_bound")
    return b


def jam_cli_compress(data, block_size: int = 8 << 20, dedupe: bool = False, filters: bool = False) -> np.ndarray:
    """The archive an unmodified `jampack d` decodes, made by one jpk_jam_cli_compress_ex call: frames of block_size input bytes, the
    pre-stages written in their stored forms + Lpx::Encode on the GPU, then the batch engine.  dedupe: repeats of >= 256 bytes inside
    a block leave as LZ77 tokens in front of the BWT (the k_dd_* kernels).  filters: every 64 KiB piece goes through the filter choice
    (k_enc_filters in the place of k_enc_wrap)."""
    t = _np_u8(data)
    out = np.empty(max(jam_cli_compress_bound(len(t), block_size), 1), dtype=np.uint8)
    n = C.c_int64(0)
    _chk(lib().jpk_jam_cli_compress_ex(_ptr(t), len(t), block_size, out.ctypes.data, len(out), C.byref(n), 0, _cli_flags(dedupe, filters)), "jam_cli_compress")
    return out[: n.value]


def jam_cli_decompress(stream) -> np.ndarray:
    """`jampack d` over an in-memory .jam stream (Jampack::Decompress's block loop, jampack.cpp:262-336)."""
    c = _np_u8(stream)
    out, o = [], 0
    while o < len(c):
        if len(c) - o < JAM_HEADER:
            raise JampackError(-3, "jam_cli_decompress: truncated header")
        bs = int(np.frombuffer(c[o + 11: o + 15].tobytes(), dtype="<i4")[0])
        if not (MIN_BLOCKSIZE <= bs <= MAX_BLOCKSIZE):
            raise JampackError(-3, "jam_cli_decompress: Refusing to read from corrupt header!")
        blk, used = jam_cli_block_read(c[o:], bs)
        out.append(blk)
        o += used
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


def jam_cli_frames(stream):
    """jpk_jam_cli_frames: host walk of a stock-CLI archive -> (frames, raw bound, bad frame or -1) of the frames in front of the first
    bad one; the raw bound (the sum of their BlockSize) is an output capacity that always suffices"""
    c = _np_u8(stream)
    k, bound, bad = C.c_int32(0), C.c_int64(0), C.c_int32(-1)
    rc = lib().jpk_jam_cli_frames(_ptr(c), len(c), C.byref(k), C.byref(bound), C.byref(bad))
    if rc not in (0, -3):
        raise JampackError(rc, "jpk_jam_cli_frames")
    return k.value, bound.value, bad.value


def jam_cli_decompress_all(stream, check: bool = True):
    """`jampack d` over an in-memory .jam stream of the stock CLI by ONE jpk_jam_cli_decompress call: every frame of a pass through the
    batched entropy decode, inverse BWT and pre-stage decoders on the GPU.  Returns the raw bytes; check=False: (raw bytes in front of
    the first bad frame, frames, bad frame, status), no exception."""
    c = _np_u8(stream)
    _, bound, _ = jam_cli_frames(c)
    out = np.empty(max(bound, 1), dtype=np.uint8)
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
    rc = lib().jpk_jam_cli_decompress(_ptr(c), len(c), out.ctypes.data, bound, C.byref(n), C.byref(nf), C.byref(bf))
    if not check:
        return out[: n.value if rc in (0, -3) else 0], nf.value, bf.value, int(rc)
    _chk(rc, f"jam_cli_decompress_all: frame {bf.value}")
    return out[: n.value]


JAM_STAGED = 1 << 30   # JPK_JAM_STAGED: the bit a staged frame's BlockSize field carries


def jam_staged_block_write(block, block_size: int, cap: int | None = None, dedupe: bool = False, filters: bool = False, flags: int | None = None) -> np.ndarray:
    """jpk_jam_staged_block_write: one staged frame -- the header with JAM_STAGED in the BlockSize field + block_compress of S2, the
    stage chain of cli_stages_encode stopped in front of Lpx::Encode.  flags (an int) overrides dedupe / filters."""
    t = _np_u8(block)
    cap = JAM_HEADER + ans_capacity(cli_stages_bound(len(t)) + TRAILER) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_int32(0)
    fl = _cli_flags(dedupe, filters) if flags is None else flags
    _chk(lib().jpk_jam_staged_block_write(_ptr(t), len(t), block_size, out.ctypes.data, cap, C.byref(n), fl), "jam_staged_block_write")
    return out[: n.value]


def jam_staged_block_read(stream, cap: int):
    """jpk_jam_staged_block_read: one staged frame -> (block bytes, bytes consumed); entropy decode and inverse BWT on the GPU,
    Filters::Decode and Lz77::Decompress on the host"""
    c = _np_u8(stream)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n, used = C.c_int32(0), C.c_int32(0)
    _chk(lib().jpk_jam_staged_block_read(_ptr(c), len(c), out.ctypes.data, cap, C.byref(n), C.byref(used)), "jam_staged_block_read")
    return out[: n.value], used.value


def jam_staged_compress_bound(n: int, block_size: int = 8 << 20) -> int:
    """jpk_jam_staged_compress_bound: the largest archive of staged frames n input bytes can give with this block size"""
    b = int(lib().jpk_jam_staged_compress_bound(n, block_size))
    _chk(b if b < 0 else 0, "jpk_jam_staged_compress_bound")
    return b


def jam_staged_compress(data, block_size: int = 8 << 20, dedupe: bool = False, filters: bool = False, flags: int | None = None) -> np.ndarray:
    """An archive of staged frames by one jpk_jam_staged_compress call: the dedupe and the filter choice (or their stored forms) in
    front of the BWT on the GPU, no LPX.  This library's decoders read it; an unmodified `jampack d` refuses its headers."""
    t = _np_u8(data)
    out = np.empty(max(jam_staged_compress_bound(len(t), block_size), 1), dtype=np.uint8)
    n = C.c_int64(0)
    fl = _cli_flags(dedupe, filters) if flags is None else flags
    _chk(lib().jpk_jam_staged_compress(_ptr(t), len(t), block_size, out.ctypes.data, len(out), C.byref(n), 0, fl), "jam_staged_compress")
    return out[: n.value]


def jam_staged_frames(stream):
    """jpk_jam_staged_frames: host walk of an archive of plain and staged frames -> (frames, raw bound, bad frame or -1); the raw bound
    counts a plain frame at its raw size and a staged one at its BlockSize"""
    c = _np_u8(stream)
    k, bound, bad = C.c_int32(0), C.c_int64(0), C.c_int32(-1)
    rc = lib().jpk_jam_staged_frames(_ptr(c), len(c), C.byref(k), C.byref(bound), C.byref(bad))
    if rc not in (0, -3):
        raise JampackError(rc, "jpk_jam_staged_frames")
    return k.value, bound.value, bad.value


def jam_staged_decompress(stream, check: bool = True):
    """An archive of plain and staged frames by ONE jpk_jam_staged_decompress call.  Returns the raw bytes; check=False: (raw bytes in
    front of the first bad frame, frames, bad frame, status), no exception."""
    c = _np_u8(stream)
    _, bound, _ = jam_staged_frames(c)
    out = np.empty(max(bound, 1), dtype=np.uint8)
    n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
    rc = lib().jpk_jam_staged_decompress(_ptr(c), len(c), out.ctypes.data, bound, C.byref(n), C.byref(nf), C.byref(bf))
    if not check:
        return out[: n.value if rc in (0, -3) else 0], nf.value, bf.value, int(rc)
    _chk(rc, f"jam_staged_decompress: frame {bf.value}")
    return out[: n.value]


def _dptr(x):
    """device pointer of a torch CUDA tensor or a raw int"""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr() if x.numel() else None


class Context:
    """jpk_ctx: one HBM arena + stream per context.  `stream` is a raw hipStream_t (e.g.
    torch.cuda.current_stream().cuda_stream) or None for a private stream."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        _chk(lib().jpk_ctx_create(C.byref(self._h), device, stream), "jpk_ctx_create")

    def close(self):
        if self._h:
            lib().jpk_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, max_block_bytes: int):
        _chk(lib().jpk_ctx_reserve(self._h, max_block_bytes), "jpk_ctx_reserve")

    def stats(self) -> Stats:
        s = Stats()
        _chk(lib().jpk_ctx_stats(self._h, C.byref(s)), "jpk_ctx_stats")
        return s

    def profile_enable(self, mode: int = 2):
        """per-kernel HIP-event timing on the context's stream: 1 = on, 2 = on + reset, 0 = off + reset"""
        _chk(lib().jpk_ctx_profile(self._h, mode), "jpk_ctx_profile")

    def profile_table(self):
        """[{name, ms, launches, units}] for every timed kernel class with at least one launch"""
        out = []
        for i in range(lib().jpk_ctx_profile_count()):
            ms, ln, un = C.c_double(0), C.c_int64(0), C.c_int64(0)
            _chk(lib().jpk_ctx_profile_get(self._h, i, C.byref(ms), C.byref(ln), C.byref(un)), "jpk_ctx_profile_get")
            if ln.value:
                out.append({"id": i, "name": lib().jpk_ctx_profile_name(i).decode(), "ms": ms.value, "launches": ln.value, "units": un.value})
        return out

    def _io(self, fn, what, d_in, in_len, d_out, out_cap) -> int:
        n = C.c_int32(0)
        _chk(fn(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n)), what)
        return n.value

    def bwt_forward(self, d_in, in_len, d_out, out_cap) -> int:
        return self._io(lib().jpk_dev_bwt_forward, "jpk_dev_bwt_forward", d_in, in_len, d_out, out_cap)

    def bwt_inverse(self, d_in, in_len, d_out, out_cap) -> int:
        return self._io(lib().jpk_dev_bwt_inverse, "jpk_dev_bwt_inverse", d_in, in_len, d_out, out_cap)

    def bwt_inverse_chains120(self, d_in, in_len, d_out, out_cap):
        """the reference's 120-chain chase (comparator); returns (bytes, chase kernel ms)"""
        n, ms = C.c_int32(0), C.c_float(0)
        _chk(lib().jpk_dev_bwt_inverse_chains120(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), C.byref(ms)), "jpk_dev_bwt_inverse_chains120")
        return n.value, ms.value

    def ans_encode(self, d_in, in_len, d_out, out_cap) -> int:
        return self._io(lib().jpk_dev_ans_encode, "jpk_dev_ans_encode", d_in, in_len, d_out, out_cap)

    def ans_decode(self, d_in, in_len, d_out, out_cap) -> int:
        return self._io(lib().jpk_dev_ans_decode, "jpk_dev_ans_decode", d_in, in_len, d_out, out_cap)

    def block_compress(self, d_in, in_len, d_out, out_cap) -> int:
        return self._io(lib().jpk_dev_block_compress, "jpk_dev_block_compress", d_in, in_len, d_out, out_cap)

    def block_decompress(self, d_in, in_len, d_out, out_cap) -> int:
        return self._io(lib().jpk_dev_block_decompress, "jpk_dev_block_decompress", d_in, in_len, d_out, out_cap)

    def _batch(self, fn, what, d_ins, in_lens, d_outs, out_caps):
        """(out_len list, status list) of a jpk_dev_blocks_* call: one pass over all blocks"""
        n = len(d_ins)
        P, I = C.c_void_p * n, C.c_int32 * n
        ins, outs = P(*[_dptr(x) for x in d_ins]), P(*[_dptr(x) for x in d_outs])
        il, oc, ol, st = I(*in_lens), I(*out_caps), I(), I()
        _chk(fn(self._h, n, ins, il, outs, oc, ol, st), what)
        return list(ol), list(st)

    def blocks_ans_decode(self, d_ins, in_lens, d_outs, out_caps):
        return self._batch(lib().jpk_dev_blocks_ans_decode, "jpk_dev_blocks_ans_decode", d_ins, in_lens, d_outs, out_caps)

    def blocks_decompress(self, d_ins, in_lens, d_outs, out_caps):
        return self._batch(lib().jpk_dev_blocks_decompress, "jpk_dev_blocks_decompress", d_ins, in_lens, d_outs, out_caps)

    def blocks_compress(self, d_ins, in_lens, d_outs, out_caps, in_flight: int = 0):
        """ForwardBwt + Ans::Encode of independent blocks in one call; the library keeps `in_flight` (0: 4) of them in flight on
        contexts of its own (jampack.cpp:205-224's OpenMP block loop).  Returns (out_len list, status list)."""
        n = len(d_ins)
        P, I = C.c_void_p * n, C.c_int32 * n
        ins, outs = P(*[_dptr(x) for x in d_ins]), P(*[_dptr(x) for x in d_outs])
        il, oc, ol, st = I(*in_lens), I(*out_caps), I(), I()
        _chk(lib().jpk_dev_blocks_compress(self._h, n, ins, il, outs, oc, ol, st, int(in_flight)), "jpk_dev_blocks_compress")
        return list(ol), list(st)

    def blocks_lz77_decompress(self, d_ins, in_lens, d_outs, out_caps):
        """jpk_dev_blocks_lz77_decompress: Lz77::Decompress of independent blocks in one launch -> (out_len list, status list)"""
        return self._batch(lib().jpk_dev_blocks_lz77_decompress, "jpk_dev_blocks_lz77_decompress", d_ins, in_lens, d_outs, out_caps)

    def blocks_lz77_expand(self, d_ins, in_lens, d_outs, out_caps):
        """jpk_dev_blocks_lz77_expand: the same stage through the parallel expander (two launches, the serial kernel for the blocks
        they leave to it) -> (out_len list, status list); lz77_expand_last() says which way the blocks went"""
        return self._batch(lib().jpk_dev_blocks_lz77_expand, "jpk_dev_blocks_lz77_expand", d_ins, in_lens, d_outs, out_caps)

    def blocks_lz77_sizes(self, d_ins, in_lens, out_caps):
        """jpk_dev_blocks_lz77_sizes: the out_len and status lists of blocks_lz77_decompress from the tokens alone, one launch, no
        output buffers -> (out_len list, status list)"""
        n = len(d_ins)
        P, I = C.c_void_p * n, C.c_int32 * n
        ol, st = I(), I()
        _chk(lib().jpk_dev_blocks_lz77_sizes(self._h, n, P(*[_dptr(x) for x in d_ins]), I(*in_lens), I(*out_caps), ol, st), "jpk_dev_blocks_lz77_sizes")
        return list(ol), list(st)

    def lz77_expand_last(self):
        """jpk_debug_lz77_expand_last -> (blocks of the last blocks_lz77_expand call on the parallel path, on the serial path)"""
        p, q = C.c_int32(0), C.c_int32(0)
        _chk(lib().jpk_debug_lz77_expand_last(self._h, C.byref(p), C.byref(q)), "jpk_debug_lz77_expand_last")
        return p.value, q.value

    def blocks_lz77_expand_deep(self, d_ins, in_lens, d_outs, out_caps):
        """jpk_dev_blocks_lz77_expand_deep: the same stage through the deep expander (record budget in output bytes, lz77_deep_limits()
        hops; the serial kernel for the blocks left to it) -> (out_len list, status list); lz77_deep_last() says which way they went"""
        return self._batch(lib().jpk_dev_blocks_lz77_expand_deep, "jpk_dev_blocks_lz77_expand_deep", d_ins, in_lens, d_outs, out_caps)

    def lz77_deep_last(self):
        """jpk_debug_lz77_deep_last -> (blocks of the last deep call on this context -- blocks_lz77_expand_deep or a staged pass -- on
        the parallel path, on the serial path)"""
        p, q = C.c_int32(0), C.c_int32(0)
        _chk(lib().jpk_debug_lz77_deep_last(self._h, C.byref(p), C.byref(q)), "jpk_debug_lz77_deep_last")
        return p.value, q.value

    def blocks_lpx_decode(self, d_ins, lens, d_outs):
        """jpk_dev_blocks_lpx_decode: Lpx::Decode of independent blocks in one launch (output length = input length) -> status list"""
        n = len(d_ins)
        P, I = C.c_void_p * max(n, 1), C.c_int32 * max(n, 1)
        st = I()
        _chk(lib().jpk_dev_blocks_lpx_decode(self._h, n, P(*[_dptr(x) for x in d_ins]), I(*lens), P(*[_dptr(x) for x in d_outs]), st), "jpk_dev_blocks_lpx_decode")
        return list(st)[:n]

    def blocks_lpx_encode(self, d_ins, lens, d_outs):
        """jpk_dev_blocks_lpx_encode: Lpx::Encode of independent blocks in one launch (output length = input length) -> status list"""
        n = len(d_ins)
        P, I = C.c_void_p * max(n, 1), C.c_int32 * max(n, 1)
        st = I()
        _chk(lib().jpk_dev_blocks_lpx_encode(self._h, n, P(*[_dptr(x) for x in d_ins]), I(*lens), P(*[_dptr(x) for x in d_outs]), st), "jpk_dev_blocks_lpx_encode")
        return list(st)[:n]

    def blocks_cli_stages_encode(self, d_ins, in_lens, d_outs, out_caps, dedupe: bool = False, filters: bool = False):
        """jpk_dev_blocks_cli_stages_encode_ex: the stage chain of independent blocks (two launches; dedupe: the k_dd_* launches and one
        host read of the lengths in front of them; filters: k_enc_filters as the first of the two) -> (out_len list, status list)"""
        fl = _cli_flags(dedupe, filters)
        fn = lib().jpk_dev_blocks_cli_stages_encode_ex
        return self._batch(lambda *a: fn(*a, fl), "jpk_dev_blocks_cli_stages_encode_ex", d_ins, in_lens, d_outs, out_caps)

    def blocks_lz77_dedupe(self, d_ins, in_lens, d_outs, out_caps):
        """jpk_dev_blocks_lz77_dedupe: Lz77().dedupe of independent blocks -> (out_len list, status list)"""
        return self._batch(lib().jpk_dev_blocks_lz77_dedupe, "jpk_dev_blocks_lz77_dedupe", d_ins, in_lens, d_outs, out_caps)

    def blocks_filters_encode(self, d_ins, in_lens, d_outs, out_caps):
        """jpk_dev_blocks_filters_encode: Filters().Encode of independent blocks in one launch -> (out_len list, status list)"""
        return self._batch(lib().jpk_dev_blocks_filters_encode, "jpk_dev_blocks_filters_encode", d_ins, in_lens, d_outs, out_caps)

    def blocks_filters_decode(self, d_ins, in_lens, d_outs, out_caps):
        """jpk_dev_blocks_filters_decode: Filters::Decode of independent blocks in one launch -> (out_len list, status list)"""
        return self._batch(lib().jpk_dev_blocks_filters_decode, "jpk_dev_blocks_filters_decode", d_ins, in_lens, d_outs, out_caps)

    def jam_cli_decompress(self, d_in, in_len, d_out, out_cap, check: bool = True):
        """jpk_dev_jam_cli_decompress: a whole stock-CLI archive in HBM -> (raw bytes, frames, bad frame); check=False: (raw bytes,
        frames, bad frame, status), no exception (out_len is the raw bound on JPK_E_CAPACITY, the verified bytes in front of the bad
        frame on JPK_E_CORRUPT)"""
        n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
        rc = lib().jpk_dev_jam_cli_decompress(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), C.byref(nf), C.byref(bf))
        if not check:
            return n.value, nf.value, bf.value, int(rc)
        _chk(rc, "jpk_dev_jam_cli_decompress")
        return n.value, nf.value, bf.value

    def jam_cli_decompress_ix(self, d_in, in_len, d_out, out_cap, check: bool = True):
        """jpk_dev_jam_cli_decompress_ix: jam_cli_decompress that also returns the index of the frames it delivered ->
        (raw bytes, frames, bad frame, JamIndex); check=False: (raw bytes, frames, bad frame, status, JamIndex or None), no exception
        (no index on JPK_E_CAPACITY)"""
        n, nf, bf, h = C.c_int64(0), C.c_int32(0), C.c_int32(-1), C.c_void_p()
        rc = lib().jpk_dev_jam_cli_decompress_ix(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), C.byref(nf), C.byref(bf), C.byref(h))
        ix = JamIndex(h, bf.value) if h else None
        if not check:
            return n.value, nf.value, bf.value, int(rc), ix
        _chk(rc, "jpk_dev_jam_cli_decompress_ix")
        return n.value, nf.value, bf.value, ix

    def checksum(self, d_in, in_len) -> int:
        crc = C.c_uint32(0)
        _chk(lib().jpk_dev_checksum(self._h, _dptr(d_in), in_len, C.byref(crc)), "jpk_dev_checksum")
        return crc.value

    def jam_block_write(self, d_in, in_len, block_size, d_out, out_cap) -> int:
        n = C.c_int32(0)
        _chk(lib().jpk_dev_jam_block_write(self._h, _dptr(d_in), in_len, block_size, _dptr(d_out), out_cap, C.byref(n)), "jpk_dev_jam_block_write")
        return n.value

    def jam_block_read(self, d_in, in_len, d_out, out_cap):
        n, used = C.c_int32(0), C.c_int32(0)
        _chk(lib().jpk_dev_jam_block_read(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), C.byref(used)), "jpk_dev_jam_block_read")
        return n.value, used.value

    def checksums(self, d_ins, in_lens):
        """jpk_dev_checksums: Checksum::IntegrityCheck of device segments in one launch pair -> list of crcs"""
        n = len(d_ins)
        P, I = C.c_void_p * max(n, 1), C.c_int32 * max(n, 1)
        crc = (C.c_uint32 * max(n, 1))()
        _chk(lib().jpk_dev_checksums(self._h, n, P(*[_dptr(x) for x in d_ins]), I(*in_lens), crc), "jpk_dev_checksums")
        return list(crc)[:n]

    def jam_compress(self, d_in, in_len, block_size, d_out, out_cap, in_flight: int = 0) -> int:
        """jpk_dev_jam_compress: the whole archive of d_in[0..in_len) into d_out; returns its length"""
        n = C.c_int64(0)
        _chk(lib().jpk_dev_jam_compress(self._h, _dptr(d_in), in_len, block_size, _dptr(d_out), out_cap, C.byref(n), in_flight), "jpk_dev_jam_compress")
        return n.value

    def jam_cli_compress(self, d_in, in_len, block_size, d_out, out_cap, in_flight: int = 0, dedupe: bool = False, filters: bool = False) -> int:
        """jpk_dev_jam_cli_compress_ex: the archive of d_in[0..in_len) an unmodified `jampack d` decodes, into d_out; returns its length"""
        n = C.c_int64(0)
        _chk(lib().jpk_dev_jam_cli_compress_ex(self._h, _dptr(d_in), in_len, block_size, _dptr(d_out), out_cap, C.byref(n), in_flight,
                                               _cli_flags(dedupe, filters)), "jpk_dev_jam_cli_compress_ex")
        return n.value

    def jam_staged_compress(self, d_in, in_len, block_size, d_out, out_cap, in_flight: int = 0, dedupe: bool = False, filters: bool = False,
                            flags: int | None = None) -> int:
        """jpk_dev_jam_staged_compress: the archive of staged frames of d_in[0..in_len) into d_out; returns its length"""
        n = C.c_int64(0)
        fl = _cli_flags(dedupe, filters) if flags is None else flags
        _chk(lib().jpk_dev_jam_staged_compress(self._h, _dptr(d_in), in_len, block_size, _dptr(d_out), out_cap, C.byref(n), in_flight, fl),
             "jpk_dev_jam_staged_compress")
        return n.value

    def jam_staged_decompress(self, d_in, in_len, d_out, out_cap, check: bool = True):
        """jpk_dev_jam_staged_decompress: an archive of plain and staged frames in HBM -> (raw bytes, frames, bad frame); check=False:
        (raw bytes, frames, bad frame, status), no exception (out_len is the raw bound on JPK_E_CAPACITY, the verified bytes in front
        of the bad frame on JPK_E_CORRUPT)"""
        n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
        rc = lib().jpk_dev_jam_staged_decompress(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), C.byref(nf), C.byref(bf))
        if not check:
            return n.value, nf.value, bf.value, int(rc)
        _chk(rc, "jpk_dev_jam_staged_decompress")
        return n.value, nf.value, bf.value

    def jam_staged_decompress_ix(self, d_in, in_len, d_out, out_cap, check: bool = True):
        """jpk_dev_jam_staged_decompress_ix: jam_staged_decompress that also returns the index (kind 2) of the frames it delivered ->
        (raw bytes, frames, bad frame, JamIndex); check=False: (raw bytes, frames, bad frame, status, JamIndex or None), no exception
        (no index on JPK_E_CAPACITY)"""
        n, nf, bf, h = C.c_int64(0), C.c_int32(0), C.c_int32(-1), C.c_void_p()
        rc = lib().jpk_dev_jam_staged_decompress_ix(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), C.byref(nf), C.byref(bf), C.byref(h))
        ix = JamIndex(h, bf.value) if h else None
        if not check:
            return n.value, nf.value, bf.value, int(rc), ix
        _chk(rc, "jpk_dev_jam_staged_decompress_ix")
        return n.value, nf.value, bf.value, ix

    def jam_decompress(self, d_in, in_len, d_out, out_cap, check: bool = True):
        """jpk_dev_jam_decompress ->(raw bytes, frames, bad frame); check=False: (raw bytes, frames, bad frame, status), no exception
        (out_len is the bytes needed on JPK_E_CAPACITY, the verified bytes in front of the bad frame on JPK_E_CORRUPT)"""
        n, nf, bf = C.c_int64(0), C.c_int32(0), C.c_int32(-1)
        rc = lib().jpk_dev_jam_decompress(self._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), C.byref(nf), C.byref(bf))
        if not check:
            return n.value, nf.value, bf.value, int(rc)
        _chk(rc, "jpk_dev_jam_decompress")
        return n.value, nf.value, bf.value

    def jam_index(self, d_in, in_len) -> JamIndex:
        """jpk_dev_jam_index_create: the index of an archive in HBM"""
        h, bad = C.c_void_p(), C.c_int32(-1)
        _chk(lib().jpk_dev_jam_index_create(self._h, _dptr(d_in), in_len, C.byref(h), C.byref(bad)), "jpk_dev_jam_index_create")
        return JamIndex(h, bad.value)

    def jam_cli_index(self, d_in, in_len) -> JamIndex:
        """jpk_dev_jam_cli_index_create: the index of a stock-CLI archive in HBM, made by decoding it once (no output buffer)"""
        h, bad = C.c_void_p(), C.c_int32(-1)
        _chk(lib().jpk_dev_jam_cli_index_create(self._h, _dptr(d_in), in_len, C.byref(h), C.byref(bad)), "jpk_dev_jam_cli_index_create")
        return JamIndex(h, bad.value)

    def jam_staged_index(self, d_in, in_len, verify: bool = False) -> JamIndex:
        """jpk_dev_jam_staged_index_create: the index (kind 2) of an archive of plain and staged frames in HBM; a staged frame's raw size
        from the token walk of its first stage (no expansion, no checksum), or with verify=True from a decode that checks its crc"""
        h, bad = C.c_void_p(), C.c_int32(-1)
        _chk(lib().jpk_dev_jam_staged_index_create(self._h, _dptr(d_in), in_len, int(verify), C.byref(h), C.byref(bad)), "jpk_dev_jam_staged_index_create")
        return JamIndex(h, bad.value)

    def jam_recover_index(self, d_in, in_len, kind: int = JAM_INDEX_PLAIN, verify: bool | None = None) -> JamIndex:
        """jpk_dev_jam_index_recover: the index of a damaged archive in HBM, past its damage (see jam_recover_index); where the frame walk
        stops, k_jam_scan_* look for the next frame.  kind 1 (frames of the stock CLI): every structurally valid frame goes through the
        stage chain and its crc, and one that fails is a gap.  verify=None is the kind's own value: True for kind 1, False otherwise."""
        h, g = C.c_void_p(), C.c_int32(0)
        _chk(lib().jpk_dev_jam_index_recover(self._h, _dptr(d_in), in_len, int(kind), _recover_verify(kind, verify), C.byref(h), C.byref(g)),
             "jpk_dev_jam_index_recover")
        return JamIndex(h, -1)

    def jam_repair(self, index: JamIndex, d_in, in_len, d_out, out_cap, frame_status=None):
        """jpk_dev_jam_repair: the kept frames of the index (every one, or with frame_status the ones whose status is 0), headers and
        payloads unchanged, back to back in d_out -> (out_len, frames).  One gather launch, no decode.  Raises JampackError(-2) when
        out_cap is too small (nothing is written)."""
        n, k = C.c_int64(0), C.c_int32(0)
        _chk(lib().jpk_dev_jam_repair(self._h, index._h, _dptr(d_in), in_len, _frame_status(index, frame_status), _dptr(d_out), out_cap, C.byref(n), C.byref(k)),
             "jpk_dev_jam_repair")
        return n.value, k.value

    def jam_update(self, index: JamIndex, d_in, in_len, writes, d_out, out_cap, d_tail=None, tail_len: int = 0, block_size: int = 8 << 20, dedupe: bool = False,
                   filters: bool = False, flags: int | None = None, in_flight: int = 0, check: bool = True):
        """jpk_dev_jam_update: the archive d_in[0..in_len) with the writes [(raw offset, length, device source), ...] applied and the tail
        appended, into d_out -> (out_len, JamIndex of the output, rewritten frames); check=False: (out_len, JamIndex or None, rewritten,
        bad frame, status), no exception (out_len is jpk_jam_update_bound's answer on JPK_E_CAPACITY)"""
        n = len(writes)
        L, P = C.c_int64 * max(n, 1), C.c_void_p * max(n, 1)
        off, ln, src = L(*[int(w[0]) for w in writes]), L(*[int(w[1]) for w in writes]), P(*[_dptr(w[2]) for w in writes])
        fl = _cli_flags(dedupe, filters) if flags is None else flags
        m, h, rw, bad = C.c_int64(0), C.c_void_p(), C.c_int32(0), C.c_int32(-1)
        rc = lib().jpk_dev_jam_update(self._h, index._h, _dptr(d_in), in_len, n, off, ln, src, _dptr(d_tail), tail_len, block_size, fl, in_flight, _dptr(d_out), out_cap,
                                      C.byref(m), C.byref(h), C.byref(rw), C.byref(bad))
        ix = JamIndex(h, -1) if h else None
        if not check:
            return m.value, ix, rw.value, bad.value, int(rc)
        _chk(rc, f"jpk_dev_jam_update: frame {bad.value}" if bad.value >= 0 else "jpk_dev_jam_update")
        return m.value, ix, rw.value

    def jam_salvage(self, index: JamIndex, d_in, in_len, d_out, out_cap):
        """jpk_dev_jam_salvage: every frame of the index into d_out at its raw offset -> (raw_len, frame_status); a failed frame has
        status -3 and zeros in its place.  Raises JampackError(-2) when out_cap is below the index's raw_len (nothing is written)."""
        st = (C.c_int32 * max(index.frames, 1))()
        n, failed = C.c_int64(0), C.c_int32(0)
        _chk(lib().jpk_dev_jam_salvage(self._h, index._h, _dptr(d_in), in_len, _dptr(d_out), out_cap, C.byref(n), st, C.byref(failed)), "jpk_dev_jam_salvage")
        return n.value, list(st)[: index.frames]

    def jam_scan(self, d_in, in_len, start: int, window: int, staged_ok: bool = False, max_cands: int = 4096):
        """jpk_debug_jam_scan (probe): the offsets of the first max_cands plausible frame headers that start in [start, start + window)"""
        offs, n = (C.c_int64 * max_cands)(), C.c_int32(0)
        _chk(lib().jpk_debug_jam_scan(self._h, _dptr(d_in), in_len, start, window, int(staged_ok), max_cands, offs, C.byref(n)), "jpk_debug_jam_scan")
        return list(offs)[: n.value]

    def jam_read(self, index: JamIndex, d_in, in_len, ranges, d_outs, check: bool = True):
        """jpk_dev_jam_read: the ranges [(raw offset, length), ...] of the archive d_in[0..in_len) into the device buffers d_outs
        -> (status list, bad frame or -1).  check=True raises JampackError with the first failing range's status."""
        n, off, ln = _ranges(ranges)
        P = C.c_void_p * max(n, 1)
        st, bad = (C.c_int32 * max(n, 1))(), C.c_int32(-1)
        _chk(lib().jpk_dev_jam_read(self._h, index._h, _dptr(d_in), in_len, n, off, ln, P(*[_dptr(x) for x in d_outs]), st, C.byref(bad)), "jpk_dev_jam_read")
        status = list(st)[:n]
        if check:
            for r, s in enumerate(status):
                if s != 0:
                    raise JampackError(s, f"jpk_dev_jam_read: range {r} (frame {bad.value})")
        return status, bad.value

    def rank_encode(self, d_t, d_freq, n):
        _chk(lib().jpk_dev_rank_encode(self._h, _dptr(d_t), _dptr(d_freq), n), "jpk_dev_rank_encode")

    def rank_decode(self, d_r, d_freq, n):
        _chk(lib().jpk_dev_rank_decode(self._h, _dptr(d_r), _dptr(d_freq), n), "jpk_dev_rank_decode")

    def suffix_array(self, d_t, n, d_sa):
        _chk(lib().jpk_dev_suffix_array(self._h, _dptr(d_t), n, _dptr(d_sa)), "jpk_dev_suffix_array")

    def sort_pairs_u64(self, d_keys, d_vals, n, bit_lo=0, bit_hi=64):
        _chk(lib().jpk_dev_sort_pairs_u64(self._h, _dptr(d_keys), _dptr(d_vals), n, bit_lo, bit_hi), "jpk_dev_sort_pairs_u64")

    def exclusive_scan_u32(self, d_data, n) -> int:
        t = C.c_uint32(0)
        _chk(lib().jpk_dev_exclusive_scan_u32(self._h, _dptr(d_data), n, C.byref(t)), "jpk_dev_exclusive_scan_u32")
        return t.value

    def rle_encode(self, d_ranks, n, d_rle) -> int:
        r = C.c_int32(0)
        _chk(lib().jpk_dev_rle_encode(self._h, _dptr(d_ranks), n, _dptr(d_rle), C.byref(r)), "jpk_dev_rle_encode")
        return r.value

    def model_pairs(self, d_rle, rlen, d_pairs):
        _chk(lib().jpk_dev_model_pairs(self._h, _dptr(d_rle), rlen, _dptr(d_pairs)), "jpk_dev_model_pairs")


def multi_plan(device_mask: int, ndev_visible: int, nblocks: int):
    """jpk_debug_multi_plan: (devices taking part, owner device of every block) -- host logic only"""
    own = (C.c_int32 * max(nblocks, 1))()
    g = lib().jpk_debug_multi_plan(device_mask, ndev_visible, nblocks, own)
    _chk(g if g < 0 else 0, "jpk_debug_multi_plan")
    return g, list(own)[:nblocks]


def blocks_compress_multi(blocks, d_out, out_cap: int, device_mask: int = 0, in_flight: int = 0, check: bool = True):
    """jpk_blocks_compress_multi(_ex): host blocks -> compressed blocks gathered in block order into `d_out` (a device buffer on the first
    device of the mask; anything with data_ptr() or an int address), `in_flight` blocks in flight per device (0: the library's default).
    Returns (offsets [nblocks + 1], status [nblocks]); check=False: no exception for a failed block, returns (offsets, status, rc) --
    the blocks whose status is 0 are in d_out whatever happened to the others."""
    arrs = [_np_u8(b) for b in blocks]
    n = len(arrs)
    P, I = C.c_void_p * max(n, 1), C.c_int32 * max(n, 1)
    ins = P(*[a.ctypes.data if len(a) else None for a in arrs])
    lens = I(*[len(a) for a in arrs])
    off = (C.c_int64 * (n + 1))()
    st = I()
    rc = lib().jpk_blocks_compress_multi_ex(device_mask, n, ins, lens, _dptr(d_out), out_cap, off, st, in_flight)
    if not check:
        return list(off), list(st)[:n], int(rc)
    _chk(rc, "jpk_blocks_compress_multi")
    return list(off), list(st)[:n]


def blocks_decompress_multi(comp_blocks, raw_lens, d_out, out_cap: int, device_mask: int = 0, check: bool = True):
    """jpk_blocks_decompress_multi: host compressed blocks (+ the decompressed size of each) -> the blocks' bytes gathered in block order
    into `d_out` on the first device of the mask.  Returns (offsets [nblocks + 1], status [nblocks]); check=False: (offsets, status, rc),
    no exception -- the blocks whose status is 0 are in d_out whatever happened to the others."""
    arrs = [_np_u8(b) for b in comp_blocks]
    n = len(arrs)
    P, I = C.c_void_p * max(n, 1), C.c_int32 * max(n, 1)
    ins = P(*[a.ctypes.data if len(a) else None for a in arrs])
    lens = I(*[len(a) for a in arrs])
    raw = I(*[int(x) for x in raw_lens])
    off = (C.c_int64 * (n + 1))()
    st = I()
    rc = lib().jpk_blocks_decompress_multi(device_mask, n, ins, lens, raw, _dptr(d_out), out_cap, off, st)
    if not check:
        return list(off), list(st)[:n], int(rc)
    _chk(rc, "jpk_blocks_decompress_multi")
    return list(off), list(st)[:n]
