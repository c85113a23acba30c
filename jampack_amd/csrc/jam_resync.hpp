// jam_resync.hpp -- the rule by which a damaged .jam archive is walked past its damage ("Damaged archives"), written once for
// the host drivers (jam_archive.hip), the kernels (jam.hip: the header test of k_jam_walk and k_jam_scan_*) and two stand-alone programs
// (tests/jam_resync_rule_host.cpp, and tests/jam_resync_cli_rule_host.cpp for stock-CLI archives) that run it under a sanitizer:
//   fields_ok / magic_ok   a plausible frame header at an offset -- exactly what k_jam_walk and jpk_jam_header_parse accept
//   ans_decoded_size       the chunk-header walk of a payload (jpk_ans_decoded_size is this function)
//   decoded_ok             what a payload may declare against its BlockSize
//   frame_at               a structurally valid frame in host memory: the three together, no more and no fewer than the walks apply
//   walk                   the resync walk, a template over where candidates come from and how a batch of them is validated; HostSrc is
//                          that pair for an archive in host memory -- of plain frames, of plain and staged ones, or (cli) of the stock CLI,
//                          whose frames may declare what a chained frame may (decoded_ok)
// Pure functions, no HIP header: magic_ok and fields_ok compile for the device too, the rest is host code.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/jampack_abi.h"
#include "prestage_rules.hpp"

// one frame of an archive as the walks see it: where its payload is, its header fields and its raw (decompressed) size
// (staged: a staged frame, DESIGN 4.6 -- block_size is the field without JPK_JAM_STAGED, raw the bytes of its S2)
struct JamFrame { int64_t payload_off; int32_t psize; uint32_t crc; int32_t block_size; int64_t raw; bool staged = false; };

namespace jrs {

JPK_HD bool magic_ok(uint32_t b0, uint32_t b1, uint32_t b2) { return b0 == 'J' && b1 == 'A' && b2 == 'M'; }

// the header fields behind the magic, `avail` bytes from the header's first byte to the end of the archive: MIN_BLOCKSIZE <= BlockSize <=
// MAX_BLOCKSIZE (staged_ok: JPK_JAM_STAGED, bit 30, may be set in a field whose bit 31 is clear), 0 <= payload size <= MAX_BLOCKSIZE,
// and header and payload end inside the archive
JPK_HD bool fields_ok(int32_t psize, int32_t field, int64_t avail, bool staged_ok)
{
    const int32_t bs = (staged_ok && field > 0) ? (field & ~JPK_JAM_STAGED) : field;
    return avail >= JPK_JAM_HEADER_BYTES && bs >= JPK_MIN_BLOCKSIZE && bs <= JPK_MAX_BLOCKSIZE && psize >= 0 && psize <= JPK_MAX_BLOCKSIZE &&
           (int64_t)psize <= avail - JPK_JAM_HEADER_BYTES;
}

// the checks of the frame walk beyond its header: the payload declares at least the BWT trailer and at most BlockSize raw bytes (the
// reference decodes into buffers of 1.05 x BlockSize, jampack.cpp:156-159) -- for a frame whose entropy-decoded bytes are the output of
// pre-stages (chained: stock-CLI and staged frames; filter headers and LZ tokens add bytes), at most the reference's stage buffers,
// 1.05 x BlockSize + 4096 (jampack.cpp:156)
inline int32_t cli_cap(int32_t block_size) { return (int32_t)((int64_t)((double)block_size * 1.05) + 4096); }
inline bool decoded_ok(int64_t decoded, int32_t block_size, bool chained)
{
    return decoded >= JPK_TRAILER_BYTES && decoded - JPK_TRAILER_BYTES <= (chained ? cli_cap(block_size) : block_size);
}

// Ans::Decode's chunk headers (ans.cpp:272-302) from first to last: 256 frequencies that sum to the chunk's length, chunks that tile the
// payload exactly.  *decoded_len = the bytes they declare
inline int ans_decoded_size(const uint8_t *in, int32_t in_len, int64_t *decoded_len, int32_t *chunks)
{
    int64_t ip = 0, total = 0;
    int32_t nch = 0;
    while (ip < in_len) {
        int64_t fsum = 0;
        uint32_t v = 0, olen = 0;
        for (int s = 0; s < 259; s++) {                 // 256 frequencies, olen, clen, rlen
            const int n = pre::leb_read(in + ip, (int64_t)in_len - ip, &v);
            if (n < 0) return JPK_E_CORRUPT;
            ip += n;
            if (s < 256) { if (v > (uint32_t)JPK_ANS_CHUNK) return JPK_E_CORRUPT; fsum += v; }
            else if (s == 256) { if (v > (uint32_t)JPK_ANS_CHUNK || (int64_t)v != fsum) return JPK_E_CORRUPT; total += v; olen = v; }
            else if (s == 257) { if (v < 16 || (int64_t)v > (int64_t)in_len - ip) return JPK_E_CORRUPT; fsum = v; }   // clen, payload follows rlen
            else { if (v > olen) return JPK_E_CORRUPT; }     // RLE0 never has more symbols than bytes ("rle mismatch!", rle.cpp:73)
        }
        if (fsum > (int64_t)in_len - ip) return JPK_E_CORRUPT;
        ip += fsum;                                      // skip the payload
        nch++;
    }
    *decoded_len = total;
    if (chunks) *chunks = nch;
    return JPK_OK;
}

// the header at in + o of an archive of in_len bytes: plausible?  f = its fields (f->staged only with staged_ok)
inline bool header_at(const uint8_t *in, int64_t in_len, int64_t o, bool staged_ok, JamFrame *f)
{
    if (o < 0 || in_len - o < JPK_JAM_HEADER_BYTES || !magic_ok(in[o], in[o + 1], in[o + 2])) return false;
    int32_t field;
    memcpy(&f->crc, in + o + 3, 4);
    memcpy(&f->psize, in + o + 7, 4);
    memcpy(&field, in + o + 11, 4);
    if (!fields_ok(f->psize, field, in_len - o, staged_ok)) return false;
    f->staged = staged_ok && (field & JPK_JAM_STAGED) != 0;
    f->block_size = f->staged ? (field & ~JPK_JAM_STAGED) : field;
    f->payload_off = o + JPK_JAM_HEADER_BYTES;
    return true;
}

// a structurally valid frame starts at o: a plausible header, a payload whose chunk headers walk, a declared size the BlockSize allows
// (cli: every frame is one of the stock CLI).  f->raw = the entropy-decoded bytes without the BWT trailer
inline bool frame_at(const uint8_t *in, int64_t in_len, int64_t o, bool staged_ok, bool cli, JamFrame *f)
{
    int64_t decoded = 0;
    if (!header_at(in, in_len, o, staged_ok, f)) return false;
    if (ans_decoded_size(in + f->payload_off, f->psize, &decoded, nullptr) != JPK_OK || !decoded_ok(decoded, f->block_size, cli || f->staged)) return false;
    f->raw = decoded - JPK_TRAILER_BYTES;
    return true;
}

// ---- the resync walk ------------------------------------------------------------------------------------------------------------------
//   g = 0
//   while g < in_len:
//       o = the smallest o' >= g at which a structurally valid frame starts (none: in_len)
//       o > g: gap(g, o - g, frames so far);  o == in_len: stop;  else append the frame at o, g = o + 15 + psize
// The smallest valid offset is searched in rounds: the first K plausible offsets of the window [p, min(in_len, p + W)) in increasing
// order, validated in one batch, the first valid one taken; none valid: on behind the last candidate seen, or behind the window when it
// held fewer than K.  The result depends on neither K nor W.
constexpr int64_t DEFAULT_WINDOW = 256ll << 20;
constexpr int32_t DEFAULT_CANDS = 4096;

// Src, the archive as the walk needs it (every member returns a status, JPK_OK to go on):
//   run(g, on_frame, &stop)            the consecutive structurally valid frames from offset g, each handed to on_frame(const JamFrame &);
//                                      *stop = the offset behind the last one (in_len, or where no valid frame starts)
//   cands(from, to, K, &n)             the first K plausible offsets in [from, to), ascending; *n = how many it holds now
//   cand(i)                            offset of candidate i
//   first_valid(n, &i, &f)             *i = the first of the n candidates that is structurally valid and f its frame, or -1
// on_frame(const JamFrame &) and on_gap(archive_off, archive_len) see frames and gaps in archive order; together they tile [0, in_len).
template <class Src, class OnFrame, class OnGap> int walk(Src &src, int64_t in_len, int64_t W, int32_t K, OnFrame on_frame, OnGap on_gap)
{
    if (W < 1) W = DEFAULT_WINDOW;
    if (K < 1) K = DEFAULT_CANDS;
    int64_t g = 0;
    while (g < in_len) {
        int64_t stop = g;
        if (int rc = src.run(g, on_frame, &stop)) return rc;
        g = stop;
        if (g >= in_len) break;
        // no valid frame at g: the first one behind it
        int64_t p = g, o = in_len;
        JamFrame f;
        while (p < in_len && o == in_len) {
            const int64_t end = W < in_len - p ? p + W : in_len;
            int32_t n = 0, hit = -1;
            if (int rc = src.cands(p, end, K, &n)) return rc;
            if (n > 0) if (int rc = src.first_valid(n, &hit, &f)) return rc;
            if (hit >= 0) o = src.cand(hit);
            else p = n >= K ? src.cand(n - 1) + 1 : end;
        }
        on_gap(g, o - g);
        if (o == in_len) break;
        on_frame(f);
        g = f.payload_off + f.psize;
    }
    return JPK_OK;
}

// Src for an archive in host memory: plain frames, with staged_ok staged ones too, or with cli (and staged_ok false: a stock-CLI header
// has no staged bit) the frames of the stock CLI, every one measured against the slot of a chained frame.  cli stays the last member:
// HostSrc{in, in_len, staged_ok, offs} is the source of kinds 0 and 2
struct HostSrc {
    const uint8_t *in;
    int64_t in_len;
    bool staged_ok;
    int64_t *offs;           // room for K offsets
    bool cli = false;
    template <class OnFrame> int run(int64_t g, OnFrame on_frame, int64_t *stop)
    {
        JamFrame f;
        while (g < in_len && frame_at(in, in_len, g, staged_ok, cli, &f)) { on_frame(f); g = f.payload_off + f.psize; }
        *stop = g;
        return JPK_OK;
    }
    int cands(int64_t from, int64_t to, int32_t K, int32_t *n)
    {
        JamFrame f;
        int32_t k = 0;
        const int64_t last = in_len - JPK_JAM_HEADER_BYTES;            // the last offset a header fits at
        for (int64_t o = from; o < to && o <= last && k < K;) {
            const void *j = memchr(in + o, 'J', (size_t)((to < last + 1 ? to : last + 1) - o));
            if (!j) break;
            o = (const uint8_t *)j - in;
            if (header_at(in, in_len, o, staged_ok, &f)) offs[k++] = o;
            o++;
        }
        *n = k;
        return JPK_OK;
    }
    int64_t cand(int32_t i) const { return offs[i]; }
    int first_valid(int32_t n, int32_t *hit, JamFrame *f)
    {
        *hit = -1;
        for (int32_t i = 0; i < n && *hit < 0; i++) if (frame_at(in, in_len, offs[i], staged_ok, cli, f)) *hit = i;
        return JPK_OK;
    }
};

}  // namespace jrs
