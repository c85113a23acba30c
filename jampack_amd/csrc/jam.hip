// jam.hip -- the frames of a .jam archive on gfx950 (Jampack::Compress / Decompress, jampack.cpp:186-336):
//   k_jam_walk   one wave walks the frame headers of an archive in HBM (DecompReadBlock's checks, jampack.cpp:140-163)
//   k_jam_pack   writes a run of frames -- "JAM" | u32 crc | i32 payload size | i32 BlockSize | payload, little-endian --
//                from payload slots in scratch, organised by destination: a thread owns aligned 16-byte words of the output
//   k_jam_gather delivers the pieces of a range read -- (source, destination, length) of decoded bytes -- organised by destination
//                in the same way: a thread owns aligned 16-byte words of a piece's destination
//   k_jam_splice writes a stretch of an updated archive -- kept frames copied from the old archive and new frames from payload slots, each
//                with a BlockSize field of its own -- organised by destination as k_jam_pack is
//   k_jam_scan_* the plausible frame headers of a window of an archive, in ascending order: where a walk past damage looks for the next
//                frame (jam_resync.hpp; DESIGN 4.6, "Damaged archives")
// The ABI entries that drive them are jpk_dev_jam_compress / jpk_dev_jam_decompress / jpk_dev_jam_read (jam_archive.hip).
#include "common.hpp"
#include "jam_resync.hpp"

namespace {

constexpr int PACK_TB = 256;

// One wave.  A frame's 15 header bytes are loaded by lanes 0..14 at once; the chain of frames is serial by format (frame k + 1 starts
// behind frame k's payload).  A frame is accepted as DecompReadBlock accepts it: magic "JAM", MIN_BLOCKSIZE <= BlockSize <=
// MAX_BLOCKSIZE, 0 <= payload size <= MAX_BLOCKSIZE, and the payload ends inside the archive; 1..14 bytes left over are a bad frame too.
// staged_ok: a BlockSize field with JPK_JAM_STAGED (bit 30) set is checked without it and goes into the table as it is.
__global__ __launch_bounds__(64) void k_jam_walk(const uint8_t *__restrict__ in, uint64_t in_len, uint64_t start, uint32_t max_frames,
                                                 JamWalkFrame *__restrict__ table, uint32_t *__restrict__ mail, uint32_t staged_ok)
{
    const int l = (int)(threadIdx.x & 63u);
    uint64_t o = start;
    uint32_t count = 0, bad = 0;
    while (count < max_frames && o < in_len) {
        if (in_len - o < (uint64_t)JPK_JAM_HEADER_BYTES) { bad = 1; break; }
        const int mine = (l < JPK_JAM_HEADER_BYTES) ? (int)in[o + (uint64_t)l] : 0;
        uint32_t h[JPK_JAM_HEADER_BYTES];
#pragma unroll
        for (int j = 0; j < JPK_JAM_HEADER_BYTES; j++) h[j] = (uint32_t)__builtin_amdgcn_readlane(mine, j);
        const uint32_t crc = h[3] | (h[4] << 8) | (h[5] << 16) | (h[6] << 24);
        const int32_t psize = (int32_t)(h[7] | (h[8] << 8) | (h[9] << 16) | (h[10] << 24));
        const int32_t field = (int32_t)(h[11] | (h[12] << 8) | (h[13] << 16) | (h[14] << 24));
        if (!jrs::magic_ok(h[0], h[1], h[2]) || !jrs::fields_ok(psize, field, (int64_t)(in_len - o), staged_ok != 0)) { bad = 1; break; }
        if (l == 0) {
            JamWalkFrame f;
            f.payload_off = o + JPK_JAM_HEADER_BYTES; f.psize = psize; f.crc = crc; f.block_size = field; f.pad = 0;
            table[count] = f;
        }
        o += (uint64_t)JPK_JAM_HEADER_BYTES + (uint64_t)psize;
        count++;
    }
    if (l == 0) {
        mail[0] = count;
        mail[1] = bad;
        mail[2] = (uint32_t)o;
        mail[3] = (uint32_t)(o >> 32);
    }
}

// byte p (0 <= p - off < 15 + psize) of frame f: header or payload
__device__ __forceinline__ uint32_t frame_byte(uint64_t rel, uint32_t crc, int32_t psize, int32_t bs, const uint8_t *slot)
{
    if (rel >= (uint64_t)JPK_JAM_HEADER_BYTES) return slot[rel - JPK_JAM_HEADER_BYTES];
    const uint32_t r = (uint32_t)rel;
    if (r < 3) return r == 0 ? 'J' : (r == 1 ? 'A' : 'M');
    const uint32_t v = r < 7 ? crc : (r < 11 ? (uint32_t)psize : (uint32_t)bs);
    const uint32_t k = r < 7 ? r - 3 : (r < 11 ? r - 7 : r - 11);
    return (v >> (8 * k)) & 0xFFu;
}

// Organised by destination: word w is the aligned 16 bytes at base + 16 w (base = d_out rounded down to 16).  Its owner finds the frame
// of its first byte by a search over the frame offsets, and then either (the whole word inside one payload) moves 16 payload bytes
// through two aligned loads, or assembles the word byte by byte from headers and payloads.  Every whole word is written once with
// one 16-byte store; only the partial words at the two ends of the range use byte stores, each byte by its word's owner.
__global__ __launch_bounds__(PACK_TB) void k_jam_pack(const JamPackFrame *__restrict__ frames, uint32_t n, const uint32_t *__restrict__ crcs,
                                                      int32_t bs, uint8_t *__restrict__ out, uint64_t total)
{
    __shared__ uint64_t s_off[JPK_JAM_PASS_FRAMES + 1];
    __shared__ const uint8_t *s_slot[JPK_JAM_PASS_FRAMES];
    __shared__ int32_t s_psize[JPK_JAM_PASS_FRAMES];
    __shared__ uint32_t s_crc[JPK_JAM_PASS_FRAMES];
    for (uint32_t i = threadIdx.x; i < n; i += PACK_TB) {
        const JamPackFrame f = frames[i];
        s_off[i] = f.off; s_slot[i] = f.slot; s_psize[i] = f.psize; s_crc[i] = crcs[i];
    }
    if (threadIdx.x == 0) s_off[n] = total;
    __syncthreads();
    const uintptr_t base = (uintptr_t)out & ~(uintptr_t)15;
    const int64_t lead = (int64_t)((uintptr_t)out - base);                     // bytes of the first word in front of the range
    const uint64_t words = ((uint64_t)lead + total + 15u) / 16u;
    for (uint64_t w = (uint64_t)blockIdx.x * PACK_TB + threadIdx.x; w < words; w += (uint64_t)gridDim.x * PACK_TB) {
        const int64_t p0 = (int64_t)(w * 16u) - lead;                          // archive position of the word's first byte (< 0: before the range)
        const uint64_t first = p0 < 0 ? 0u : (uint64_t)p0;
        uint32_t lo = 0, hi = n;                                              // frame of `first`: the last with s_off <= first
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s_off[mid] <= first) lo = mid; else hi = mid; }
        uint32_t f = lo;
        uint8_t *dst = reinterpret_cast<uint8_t *>(base + w * 16u);
        const bool whole = p0 >= 0 && (uint64_t)p0 + 16u <= total;
        const uint64_t pay = s_off[f] + JPK_JAM_HEADER_BYTES;
        if (whole && (uint64_t)p0 >= pay && (uint64_t)p0 + 16u <= pay + (uint64_t)s_psize[f]) {
            *reinterpret_cast<uint4 *>(dst) = load16_unaligned(s_slot[f] + ((uint64_t)p0 - pay));
            continue;
        }
        uint32_t b[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            b[j] = 0;
            if (p < 0 || (uint64_t)p >= total) continue;
            while (f + 1 < n && (uint64_t)p >= s_off[f + 1]) f++;
            b[j] = frame_byte((uint64_t)p - s_off[f], s_crc[f], s_psize[f], bs, s_slot[f]);
            if (!whole) dst[j] = (uint8_t)b[j];
        }
        if (whole) {
            uint4 v;
            v.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            v.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            v.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            v.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
            *reinterpret_cast<uint4 *>(dst) = v;
        }
    }
}

// Organised by destination, piece by piece: word w of piece i is the aligned 16 bytes at base_i + 16 (w - word0_i) (base_i = the piece's
// dst rounded down to 16), and word0 is the prefix sum of the pieces' word counts, so a thread finds the piece of its word by a search
// over word0.  A word that lies wholly inside the piece is written with one 16-byte store -- fed by load16_unaligned when its two
// aligned loads stay inside [src_lo, src_hi), the bytes the source may be read at (a scratch slot with its padding; a frame decoded
// in place in a caller's buffer has none, so the words at its ends are assembled byte by byte); the partial words at the piece's two
// ends use byte stores.  Nothing outside [dst, dst + len) is written, so pieces that share a destination word do not disturb each other.
// The search is log2(n) reads of 48-byte entries per word, through L2 (the table of a call is not bounded, so it is not staged in LDS as
// k_jam_pack's 128 frames are): neighbouring threads walk the same entries, and next to the decode of whole frames that every read
// pays for, the gather is small (profiles/jam_read_ranges.txt, variant c).
__global__ __launch_bounds__(PACK_TB) void k_jam_gather(const JamGatherPiece *__restrict__ pieces, uint32_t n, uint64_t words)
{
    for (uint64_t w = (uint64_t)blockIdx.x * PACK_TB + threadIdx.x; w < words; w += (uint64_t)gridDim.x * PACK_TB) {
        uint32_t lo = 0, hi = n;                                              // piece of word w: the last with word0 <= w
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (pieces[mid].word0 <= w) lo = mid; else hi = mid; }
        const JamGatherPiece pc = pieces[lo];
        const uintptr_t d = (uintptr_t)pc.dst, base = d & ~(uintptr_t)15;
        const int64_t p0 = (int64_t)((w - pc.word0) * 16u) - (int64_t)(d - base);   // piece position of the word's first byte (< 0: before the piece)
        uint8_t *dst = reinterpret_cast<uint8_t *>(base + (w - pc.word0) * 16u);
        if (p0 >= 0 && (uint64_t)p0 + 16u <= pc.len) {
            const uint8_t *src = pc.src + p0;
            const uintptr_t a = (uintptr_t)src & ~(uintptr_t)15;
            uint4 v;
            if (a >= (uintptr_t)pc.src_lo && a + (((uintptr_t)src & 15u) ? 32u : 16u) <= (uintptr_t)pc.src_hi) {
                v = load16_unaligned(src);
            } else {
                uint32_t b[16];
#pragma unroll
                for (int j = 0; j < 16; j++) b[j] = src[j];
                v.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
                v.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
                v.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
                v.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
            }
            *reinterpret_cast<uint4 *>(dst) = v;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            if (p >= 0 && (uint64_t)p < pc.len) dst[j] = pc.src[p];
        }
    }
}

// Organised by destination like k_jam_pack: word w is the aligned 16 bytes at base + 16 w (base = out rounded down to 16), and its owner
// finds the frame of its first byte by a search over the frames' offsets.  The frames are of two sorts, in any mix: a kept frame is 15 +
// psize contiguous bytes of the archive, header included; a new frame is a header made of its fields in front of a payload slot, the
// BlockSize field its own.  A whole word inside one source -- a kept frame's span, a new frame's payload -- takes one unaligned 16-byte
// load (two aligned ones) and one 16-byte store; the two aligned loads of a kept frame must stay inside [in_lo, in_hi), the archive, which
// has no padding, so the few words at the archive's two ends go the other way: byte by byte, as every word that straddles a frame edge
// or holds header bytes of a new frame.  Only the partial words at the two ends of the stretch use byte stores; nothing outside
// [out, out + total) is written.  A stretch holds the kept frames between two passes, thousands perhaps, so the table is read through L2
// as k_jam_gather's is (32-byte entries, log2(n) of them per word, neighbouring threads the same ones), not staged in LDS.
__global__ __launch_bounds__(PACK_TB) void k_jam_splice(const JamSpliceFrame *__restrict__ frames, uint32_t n, uint8_t *__restrict__ out, uint64_t total,
                                                        const uint8_t *in_lo, const uint8_t *in_hi)
{
    const uintptr_t base = (uintptr_t)out & ~(uintptr_t)15;
    const int64_t lead = (int64_t)((uintptr_t)out - base);                     // bytes of the first word in front of the stretch
    const uint64_t words = ((uint64_t)lead + total + 15u) / 16u;
    for (uint64_t w = (uint64_t)blockIdx.x * PACK_TB + threadIdx.x; w < words; w += (uint64_t)gridDim.x * PACK_TB) {
        const int64_t p0 = (int64_t)(w * 16u) - lead;                          // stretch position of the word's first byte (< 0: before the stretch)
        const uint64_t first = p0 < 0 ? 0u : (uint64_t)p0;
        uint32_t lo = 0, hi = n;                                              // frame of `first`: the last with off <= first
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (frames[mid].off <= first) lo = mid; else hi = mid; }
        uint32_t f = lo;
        JamSpliceFrame fr = frames[f];
        uint8_t *dst = reinterpret_cast<uint8_t *>(base + w * 16u);
        const bool whole = p0 >= 0 && (uint64_t)p0 + 16u <= total;
        if (whole) {
            // the contiguous source the word may lie in: the frame's span in the archive, or its payload in the slot
            const uint64_t s0 = fr.off + (fr.kept ? 0u : (uint64_t)JPK_JAM_HEADER_BYTES), s1 = fr.off + JPK_JAM_HEADER_BYTES + (uint64_t)fr.psize;
            if ((uint64_t)p0 >= s0 && (uint64_t)p0 + 16u <= s1) {
                const uint8_t *src = fr.src + ((uint64_t)p0 - s0);
                const uintptr_t a = (uintptr_t)src & ~(uintptr_t)15;
                if (!fr.kept || (a >= (uintptr_t)in_lo && a + (((uintptr_t)src & 15u) ? 32u : 16u) <= (uintptr_t)in_hi)) {
                    *reinterpret_cast<uint4 *>(dst) = load16_unaligned(src);
                    continue;
                }
            }
        }
        uint32_t b[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            b[j] = 0;
            if (p < 0 || (uint64_t)p >= total) continue;
            while (f + 1 < n && (uint64_t)p >= frames[f + 1].off) fr = frames[++f];
            const uint64_t rel = (uint64_t)p - fr.off;
            b[j] = fr.kept ? (uint32_t)fr.src[rel] : frame_byte(rel, fr.crc, fr.psize, fr.field, fr.src);
            if (!whole) dst[j] = (uint8_t)b[j];
        }
        if (whole) {
            uint4 v;
            v.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            v.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            v.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            v.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
            *reinterpret_cast<uint4 *>(dst) = v;
        }
    }
}

// ---- k_jam_scan_count / k_jam_scan_emit: the plausible headers (jrs::magic_ok + jrs::fields_ok) that start in [start, end) -----------
// A streaming read.  Word w is the aligned 16 bytes at base + 16 w, base = `in` rounded down to 16; a lane loads SCAN_ROWS words per tile,
// 64 words apart, so a wave's loads are 1 KiB each and a tile is SCAN_TILE = 4 KiB of one wave's own.  A lane tests the 16 offsets of a
// word for the magic in registers; the two bytes behind its word are the first dword of its neighbour's word (the last lane's: the
// first lane's next row, and behind the tile one overlapping dword load).  The other 12 header bytes are read only on a magic hit.
// Only words that hold a byte of the archive are loaded (an aligned word lies in one page), and no offset o with o + 15 > in_len is
// looked at, so nothing at or behind in + in_len reaches the result; `in` and start may have any alignment.
// The order comes from position alone: k_jam_scan_count leaves the hits of tile t in counts[t] (ballot + popcount per offset column, and
// only in a row that has a hit), the host scans them (jpk_dev_exclusive_scan_u32 over ntiles + 1 words), and k_jam_scan_emit walks the
// tiles that hold a rank below K again and writes candidate r to out[r]: rank = the tile's prefix + the hits of the rows and lanes in
// front + the hits below in the lane's own word.  No atomics, no LDS; the grid is capped and strides by waves.
constexpr int SCAN_TB = 256, SCAN_ROWS = 4, SCAN_TILE = SCAN_ROWS * 64 * 16;

// the hits among the 16 offsets of the lane's word x (nxt: the dword behind it); o0 = the archive offset of the word's first byte
__device__ __forceinline__ uint32_t scan_word(const uint8_t *__restrict__ in, int64_t in_len, int64_t start, int64_t end, bool staged_ok, int64_t o0, uint4 x,
                                              uint32_t nxt)
{
    // offsets [lo, hi) of the word are in the window and leave room for a header
    const int64_t top = end < in_len - (JPK_JAM_HEADER_BYTES - 1) ? end : in_len - (JPK_JAM_HEADER_BYTES - 1);
    const int64_t lo64 = start - o0, hi64 = top - o0;
    if (hi64 <= 0 || lo64 >= 16) return 0u;
    const uint32_t lo = lo64 < 0 ? 0u : (uint32_t)lo64, hi = hi64 > 16 ? 16u : (uint32_t)hi64;
    const uint32_t v[5] = {x.x, x.y, x.z, x.w, nxt};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t t = __builtin_amdgcn_alignbyte(v[j / 4 + 1], v[j / 4], j & 3) & 0xFFFFFFu;
        m |= (t == ('J' | ('A' << 8) | ('M' << 16)) ? 1u : 0u) << j;
    }
    m &= (0xFFFFu << lo) & (0xFFFFu >> (16u - hi));
    uint32_t hits = 0;
    while (m) {                                                                // rare: a magic in the window
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const uint8_t *h = in + (o0 + j);
        const int32_t psize = (int32_t)((uint32_t)h[7] | ((uint32_t)h[8] << 8) | ((uint32_t)h[9] << 16) | ((uint32_t)h[10] << 24));
        const int32_t field = (int32_t)((uint32_t)h[11] | ((uint32_t)h[12] << 8) | ((uint32_t)h[13] << 16) | ((uint32_t)h[14] << 24));
        if (jrs::fields_ok(psize, field, in_len - (o0 + j), staged_ok)) hits |= 1u << j;
    }
    return hits;
}

template <bool EMIT>
__device__ __forceinline__ void scan_tiles(const uint8_t *__restrict__ in, int64_t in_len, int64_t start, int64_t end, bool staged_ok, uint32_t ntiles,
                                           uint32_t *__restrict__ counts, JamWalkFrame *__restrict__ out, uint32_t K)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * SCAN_TB + threadIdx.x) >> 6, nwaves = gridDim.x * (SCAN_TB / 64);
    const int64_t lead = (int64_t)((uintptr_t)in & 15u);
    const uint8_t *base = in - lead;
    const int64_t w_lo = (lead + start) >> 4, w_hi = (lead + in_len + 15) >> 4;   // the window's first word; the words with a byte of the archive
    for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {                    // (wave-uniform)
        uint32_t rank = 0;
        if (EMIT) {
            rank = (uint32_t)__builtin_amdgcn_readfirstlane((int)counts[tile]);
            const uint32_t next = (uint32_t)__builtin_amdgcn_readfirstlane((int)counts[tile + 1]);
            if (next == rank || rank >= K) continue;
        }
        const int64_t w0 = w_lo + (int64_t)tile * (SCAN_ROWS * 64) + lane;
        uint4 x[SCAN_ROWS];
#pragma unroll
        for (int u = 0; u < SCAN_ROWS; u++) {
            const int64_t w = w0 + u * 64;
            x[u] = make_uint4(0u, 0u, 0u, 0u);
            if (w < w_hi) x[u] = *reinterpret_cast<const uint4 *>(base + w * 16);
        }
        uint32_t behind = 0;                                                       // the dword behind the tile, for its last lane
        if (lane == 63u && w0 + (SCAN_ROWS - 1) * 64 + 1 < w_hi) behind = *reinterpret_cast<const uint32_t *>(base + (w0 + (SCAN_ROWS - 1) * 64 + 1) * 16);
        uint32_t total = 0;
#pragma unroll
        for (int u = 0; u < SCAN_ROWS; u++) {
            uint32_t nxt = (uint32_t)__shfl_down((int)x[u].x, 1);
            const uint32_t row_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)x[(u + 1) % SCAN_ROWS].x);   // the first lane's word of the next row
            if (lane == 63u) nxt = u + 1 < SCAN_ROWS ? row_next : behind;
            const int64_t o0 = (w0 + u * 64) * 16 - lead;
            const uint32_t hits = scan_word(in, in_len, start, end, staged_ok, o0, x[u], nxt);
            if (__ballot(hits != 0u) == 0ull) continue;                           // (wave-uniform)
            uint32_t before = 0, row = 0;                                          // hits of the lanes in front; of the row
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint64_t b = __ballot((hits >> j) & 1u);
                before += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                row += (uint32_t)__popcll(b);
            }
            if (EMIT) {
                uint32_t m = hits, r = rank + total + before;
                while (m) {
                    const uint32_t j = (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                    if (r < K) {
                        const uint8_t *h = in + (o0 + j);
                        JamWalkFrame f;
                        f.payload_off = (uint64_t)(o0 + j) + JPK_JAM_HEADER_BYTES;
                        f.crc = (uint32_t)h[3] | ((uint32_t)h[4] << 8) | ((uint32_t)h[5] << 16) | ((uint32_t)h[6] << 24);
                        f.psize = (int32_t)((uint32_t)h[7] | ((uint32_t)h[8] << 8) | ((uint32_t)h[9] << 16) | ((uint32_t)h[10] << 24));
                        f.block_size = (int32_t)((uint32_t)h[11] | ((uint32_t)h[12] << 8) | ((uint32_t)h[13] << 16) | ((uint32_t)h[14] << 24));
                        f.pad = 0;
                        out[r] = f;
                    }
                    r++;
                }
            }
            total += row;
        }
        if (!EMIT && lane == 0u) counts[tile] = total;
    }
    if (!EMIT && blockIdx.x == 0 && threadIdx.x == 0) counts[ntiles] = 0u;        // the scan's last word: its prefix is the total
}

__global__ __launch_bounds__(SCAN_TB) void k_jam_scan_count(const uint8_t *__restrict__ in, int64_t in_len, int64_t start, int64_t end, uint32_t staged_ok,
                                                            uint32_t ntiles, uint32_t *__restrict__ counts)
{
    scan_tiles<false>(in, in_len, start, end, staged_ok != 0u, ntiles, counts, nullptr, 0u);
}

// counts: the exclusive prefix sums of k_jam_scan_count's, ntiles + 1 words
__global__ __launch_bounds__(SCAN_TB) void k_jam_scan_emit(const uint8_t *__restrict__ in, int64_t in_len, int64_t start, int64_t end, uint32_t staged_ok,
                                                           uint32_t ntiles, uint32_t *__restrict__ counts, JamWalkFrame *__restrict__ out, uint32_t K)
{
    scan_tiles<true>(in, in_len, start, end, staged_ok != 0u, ntiles, counts, out, K);
}

}  // namespace

int jpk_jam_walk_enqueue(jpk_ctx *ctx, const uint8_t *d_in, uint64_t in_len, uint64_t start, uint32_t max_frames, JamWalkFrame *d_table,
                         uint32_t *d_mail, bool staged_ok)
{
    JPK_LAUNCH(ctx, PROF_JAM, 0, k_jam_walk, dim3(1), dim3(64), d_in, in_len, start, max_frames, d_table, d_mail, staged_ok ? 1u : 0u);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

int jpk_jam_pack_enqueue(jpk_ctx *ctx, const JamPackFrame *d_frames, int n, const uint32_t *d_crc, int32_t block_size, uint8_t *d_out, uint64_t total)
{
    if (n <= 0 || n > JPK_JAM_PASS_FRAMES) return JPK_E_ARG;
    if (total == 0) return JPK_OK;
    const uint64_t words = (total + 31u) / 16u;
    uint64_t grid = (words + PACK_TB - 1) / PACK_TB;
    if (grid > 8192) grid = 8192;                                              // grid-stride beyond: 2M threads cover a pass
    JPK_LAUNCH(ctx, PROF_JAM, total, k_jam_pack, dim3((unsigned)grid), dim3(PACK_TB), d_frames, (uint32_t)n, d_crc, block_size, d_out, total);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

int jpk_jam_gather_enqueue(jpk_ctx *ctx, const JamGatherPiece *d_pieces, uint32_t n, uint64_t words, uint64_t bytes)
{
    if (n == 0 || words == 0) return JPK_OK;
    uint64_t grid = (words + PACK_TB - 1) / PACK_TB;
    if (grid > 8192) grid = 8192;                                              // grid-stride beyond, as k_jam_pack
    JPK_LAUNCH(ctx, PROF_JAM, bytes, k_jam_gather, dim3((unsigned)grid), dim3(PACK_TB), d_pieces, n, words);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

int jpk_jam_splice_enqueue(jpk_ctx *ctx, const JamSpliceFrame *d_frames, uint32_t n, uint8_t *d_out, uint64_t total, const uint8_t *in_lo, const uint8_t *in_hi)
{
    if (n == 0 || total == 0) return JPK_OK;
    const uint64_t words = (total + 31u) / 16u;
    uint64_t grid = (words + PACK_TB - 1) / PACK_TB;
    if (grid > 8192) grid = 8192;                                              // grid-stride beyond, as k_jam_pack
    JPK_LAUNCH(ctx, PROF_JAM, total, k_jam_splice, dim3((unsigned)grid), dim3(PACK_TB), d_frames, n, d_out, total, in_lo, in_hi);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

uint32_t jpk_jam_scan_tiles(const uint8_t *d_in, int64_t start, int64_t end)
{
    const int64_t lead = (int64_t)((uintptr_t)d_in & 15u);
    const int64_t words = ((lead + end + 15) >> 4) - ((lead + start) >> 4);
    return (uint32_t)((words * 16 + SCAN_TILE - 1) / SCAN_TILE);
}

static unsigned scan_grid(uint32_t ntiles)
{
    const uint32_t blocks = (ntiles + SCAN_TB / 64 - 1) / (SCAN_TB / 64);
    return blocks > 2048u ? 2048u : blocks;                                        // waves stride over the tiles beyond
}

int jpk_jam_scan_count_enqueue(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int64_t start, int64_t end, bool staged_ok, uint32_t *d_counts)
{
    const uint32_t ntiles = jpk_jam_scan_tiles(d_in, start, end);
    JPK_LAUNCH(ctx, PROF_JAM_SCAN, end - start, k_jam_scan_count, dim3(scan_grid(ntiles)), dim3(SCAN_TB), d_in, in_len, start, end, staged_ok ? 1u : 0u, ntiles,
               d_counts);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

int jpk_jam_scan_emit_enqueue(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int64_t start, int64_t end, bool staged_ok, uint32_t *d_counts,
                              JamWalkFrame *d_out, uint32_t max_cands)
{
    const uint32_t ntiles = jpk_jam_scan_tiles(d_in, start, end);
    JPK_LAUNCH(ctx, PROF_JAM_SCAN, 0, k_jam_scan_emit, dim3(scan_grid(ntiles)), dim3(SCAN_TB), d_in, in_len, start, end, staged_ok ? 1u : 0u, ntiles, d_counts,
               d_out, max_cands);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}
