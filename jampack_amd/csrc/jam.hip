// jam.hip -- the frames of a .jam archive on gfx950 (Jampack::Compress / Decompress, jampack.cpp:186-336):
//   k_jam_walk   one wave walks the frame headers of an archive in HBM (DecompReadBlock's checks, jampack.cpp:140-163)
//   k_jam_pack   writes a run of frames -- "JAM" | u32 crc | i32 payload size | i32 BlockSize | payload, little-endian --
//                from payload slots in scratch, organised by destination: a thread owns aligned 16-byte words of the output
//   k_jam_gather delivers the pieces of a range read -- (source, destination, length) of decoded bytes -- organised by destination
//                in the same way: a thread owns aligned 16-byte words of a piece's destination
// The ABI entries that drive them are jpk_dev_jam_compress / jpk_dev_jam_decompress / jpk_dev_jam_read (jam_archive.hip).
#include "common.hpp"

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
        const int32_t bs = (staged_ok && field > 0) ? (field & ~JPK_JAM_STAGED) : field;
        if (h[0] != 'J' || h[1] != 'A' || h[2] != 'M' || bs < JPK_MIN_BLOCKSIZE || bs > JPK_MAX_BLOCKSIZE || psize < 0 || psize > JPK_MAX_BLOCKSIZE ||
            (uint64_t)psize > in_len - o - JPK_JAM_HEADER_BYTES) { bad = 1; break; }
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
