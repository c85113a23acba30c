// ans_enc_front.hip -- rANS encoder, the front: sorted-rank coding (rank.cpp:45-90) and RLE0 (rle.cpp:22-47) of every chunk (overview:
// ans_enc.hip).  One unit for both stages: the RLE0 half alone is under 200 lines.
#include "ans_enc.hpp"

using namespace jpk;
using namespace jpk_enc;

namespace {

// ---------------------------------------------------------------------------------------------------------------
// rank coding
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void k_enc_hist(const uint8_t *__restrict__ in, EncDims d, uint32_t *__restrict__ tilecnt,
                                                int32_t *__restrict__ lastpos)
{
    const uint32_t c = chunk_of(d, blockIdx.y), t = blockIdx.x;
    const uint32_t clen = chunk_len(d, c), ts = t * ATILE;
    if (ts >= clen) return;
    __shared__ uint32_t h[TB / 64][256];
    __shared__ int32_t lp[TB / 64][256];
#pragma unroll
    for (int k = 0; k < TB / 64; k++) { h[k][threadIdx.x] = 0; lp[k][threadIdx.x] = -1; }
    __syncthreads();
    const uint8_t *src = in + (size_t)c * d.chunk;
    uint8_t sy[ATILE / TB];
#pragma unroll
    for (int it = 0; it < ATILE / TB; it++) {          // the tile's loads in flight together (clamped; masked below)
        const uint32_t i = ts + it * TB + threadIdx.x;
        sy[it] = src[i < clen ? i : clen - 1];
    }
    // The input is a BWT image: runs of equal bytes, so most lanes of a wave hit the same bin.  Counted by wave match (ballots; the
    // first lane of each set of equal bytes adds their number and records the position of the set's LAST lane -- positions grow
    // with the lane and with the iteration, so a plain store keeps the maximum) on per-wave tables, no LDS atomics.
    const int w = threadIdx.x >> 6;
    const uint64_t lt = lanemask_lt();
#pragma unroll
    for (int it = 0; it < ATILE / TB; it++) {
        const uint32_t i = ts + it * TB + threadIdx.x;
        const bool valid = i < clen;
        const uint32_t s = sy[it];
        const uint64_t m = match_any8(s, valid);
        if (valid && (m & lt) == 0ull) {
            h[w][s] += (uint32_t)__popcll(m);
            lp[w][s] = (int32_t)(i - (uint32_t)lane_id() + (63u - (uint32_t)__clzll((long long)m)));
        }
    }
    __syncthreads();
    size_t o = ((size_t)c * d.tpc + t) * 256 + threadIdx.x;
    uint32_t hs = 0;
    int32_t lm = -1;
#pragma unroll
    for (int k = 0; k < TB / 64; k++) { hs += h[k][threadIdx.x]; lm = lp[k][threadIdx.x] > lm ? lp[k][threadIdx.x] : lm; }
    tilecnt[o] = hs;
    lastpos[o] = lm;
}

// per chunk: Freq[], per-tile prefix counts, carried last-occurrence table, bucket starts in the order of
// GenerateSortedMap (rank.cpp:15-39: descending frequency, ties -> smaller symbol first)
__global__ __launch_bounds__(256) void k_enc_prep(EncDims d, uint32_t *__restrict__ tilecnt, int32_t *__restrict__ lastpos,
                                                 int32_t *__restrict__ freq, uint32_t *__restrict__ bstart)
{
    const uint32_t c = chunk_of(d, blockIdx.x), s = threadIdx.x;
    const uint32_t clen = chunk_len(d, c);
    const uint32_t nt = (clen + ATILE - 1) / ATILE;
    uint32_t f = 0;
    int32_t p = -1;
    for (uint32_t t = 0; t < nt; t++) {
        size_t o = ((size_t)c * d.tpc + t) * 256 + s;
        uint32_t n = tilecnt[o];
        tilecnt[o] = f;
        f += n;
        int32_t l = lastpos[o];
        lastpos[o] = p;
        p = l > p ? l : p;
    }
    __shared__ uint32_t sf[256];
    sf[s] = f;
    freq[(size_t)c * 256 + s] = (int32_t)f;
    __syncthreads();
    uint32_t b = 0;
    for (uint32_t k = 0; k < 256; k++) {
        uint32_t fk = sf[k];
        if (fk > f || (fk == f && k < s)) b += fk;
    }
    bstart[(size_t)c * 256 + s] = b;
}

// one wave per tile: wave-sequential MTF on the recency list itself + bucket scatter (rank.cpp:69-87).
// The list lives in 4 registers per lane: lane p of lst_j holds the symbol at list position 64 j + p (0xFFFF behind the symbols seen
// so far in the chunk: a symbol's first occurrence has rank = number of distinct symbols before it, i.e. it sits at the first free
// position).  A head's rank is its position -- one v_cmp + s_ff1 when it is among the first 64, which is nearly every head of a BWT
// image -- and the move to front is one DPP wave_shr:1 under a lane mask (positions below it move down by one, the symbol enters at
// lane 0).  Positions 64.. are searched, and the shift carried from register to register, only when the first compare misses.  The
// list at the start of the tile is rebuilt from the carried last-occurrence stamps: position = number of symbols with a later stamp.
// Only run HEADS are walked serially (a repeat has rank 0, leaves the list unchanged and lands right behind its head in the same
// bucket): a ballot marks them in each 64-byte group, the loop visits the set bits, and every lane then derives its own
// (destination, rank) from the record of the head at or before it.  All loop control is wave-uniform (scalar branches, no exec-mask
// loops): the wave index is read with readfirstlane.  A per-wave LDS table holds the bucket write positions (wave-uniform accesses).
__device__ __forceinline__ uint32_t mtf_shr1(uint32_t carry_in, uint32_t v)          // lane i <- lane i - 1, lane 0 <- carry_in
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)carry_in, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

__global__ __launch_bounds__(TB) void k_enc_mtf(const uint8_t *__restrict__ in, EncDims d, const uint32_t *__restrict__ tilebase,
                                               const int32_t *__restrict__ prevlast, const uint32_t *__restrict__ bstart,
                                               uint8_t *__restrict__ ranks)
{
    struct WaveLds {                       // one per wave; neighbours in one struct so that pairs of accesses share an address register
        uint32_t pos[256];                 // next write position of every symbol's bucket
        uint32_t dst[64], rk[64];          // (bucket position, rank) of the heads of the group in flight
        uint32_t lst[256];                 // the list at the start of the tile, while it is built
    };
    __shared__ WaveLds s_w[TB / 64];
    const uint32_t c = chunk_of(d, blockIdx.y);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t t = blockIdx.x * (TB / 64) + (uint32_t)w;
    const uint32_t clen = chunk_len(d, c), ts = t * ATILE;
    if (ts >= clen) return;
    const int l = lane_id();
    const size_t o = ((size_t)c * d.tpc + t) * 256;
    const int32_t last0 = prevlast[o + l], last1 = prevlast[o + 64 + l], last2 = prevlast[o + 128 + l], last3 = prevlast[o + 192 + l];
    const uint32_t *bs = bstart + (size_t)c * 256;
    WaveLds &L = s_w[w];
    const uint8_t *src = in + (size_t)c * d.chunk;
    uint8_t *dst = ranks + (size_t)c * d.chunk;
    const uint32_t te = (ts + ATILE < clen) ? ts + ATILE : clen;
    uint32_t bn = ((uint32_t)l < te - ts) ? src[ts + l] : 0x100u;             // group in flight
#pragma unroll
    for (int qq = 0; qq < 4; qq++) {
        L.pos[qq * 64 + l] = bs[qq * 64 + l] + tilebase[o + qq * 64 + l];
        L.lst[qq * 64 + l] = 0xFFFFu;
    }
    // the list before the tile: every symbol seen so far goes to position #{symbols with a later stamp} (stamps are positions: distinct)
    uint32_t nseen = 0;
#define JPK_MTF_PLACE(LASTJ, J)                                                                                                   \
    {                                                                                                                             \
        uint64_t sm = __ballot(LASTJ >= 0);                                                                                       \
        nseen += (uint32_t)__popcll(sm);                                                                                          \
        while (sm) {                                                                                                              \
            const uint32_t ln = (uint32_t)__builtin_ctzll(sm);                                                                    \
            sm &= sm - 1;                                                                                                         \
            const int32_t own = __builtin_amdgcn_readlane(LASTJ, (int)ln);                                                        \
            const uint32_t at = (uint32_t)__popcll(__ballot(last0 > own)) + (uint32_t)__popcll(__ballot(last1 > own)) +           \
                                (uint32_t)__popcll(__ballot(last2 > own)) + (uint32_t)__popcll(__ballot(last3 > own));            \
            L.lst[at] = (uint32_t)(J) * 64u + ln;                              /* every lane stores the same value */              \
        }                                                                                                                         \
    }
    JPK_MTF_PLACE(last0, 0)
    JPK_MTF_PLACE(last1, 1)
    JPK_MTF_PLACE(last2, 2)
    JPK_MTF_PLACE(last3, 3)
#undef JPK_MTF_PLACE
    uint32_t lst0 = L.lst[l], lst1 = L.lst[64 + l], lst2 = L.lst[128 + l], lst3 = L.lst[192 + l];
    uint32_t prevc = 256;                                                     // no byte before the tile: its first byte is a head
    for (uint32_t i0 = ts; i0 < te; i0 += 64) {
        const uint32_t nvalid = (te - i0 < 64u) ? te - i0 : 64u;
        const uint32_t b = bn;
        if (i0 + 64 < te) bn = (i0 + 64 + (uint32_t)l < te) ? src[i0 + 64 + l] : 0x100u;      // next group, loaded under this one's walk
        // byte before mine (lane 0: the last byte of the previous group)
        uint32_t pb = (uint32_t)__builtin_amdgcn_update_dpp((int)prevc, (int)b, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        uint64_t rem = __ballot((uint32_t)l < nvalid && (b != pb || l == 0));     // lane 0 is always walked: a repeat gets rank 0 there
        const uint64_t heads = rem;
        // length of the run that starts at my lane (used by head lanes only): distance to the next head, or to the end of the group
        const uint64_t above = (heads >> 1) >> l;
        const uint32_t runlen = above ? (uint32_t)__builtin_ctzll(above) + 1u : nvalid - (uint32_t)l;
        while (rem) {
            const uint32_t k = (uint32_t)__builtin_ctzll(rem);
            rem &= rem - 1;
            const uint32_t cc = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)k);
            const uint32_t run = (uint32_t)__builtin_amdgcn_readlane((int)runlen, (int)k);
            const uint32_t dpos = L.pos[cc];
            const uint64_t m0 = __ballot(lst0 == cc);
            uint32_t rank;
            if (m0) {                                          // among the first 64: the common case
                rank = (uint32_t)__builtin_ctzll(m0);
            } else {                                           // search the rest; shift the registers behind the first here
                const uint64_t m1 = __ballot(lst1 == cc), m2 = __ballot(lst2 == cc), m3 = __ballot(lst3 == cc);
                if (m1) rank = 64u + (uint32_t)__builtin_ctzll(m1);
                else if (m2) rank = 128u + (uint32_t)__builtin_ctzll(m2);
                else if (m3) rank = 192u + (uint32_t)__builtin_ctzll(m3);
                else rank = nseen++;                           // first occurrence in the chunk: enters from the first free position
                const uint32_t j = rank >> 6, q = rank & 63u;
                const bool part = (uint32_t)l <= q;            // lanes that move in the register holding the position
                if (j >= 1) {
                    const uint32_t c1 = (uint32_t)__builtin_amdgcn_readlane((int)lst0, 63);
                    if (j == 1) {
                        const uint32_t sh = mtf_shr1(c1, lst1);
                        lst1 = part ? sh : lst1;
                    } else {
                        const uint32_t c2 = (uint32_t)__builtin_amdgcn_readlane((int)lst1, 63);
                        lst1 = mtf_shr1(c1, lst1);
                        if (j == 2) {
                            const uint32_t sh = mtf_shr1(c2, lst2);
                            lst2 = part ? sh : lst2;
                        } else {
                            const uint32_t c3 = (uint32_t)__builtin_amdgcn_readlane((int)lst2, 63);
                            lst2 = mtf_shr1(c2, lst2);
                            const uint32_t sh = mtf_shr1(c3, lst3);
                            lst3 = part ? sh : lst3;
                        }
                    }
                }
            }
            {                                                  // first register: positions 0 .. min(rank, 63) move down, the symbol enters at 0
                const uint32_t sh = mtf_shr1(cc, lst0);
                lst0 = ((uint32_t)l <= rank) ? sh : lst0;
            }
            L.pos[cc] = dpos + run;
            L.dst[k] = dpos;
            L.rk[k] = rank;
        }
        prevc = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)(nvalid - 1u));
        if ((uint32_t)l < nvalid) {
            const uint32_t hl = 63u - (uint32_t)__builtin_clzll(heads & ((2ull << l) - 1ull));     // my head (bit 0 is always set)
            const uint32_t dp = L.dst[hl] + ((uint32_t)l - hl);
            dst[dp] = ((uint32_t)l == hl) ? (uint8_t)L.rk[hl] : (uint8_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// RLE0 (rle.cpp:22-47)
// ---------------------------------------------------------------------------------------------------------------
// leading zeros of every tile of the rank array
__global__ __launch_bounds__(TB) void k_rle_lz(const uint8_t *__restrict__ ranks, EncDims d, uint32_t *__restrict__ lz)
{
    const uint32_t c = chunk_of(d, blockIdx.y), t = blockIdx.x;
    const uint32_t clen = chunk_len(d, c), ts = t * ATILE;
    if (ts >= clen) return;
    const uint32_t tl = (clen - ts < (uint32_t)ATILE) ? clen - ts : (uint32_t)ATILE;
    const uint8_t *src = ranks + (size_t)c * d.chunk + ts;
    uint32_t first = 0xFFFFFFFFu;
    uint8_t rv[ATILE / TB];
#pragma unroll
    for (int k = 0; k < ATILE / TB; k++) {            // loads first (clamped), all in flight
        const uint32_t p = k * TB + threadIdx.x;
        rv[k] = src[p < tl ? p : tl - 1];
    }
#pragma unroll
    for (int k = ATILE / TB - 1; k >= 0; k--) {
        uint32_t p = k * TB + threadIdx.x;
        if (p < tl && rv[k] != 0) first = p;
    }
    __shared__ uint32_t sm[TB / 64 + 1];
    uint32_t tot;
    block_incl_scan<OpMin>(first, sm, &tot);
    if (threadIdx.x == 0) lz[(size_t)c * d.tpc + t] = tot < tl ? tot : tl;
}

// ext[t] = zeros that follow the end of tile t without interruption (within the chunk)
__global__ void k_rle_ext(EncDims d, const uint32_t *__restrict__ lz, uint32_t *__restrict__ ext)
{
    const uint32_t ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= d.ncl) return;
    const uint32_t c = chunk_of(d, ci);
    const uint32_t clen = chunk_len(d, c);
    const uint32_t nt = (clen + ATILE - 1) / ATILE;
    uint32_t e = 0;
    for (int t = (int)nt - 1; t >= 0; t--) {
        ext[(size_t)c * d.tpc + t] = e;
        uint32_t tl = (clen - t * ATILE < (uint32_t)ATILE) ? clen - t * ATILE : (uint32_t)ATILE;
        uint32_t z = lz[(size_t)c * d.tpc + t];
        e = (z == tl) ? z + e : z;
    }
}

// EMIT=false: symbols per tile -> tcount ; EMIT=true: write symbols at toff[tile]
template <bool EMIT>
__global__ __launch_bounds__(TB) void k_rle_tiles(const uint8_t *__restrict__ ranks, EncDims d, const uint32_t *__restrict__ ext,
                                                 uint32_t *__restrict__ tcount, const uint32_t *__restrict__ toff, uint16_t *__restrict__ rle,
                                                 size_t rle_stride)
{
    const uint32_t c = chunk_of(d, blockIdx.y), t = blockIdx.x;
    const uint32_t clen = chunk_len(d, c), ts = t * ATILE;
    if (ts >= clen) return;
    const uint32_t tl = (clen - ts < (uint32_t)ATILE) ? clen - ts : (uint32_t)ATILE;
    const uint8_t *src = ranks + (size_t)c * d.chunk + ts;
    const uint32_t p0 = threadIdx.x * 16;
    uint8_t v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = (p0 + k < tl) ? src[p0 + k] : (uint8_t)1;
    uint32_t first = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 15; k >= 0; k--)
        if (p0 + k < tl && v[k] != 0) first = p0 + k;
    // exclusive suffix-min over threads of `first`
    __shared__ uint32_t fz[TB];
    __shared__ uint32_t res[TB];
    __shared__ uint32_t sm[TB / 64 + 1];
    fz[threadIdx.x] = first;
    __syncthreads();
    uint32_t rv = fz[TB - 1 - threadIdx.x];
    uint32_t inc = block_incl_scan<OpMin>(rv, sm, nullptr);
    res[threadIdx.x] = inc;
    __syncthreads();
    uint32_t after = (threadIdx.x == TB - 1) ? 0xFFFFFFFFu : res[TB - 2 - threadIdx.x];
    if (after == 0xFFFFFFFFu) after = tl + ext[(size_t)c * d.tpc + t];
    // next non-zero position for every zero of my segment
    uint32_t nxt[16];
    uint32_t nn = after;
#pragma unroll
    for (int k = 15; k >= 0; k--) {
        nxt[k] = nn;
        if (p0 + k < tl && v[k] != 0) nn = p0 + k;
    }
    uint32_t prev;
    if (p0 == 0) prev = (ts == 0) ? 1u : src[-1];
    else prev = (p0 - 1 < tl) ? src[p0 - 1] : 1u;
    uint32_t cnt = 0;
    uint32_t pv = prev;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (p0 + k < tl) {
            if (v[k] != 0) cnt += 1;
            else if (pv != 0) {
                uint32_t L = nxt[k] - (p0 + k) + 1;
                cnt += 31 - __clz((int)L);
            }
            pv = v[k];
        }
    }
    uint32_t tot;
    uint32_t incl = block_incl_scan<OpSum>(cnt, sm, &tot);
    if (!EMIT) {
        if (threadIdx.x == 0) tcount[(size_t)c * d.tpc + t] = tot;
        return;
    }
    uint16_t *out = rle + (size_t)c * rle_stride + toff[(size_t)c * d.tpc + t] + (incl - cnt);
    pv = prev;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (p0 + k < tl) {
            if (v[k] != 0) *out++ = (uint16_t)(v[k] + 1);
            else if (pv != 0) {
                uint32_t L = nxt[k] - (p0 + k) + 1;
                for (int b = 30 - __clz((int)L); b >= 0; b--) *out++ = (uint16_t)((L >> b) & 1u);
            }
            pv = v[k];
        }
    }
}

// serial prefix over the tiles of each chunk (<= 256 tiles in the ANS path)
__global__ void k_tile_prefix(EncDims d, const uint32_t *__restrict__ tcount, uint32_t *__restrict__ toff, uint32_t *__restrict__ total,
                              uint32_t unit_from_len /*1: tiles from chunk_len, 0: tiles from total_in*/, const uint32_t *__restrict__ count_in)
{
    const uint32_t ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= d.ncl) return;
    const uint32_t c = chunk_of(d, ci);
    const uint32_t n = unit_from_len ? chunk_len(d, c) : count_in[c];
    const uint32_t nt = (n + ATILE - 1) / ATILE;
    uint32_t s = 0;
    for (uint32_t t = 0; t < nt; t++) {
        uint32_t v = tcount[(size_t)c * d.tpc + t];
        toff[(size_t)c * d.tpc + t] = s;
        s += v;
    }
    total[c] = s;
}

}  // namespace

namespace jpk_enc {

int run_rank(jpk_ctx *ctx, const uint8_t *d_in, const EncDims &d, EncBufs &b)
{
    JPK_LAUNCH(ctx, PROF_ENC_HIST, d.len, k_enc_hist, dim3(d.tpc, d.ncl), dim3(TB), d_in, d, b.tilecnt, b.lastpos);
    JPK_LAUNCH(ctx, PROF_ENC_HIST, d.len, k_enc_prep, dim3(d.ncl), dim3(256), d, b.tilecnt, b.lastpos, b.freq, b.bstart);
    JPK_LAUNCH(ctx, PROF_ENC_MTF, d.len, k_enc_mtf, dim3((d.tpc + 3) / 4, d.ncl), dim3(TB), d_in, d, b.tilecnt, b.lastpos, b.bstart, b.ranks);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

int run_rle(jpk_ctx *ctx, const uint8_t *d_ranks, const EncDims &d, EncBufs &b)
{
    JPK_LAUNCH(ctx, PROF_ENC_RLE, d.len, k_rle_lz, dim3(d.tpc, d.ncl), dim3(TB), d_ranks, d, b.lz);
    JPK_LAUNCH(ctx, PROF_ENC_RLE, d.len, k_rle_ext, dim3(jpk_grid(d.ncl, 64)), dim3(64), d, b.lz, b.ext);
    JPK_LAUNCH(ctx, PROF_ENC_RLE, d.len, (k_rle_tiles<false>), dim3(d.tpc, d.ncl), dim3(TB), d_ranks, d, b.ext, b.tcount, b.toff, b.rle, (size_t)d.chunk);
    JPK_LAUNCH(ctx, PROF_ENC_RLE, d.len, k_tile_prefix, dim3(jpk_grid(d.ncl, 64)), dim3(64), d, b.tcount, b.toff, b.rlen, 1u, (const uint32_t *)nullptr);
    JPK_LAUNCH(ctx, PROF_ENC_RLE, d.len, (k_rle_tiles<true>), dim3(d.tpc, d.ncl), dim3(TB), d_ranks, d, b.ext, b.tcount, b.toff, b.rle, (size_t)d.chunk);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

}  // namespace jpk_enc
