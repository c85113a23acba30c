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

// one wave per tile: the rank of every run head counted in its own window + bucket scatter (rank.cpp:69-87).  No recency list is kept:
// in the index space of the tile's run heads (a repeat has rank 0 and lands right behind its head in the same bucket), with P(k) the
// previous head of head k's symbol and N(j) the next head of head j's symbol,
//     rank(k) = #{ j : P(k) < j < k and N(j) >= k }
// -- every distinct symbol between the two occurrences, counted once at its last head there.  The wave goes over the tile in 64-byte
// groups.  One wave match of the group's bytes gives every byte its bucket position (pos[sym] + equal bytes below it in the group; the
// last lane of each set advances pos[sym]) and every head its P (the nearest equal head below it in the group, else lasth[sym]); the head
// then writes nx[k] = INF and nx[P(k)] = k, so that when a group counts, nx[j] holds N(j) for every j whose N(j) lies at or before
// the group and INF (>= every k) otherwise -- exactly what the compare needs.  The count itself has no running state:
//   * every head tests the RW_CAP = 32 positions right below it from its own lane: one 64-byte LDS read from one address, two slots
//     compared per subtraction.  83 % of the windows of the bench's first block end there (profiles/rank_window_ab.txt: median 6,
//     75 % 20, 90 % 55, 99 % 227 heads);
//   * a head whose window is longer gets the wave for the rest of it: 64 positions per LDS read, compare, ballot and popcount, two
//     such heads at a time so that their reads overlap;
//   * a symbol's FIRST head in the tile has no P in the tile.  Its window is the tile so far -- the number of first heads before it, a
//     counter -- plus what the chunk carried in: the symbols without a head in the tile yet whose stamp (k_enc_prep's last occurrence
//     before the tile) is later than its own.  The four stamp registers are compared as the old tile-start rebuild compared them; a symbol
//     that got its head drops out by taking stamp -2.  At most 256 of these per tile, walked in order.
// A head depends on no head before it: only the two tables (pos, lasth) run along the groups, at a handful of instructions per GROUP.
// LDS: 9.7 KB per wave (nx is sized for a tile of 4096 heads, plus RW_CAP slots in front for the own-lane read of the tile's first heads
// and the 63 positions a last window step reads past its end), 38.75 KB per workgroup of four tiles: four workgroups per CU, 4 waves
// per SIMD (the serial walk had 16).  All loop control is wave-uniform (scalar branches).  tests/rank_window_model.py restates it.
constexpr int RW_CAP = 32;                    // window positions a head tests from its own lane
static_assert(RW_CAP == 32, "the own-lane flags fill one 32-bit word: sixteen dwords of two slots");
constexpr uint32_t RW_NONE = 0x7FFFu;        // lasth: no head of the symbol in the tile yet; nx: no later head of the symbol so far

__global__ __launch_bounds__(TB) void k_enc_mtf(const uint8_t *__restrict__ in, EncDims d, const uint32_t *__restrict__ tilebase,
                                               const int32_t *__restrict__ prevlast, const uint32_t *__restrict__ bstart,
                                               uint8_t *__restrict__ ranks)
{
    struct WaveLds {                       // one per wave
        uint16_t nx[RW_CAP + ATILE + 64];  // N(j) of the tile's heads, as far as the groups walked so far know it; RW_CAP slots in front
        uint16_t lasth[256];               // the last head of every symbol in the tile so far
        uint32_t pos[256];                 // next write position of every symbol's bucket
    };
    __shared__ WaveLds s_w[TB / 64];
    const uint32_t c = chunk_of(d, blockIdx.y);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t t = blockIdx.x * (TB / 64) + (uint32_t)w;
    const uint32_t clen = chunk_len(d, c), ts = t * ATILE;
    if (ts >= clen) return;
    const uint32_t l = (uint32_t)lane_id();
    const uint64_t lt = lanemask_lt();
    const size_t o = ((size_t)c * d.tpc + t) * 256;
    int32_t last0 = prevlast[o + l], last1 = prevlast[o + 64 + l], last2 = prevlast[o + 128 + l], last3 = prevlast[o + 192 + l];
    const uint32_t *bs = bstart + (size_t)c * 256;
    WaveLds &L = s_w[w];
    const uint8_t *src = in + (size_t)c * d.chunk;
    uint8_t *dst = ranks + (size_t)c * d.chunk;
    const uint32_t te = (ts + ATILE < clen) ? ts + ATILE : clen;
    uint32_t bn = (l < te - ts) ? src[ts + l] : 0x100u;                       // group in flight
#pragma unroll
    for (int qq = 0; qq < 4; qq++) {
        L.pos[qq * 64 + l] = bs[qq * 64 + l] + tilebase[o + qq * 64 + l];
        L.lasth[qq * 64 + l] = (uint16_t)RW_NONE;
    }
    uint32_t prevc = 256;                                                     // no byte before the tile: its first byte is a head
    uint32_t hb = 0;                                                          // heads of the tile before the group
    uint32_t nfirst = 0;                                                      // first heads so far = distinct symbols of the tile so far
    for (uint32_t i0 = ts; i0 < te; i0 += 64) {
        const uint32_t nvalid = (te - i0 < 64u) ? te - i0 : 64u;
        const uint32_t b = bn;
        if (i0 + 64 < te) bn = (i0 + 64 + l < te) ? src[i0 + 64 + l] : 0x100u;                // next group, loaded under this one's work
        const bool valid = l < nvalid;
        const uint32_t sy = valid ? b : 0u;                                   // a table index for every lane
        // byte before mine (lane 0: the last byte of the previous group)
        const uint32_t pb = (uint32_t)__builtin_amdgcn_update_dpp((int)prevc, (int)b, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        const uint64_t heads = __ballot(valid && b != pb);
        const bool ishead = (heads >> l) & 1ull;
        const uint64_t m = match_any8(b, valid);                              // the group's bytes equal to mine
        const uint32_t p0 = L.pos[sy], lh = L.lasth[sy];                      // both tables as they stand in front of the group
        // bucket position of every byte, head or repeat: the bytes of its symbol before it
        const uint32_t dp = p0 + (uint32_t)__popcll(m & lt);
        if (valid && ((m >> l) >> 1) == 0ull) L.pos[sy] = dp + 1u;            // the last lane of each set
        // head index, and the previous head of the symbol: in the group, else in the table
        const uint32_t k = hb + (uint32_t)__popcll(heads & lt);
        const uint64_t mh = m & heads;
        const uint64_t below = mh & lt;
        const uint32_t top = 63u - (uint32_t)__clzll((long long)(below | 1ull));              // (lane 0 when there is none: not used then)
        const int32_t pin = (int32_t)(hb + (uint32_t)__popcll(heads & ((1ull << top) - 1ull)));
        const int32_t ptab = (lh == RW_NONE) ? -1 : (int32_t)lh;
        const int32_t P = below ? pin : ptab;
        if (ishead && ((mh >> l) >> 1) == 0ull) L.lasth[sy] = (uint16_t)k;    // the symbol's last head of the group
        uint16_t *const nx = L.nx + RW_CAP;                                   // nx[j], j >= -RW_CAP
        if (ishead) nx[k] = (uint16_t)RW_NONE;
        if (ishead && P >= 0) nx[P] = (uint16_t)k;
        // the window (Pw, k): empty for repeats and for first heads, which are counted below
        const int32_t Pw = (ishead && P >= 0) ? P : (int32_t)k;
        // own lane: positions k - 1 .. k - RW_CAP, all read (one address, 64 bytes), those inside the window counted.
        // Two slots a dword, compared in one subtraction: every slot and k are below 0x8000, so (slot | 0x8000) - k keeps bit 15 exactly
        // where slot >= k and never borrows from the half above.  Dword i's two flags go to bits 15 - i and 31 - i (a rotate and a
        // bit-field insert): four instructions per pair of positions.  Slot e = 0 .. RW_CAP - 1 of the read is position k - RW_CAP + e.
        uint32_t ge = 0;
        {
            uint32_t wd[RW_CAP / 2];
            __builtin_memcpy(wd, L.nx + k, RW_CAP * 2);                       // L.nx + k = nx + (k - RW_CAP); 2-byte aligned
            const uint32_t kk = k | (k << 16);
#pragma unroll
            for (int i = 0; i < RW_CAP / 2; i++) {
                const uint32_t dd = (wd[i] | 0x80008000u) - kk;
                const uint32_t at = 0x80008000u >> i;
                ge = (__builtin_rotateright32(dd, (unsigned)i) & at) | (ge & ~at);
            }
        }
        const uint32_t wl = k - (uint32_t)Pw;                                 // positions k - 1 .. k - (wl - 1); 0: no window
        const uint32_t nown = (wl == 0u) ? 0u : (wl - 1u < (uint32_t)RW_CAP ? wl - 1u : (uint32_t)RW_CAP);
        const uint32_t e0 = (uint32_t)RW_CAP - nown;                          // slots e0 .. RW_CAP - 1 lie inside the window
        const uint32_t inwin = ((1u << (16u - ((e0 + 1u) >> 1))) - 1u) | (((1u << (16u - (e0 >> 1))) - 1u) << 16);
        uint32_t cnt = (uint32_t)__popc(ge & inwin);
        // the rest of a longer window: the wave, 64 positions a step; two heads at a time, so that their first reads overlap
        uint64_t lng = __ballot(wl > (uint32_t)RW_CAP + 1u);
        while (lng) {
            const uint32_t la = (uint32_t)__builtin_ctzll(lng);
            lng &= lng - 1;
            const bool two = lng != 0ull;
            const uint32_t lb = two ? (uint32_t)__builtin_ctzll(lng) : la;
            lng &= lng - 1;
            const uint32_t ka = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)la), kb = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)lb);
            const uint32_t ja = (uint32_t)__builtin_amdgcn_readlane(Pw, (int)la) + 1u, jb = (uint32_t)__builtin_amdgcn_readlane(Pw, (int)lb) + 1u;
            const uint32_t ha = ka - (uint32_t)RW_CAP, hbb = kb - (uint32_t)RW_CAP;            // positions [P + 1, k - RW_CAP) are left
            const uint32_t va = nx[ja + l], vb = nx[jb + l];                  // index < ATILE + 63: inside nx
            uint32_t sa = (uint32_t)__popcll(__ballot((ja + l < ha) & (va >= ka)));
            uint32_t sb = (uint32_t)__popcll(__ballot((jb + l < hbb) & (vb >= kb)));
            for (uint32_t j0 = ja + 64; j0 < ha; j0 += 64) {
                const uint32_t v = nx[j0 + l];
                sa += (uint32_t)__popcll(__ballot((j0 + l < ha) & (v >= ka)));
            }
            for (uint32_t j0 = jb + 64; j0 < hbb; j0 += 64) {
                const uint32_t v = nx[j0 + l];
                sb += (uint32_t)__popcll(__ballot((j0 + l < hbb) & (v >= kb)));
            }
            cnt += (l == la) ? sa : 0u;
            cnt += (two && l == lb) ? sb : 0u;
        }
        uint64_t fh = __ballot(ishead && P < 0);
        while (fh) {                                                          // first heads, in order
            const uint32_t ln = (uint32_t)__builtin_ctzll(fh);
            fh &= fh - 1;
            const uint32_t cc = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)ln);
            const int q = (int)(cc & 63u);
            int32_t own;
            if (cc < 64u) own = __builtin_amdgcn_readlane(last0, q);
            else if (cc < 128u) own = __builtin_amdgcn_readlane(last1, q);
            else if (cc < 192u) own = __builtin_amdgcn_readlane(last2, q);
            else own = __builtin_amdgcn_readlane(last3, q);
            // stamps are positions (distinct), -1 = not seen in the chunk, -2 = has a head in this tile: own >= -1
            const uint32_t carried = (uint32_t)__popcll(__ballot(last0 > own)) + (uint32_t)__popcll(__ballot(last1 > own)) +
                                     (uint32_t)__popcll(__ballot(last2 > own)) + (uint32_t)__popcll(__ballot(last3 > own));
            cnt = (l == ln) ? nfirst + carried : cnt;
            nfirst++;
            const uint32_t me = cc - l;
            last0 = (me == 0u) ? -2 : last0;
            last1 = (me == 64u) ? -2 : last1;
            last2 = (me == 128u) ? -2 : last2;
            last3 = (me == 192u) ? -2 : last3;
        }
        if (valid) dst[dp] = ishead ? (uint8_t)cnt : (uint8_t)0;
        hb += (uint32_t)__popcll(heads);
        prevc = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)(nvalid - 1u));
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
