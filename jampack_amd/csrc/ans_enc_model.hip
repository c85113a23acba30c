// ans_enc_model.hip -- rANS encoder, the models (model.cpp; ans.cpp:152-187): class histograms and ordinals, the QuasiModel tables, and
// the AdaptiveModel recurrences parallel in time (overview: ans_enc.hip).
#include "ans_enc.hpp"

using namespace jpk;
using namespace jpk_enc;

namespace {

// ---------------------------------------------------------------------------------------------------------------
// models (ans.cpp:152-187)
// ---------------------------------------------------------------------------------------------------------------
// class histogram per tile of RLE symbols
__global__ __launch_bounds__(TB) void k_cls_count(const uint16_t *__restrict__ rle, size_t rle_stride, EncDims d, const uint32_t *__restrict__ rlen,
                                                 uint32_t *__restrict__ clscnt)
{
    const uint32_t c = chunk_of(d, blockIdx.y), t = blockIdx.x;
    const uint32_t n = rlen[c], ts = t * ATILE;
    if (ts >= n) return;
    __shared__ uint32_t h[8];
    if (threadIdx.x < 8) h[threadIdx.x] = 0;
    __syncthreads();
    const uint16_t *src = rle + (size_t)c * rle_stride;
    uint32_t loc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint16_t sv[ATILE / TB];
#pragma unroll
    for (int it = 0; it < ATILE / TB; it++) {          // loads first (clamped), all in flight
        const uint32_t i = ts + it * TB + threadIdx.x;
        sv[it] = src[i < n ? i : n - 1];
    }
#pragma unroll
    for (int it = 0; it < ATILE / TB; it++) {
        uint32_t i = ts + it * TB + threadIdx.x;
        if (i < n) {
            int e = sym_class(sv[it]);
#pragma unroll
            for (int k = 0; k < 8; k++) loc[k] += (e == k);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t s = wave_sum(loc[k]);
        if (lane_id() == 0 && s) atomicAdd(&h[k], s);
    }
    __syncthreads();
    if (threadIdx.x < 8) clscnt[((size_t)c * d.tpc + t) * 8 + threadIdx.x] = h[threadIdx.x];
}

__global__ void k_cls_prefix(EncDims d, const uint32_t *__restrict__ rlen, uint32_t *__restrict__ clscnt, uint32_t *__restrict__ clstotal)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = g & 7u;
    if ((g >> 3) >= d.ncl) return;
    const uint32_t c = chunk_of(d, g >> 3);
    const uint32_t nt = (rlen[c] + ATILE - 1) / ATILE;
    uint32_t s = 0;
    for (uint32_t t = 0; t < nt; t++) {
        size_t o = ((size_t)c * d.tpc + t) * 8 + k;
        uint32_t v = clscnt[o];
        clscnt[o] = s;
        s += v;
    }
    clstotal[(size_t)c * 8 + k] = s;
}

// ordinal of every symbol inside its class (stable) + per-interval mantissa histograms of the quasi classes
__global__ __launch_bounds__(TB) void k_cls_ord(const uint16_t *__restrict__ rle, size_t rle_stride, EncDims d, const uint32_t *__restrict__ rlen,
                                               const uint32_t *__restrict__ clsbase, uint32_t *__restrict__ ord, uint32_t *__restrict__ qhist,
                                               uint8_t *__restrict__ cls8, uint32_t *__restrict__ clist)
{
    const uint32_t c = chunk_of(d, blockIdx.y), t = blockIdx.x;
    const uint32_t n = rlen[c], ts = t * ATILE;
    if (ts >= n) return;
    constexpr int W = TB / 64, IT = ATILE / TB;
    __shared__ uint32_t cnt[W][8];
    if (threadIdx.x < W * 8) (&cnt[0][0])[threadIdx.x] = 0;
    __syncthreads();
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint16_t *src = rle + (size_t)c * rle_stride;
    const size_t sb = sym_base(d, c, rle_stride), cs = sym_stride(d, c, rle_stride);
    const uint64_t lt = lanemask_lt();
    uint32_t sy[IT], rk[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) {                  // the tile's loads in flight together (clamped; masked below)
        const uint32_t i = ts + w * (64 * IT) + it * 64 + l;
        sy[it] = src[i < n ? i : n - 1];
    }
#pragma unroll
    for (int it = 0; it < IT; it++) {
        uint32_t i = ts + w * (64 * IT) + it * 64 + l;
        bool valid = i < n;
        uint32_t s = valid ? sy[it] : 0;
        sy[it] = s;
        uint32_t e = (uint32_t)sym_class(s);
        const uint64_t m = match_any<3>(e, valid);
        uint32_t below = (uint32_t)__popcll(m & lt);
        uint32_t cc = valid ? cnt[w][e] : 0;
        rk[it] = cc + below;
        if (valid && below == 0) cnt[w][e] = cc + (uint32_t)__popcll(m);
    }
    __syncthreads();
    // mantissa histograms: the interval in which the tile starts (per class) is accumulated in LDS and flushed once;
    // the few symbols that fall into later intervals go straight to global atomics
    __shared__ uint32_t lh[6][QSTRIDE];
    __shared__ int q0[8];
    for (int i = threadIdx.x; i < 6 * QSTRIDE; i += TB) (&lh[0][0])[i] = 0;
    if (threadIdx.x < 8) {
        uint32_t s = clsbase[((size_t)c * d.tpc + t) * 8 + threadIdx.x];
        q0[threadIdx.x] = qinterval(s);
#pragma unroll
        for (int k = 0; k < W; k++) { uint32_t v = cnt[k][threadIdx.x]; cnt[k][threadIdx.x] = s; s += v; }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; it++) {
        uint32_t i = ts + w * (64 * IT) + it * 64 + l;
        if (i < n) {
            uint32_t s = sy[it];
            int e = sym_class(s);
            uint32_t k = cnt[w][e] + rk[it];
            ord[sb + i] = k;
            cls8[sb + i] = (uint8_t)(e | ((s & 1u) << 3));      // class | mantissa bit of classes 0/1
            if (e < 2) clist[2 * sb + (size_t)e * ((cs + 3) & ~(size_t)3) + k] = i | ((s & 1u) << 31);   // compact list of the class
            else {
                const int q = qinterval(k);
                const uint32_t m = s - (uint32_t)class_base(e);
                if (q == q0[e]) atomicAdd(&lh[e - 2][m], 1u);
                else atomicAdd(&qhist[(((size_t)c * 6 + (e - 2)) * NQ + q) * QSTRIDE + m], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 6 * QSTRIDE; i += TB) {
        const uint32_t v = (&lh[0][0])[i];
        if (v) {
            const int e2 = i / QSTRIDE, m = i % QSTRIDE;
            atomicAdd(&qhist[(((size_t)c * 6 + e2) * NQ + q0[e2 + 2]) * QSTRIDE + m], v);
        }
    }
}

// one wave per (interval, class, chunk): CDF of interval r from the histogram of interval r-1 (model.cpp:160-204)
__global__ __launch_bounds__(64) void k_quasi_build(EncDims d, const uint32_t *__restrict__ clstotal, const uint32_t *__restrict__ qhist,
                                                   uint32_t *__restrict__ qcdf)
{
    const int r = blockIdx.x, e = blockIdx.y + 2;
    const uint32_t c = chunk_of(d, blockIdx.z);
    const int A = class_alpha(e), l = lane_id();
    uint32_t *cdf = qcdf + (((size_t)c * 6 + (e - 2)) * NQ + r) * QSTRIDE;
    if (r == 0) {
        for (int i = l; i <= A; i += 64) cdf[i] = uniform_cdf(A, i);
        return;
    }
    if (clstotal[(size_t)c * 8 + e] < qbound(r)) return;   // this table is never reached
    const uint32_t *h = qhist + (((size_t)c * 6 + (e - 2)) * NQ + (r - 1)) * QSTRIDE;
    uint32_t F[3];
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int i = l + 64 * k;
        F[k] = (i < A) ? 16u * h[i] : 0u;
        tot += F[k];
    }
    tot = wave_sum(tot);
    int lg = 0;
    while ((tot >> lg) + (uint32_t)A > 65536u) lg++;
    uint32_t t2 = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int i = l + 64 * k;
        F[k] = (i < A) ? (F[k] >> lg) + 1u : 0u;
        t2 += F[k];
    }
    t2 = wave_sum(t2);
    uint32_t t3 = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        F[k] = (65536u * F[k]) / t2;      // unsigned 32-bit, as model.cpp:183
        t3 += F[k];
    }
    t3 = wave_sum(t3);
    if (l == 0) F[0] += 65536u - t3;
    uint32_t carry = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int i = l + 64 * k;
        uint32_t inc = wave_incl_sum(F[k]);
        if (i < A) cdf[i] = carry + inc - F[k];
        carry += __shfl(inc, 63, 64);
    }
    if (l == 0) cdf[A] = 65536u;
}

// ---- AdaptiveModel recurrences, parallel in time ---------------------------------------------------------------
// Nine independent scalar recurrences per chunk: exponent model cdf[1..7] (alphabet 8) and cdf[1] of the two
// alphabet-2 mantissa models.  One step is x += (mix - x) >> 5 with mix in {i, i + 65536 - A} (model.cpp:60-77):
// a monotone map that shrinks any interval of states by >= floor(width/32) per update, so after >= ~500 updates
// the set of reachable states is an interval of width <= 31 whatever the history was.
// Item streams: the exponent entries see every symbol (class byte stream cls8); a mantissa model only sees the symbols
// of its class, which k_cls_ord has compacted into a list (position | mantissa bit << 31), so its "time" is the
// class ordinal and a warm-up is always the AD_WARM_DEFAULT list entries in front of the segment.  Per 4096-item segment:
//   A    warm up the two extreme states over the preceding 320 items -> [lo, hi], and walk on into the segment.  lo == hi from the
//        start: the start state is exact, the whole segment is written.  Otherwise both ends walk the segment until they meet (the
//        merge step: a median of 44 items in, 99 % within 180 on text, profiles/adapt_merge_kernel_stats.txt); the step is monotone
//        in the state and the true start state lies in [lo, hi], so once the ends are equal every state between them has reached
//        that value too: the trajectory from the merge step on IS the exact one, and A writes its outputs there and then, with the
//        one state that is left.  It records the end state (the segment's transfer is a constant, flag 3) and how many items at
//        the front it could not write (seg_miss, whole groups of sixteen).  A plateau lane (an entry above every class that occurs,
//        see k_adapt_a) that no symbol of the segment reaches is the identity (flag 2) and is not walked; one that is reached
//        also records the quiet stretch in front of its first reaching symbol (seg_reach).  Ends that never meet: flag 0.
//   tab  flag 0 only (rare: a quiet mantissa run): 32 lanes walk the segment from the 32 candidate start states -> transfer table.
//   B    one lane per (chunk, recurrence) walks the segments in order composing exact start states through end states (flags 1, 3),
//        identities (2) and tables (0).
//   C    writes what A left out from the now exact start state: a constant row over the quiet stretch (16-byte stores), one walk
//        over [seg_reach, seg_miss) -- at most a few hundred items -- and the whole segment only behind a table.
// Every output is produced from an exact state: the result is bit-identical to the sequential reference.
// (Before: A stopped after the warm-up unless lo == hi -- 6 % of the segments of text --, a kernel k_adapt_ext walked every open
// segment with both ends only to learn its end state, and C walked all of it again to write it.  Measured against that scheme on
// one box, profiles/adapt_merge_kernel_stats.txt: one 64 MiB text block alone, k_adapt_* 3.84 -> 2.15 ms (a 0.98 -> 1.25, ext 0.64 ->
// gone, c 1.61 -> 0.27, tab and b as they were); per 100 MB pass of the bench loop, ten blocks in flight, 4.71 -> 3.28 ms (c 2.40 ->
// 0.48) and all kernels together 1752 -> 1652 ms per 23 passes; the bench line 5285 -> 5425 MB/s, median of eight alternating
// pairs, higher in seven of them, profiles/adapt_merge_ab.txt.)
// Warm-up items in front of a segment.  The interval of reachable states contracts by >= floor(width / 32) per item whatever the
// item is (floor is superadditive), so from the full range it is <= 31 wide after 259 items: any warm-up >= 320 keeps the guarantee
// the table of 32 candidates rests on.  Beyond that a longer warm-up only decides how many segments are already a single state
// when the segment starts, and how soon the others merge inside it (a longer warm-up trades against a shorter stretch for k_adapt_c).
// Rounds 1-3 used 1280, which was best for a block ALONE under the old scheme (the five k_adapt_* kernels: 4.3 ms per 64 MiB block
// against 4.9 with 320) -- but the warm-up is pure vector work (two states per item, +62 % on k_adapt_a), and with blocks in
// flight vector issue is what is short: the bench line preferred 320 (4.41 / 4.38 / 4.29 / 4.15 GB/s for 320 / 384 / 512 / 1280 in
// one sequence, 4.22 / 4.13 / 4.11 for 320 / 384 / 1280 interleaved three times; profiles/r04_adapt_warm.txt).
// With the walk-on scheme a longer warm-up also shortens what k_adapt_c re-walks, so 512 was alternated against 320 again: a block
// alone 2.11 against 2.15 ms of k_adapt_*, the bench line 5534 against 5531 MB/s (medians of twelve alternating pairs, 512 ahead in
// six of them, median difference +27 MB/s against a run-to-run yardstick of 98): no difference, 320 stays (profiles/adapt_merge_ab.txt).
constexpr uint32_t AD_WARM_DEFAULT = 320;
static_assert(AD_WARM_DEFAULT % 64 == 0 && AD_WARM_DEFAULT >= 320 && AD_WARM_DEFAULT <= 4096, "whole waves of warm-up items, guarantee above");

struct AdRec {                          // one recurrence
    bool exp;                           // exponent model entry (true) or alphabet-2 mantissa model (false)
    int i;                              // cdf index (exp) / 1
    int cls;                            // class of the mantissa model
    int A;
    __device__ __forceinline__ AdRec(uint32_t rec) : exp(rec < 7), i(rec < 7 ? (int)rec + 1 : 1), cls((int)rec - 7), A(rec < 7 ? 8 : 2) {}
    __device__ __forceinline__ int32_t init() const { return (int32_t)uniform_cdf(A, i); }
    __device__ __forceinline__ int32_t smin() const { return i; }
    __device__ __forceinline__ int32_t smax() const { return i + 65536 - A; }
};

// the item stream of a recurrence inside one chunk
__host__ __device__ __forceinline__ size_t clist_stride(size_t rle_stride) { return (rle_stride + 3) & ~(size_t)3; }   // 16-byte rows

struct AdStream {
    const uint8_t *c8;        // exponent entries: class byte of every symbol
    const uint32_t *list;     // mantissa models: compacted (position | bit << 31) of the class
    uint32_t n;               // items
};
__device__ __forceinline__ AdStream ad_stream(const EncDims &d, const AdRec &r, uint32_t c, const uint8_t *cls8, const uint32_t *clist, size_t rle_stride,
                                              const uint32_t *rlen, const uint32_t *clstotal)
{
    AdStream st;
    const size_t sb = sym_base(d, c, rle_stride), cs = sym_stride(d, c, rle_stride);
    st.c8 = cls8 + sb;
    st.list = r.exp ? nullptr : clist + 2 * sb + (size_t)r.cls * clist_stride(cs);
    st.n = r.exp ? rlen[c] : clstotal[(size_t)c * 8 + r.cls];
    return st;
}

// f(position, coded symbol) for the items [t0, t1) of a stream; 16-byte loads where aligned, the next load is
// issued (unconditionally, clamped) before the current group is consumed
template <class F>
__device__ __forceinline__ void ad_for_each(const AdRec &r, const AdStream &st, uint32_t t0, uint32_t t1, F f)
{
    uint32_t t = t0;
    if (r.exp) {
        const uint8_t *p = st.c8;
        while (t < t1 && (t & 15u)) { f(t, (int)(p[t] & 7u)); t++; }
        // Lanes walk segments 4 KiB apart: every load of a wave touches 64 different lines, and a lane that keeps ONE 16-byte load in
        // flight spends its time waiting for it (the walk ran at ~30 cycles per instruction).  Round 4: a whole 64-byte line per lane
        // and step, the next line requested before the current one is consumed (four loads in flight per lane).
        if (t + 64 <= t1) {
            uint4 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const uint4 *>(p + t + 16 * q);
            for (; t + 64 <= t1; t += 64) {
                const uint32_t tn = (t + 128 <= t1) ? t + 64 : t;
                uint4 nv[4];
#pragma unroll
                for (int q = 0; q < 4; q++) nv[q] = *reinterpret_cast<const uint4 *>(p + tn + 16 * q);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                    for (int k = 0; k < 16; k++) f(t + 16 * q + k, (int)((w[k >> 2] >> (8 * (k & 3))) & 7u));
                }
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = nv[q];
            }
        }
        if (t + 16 <= t1) {
            uint4 v = *reinterpret_cast<const uint4 *>(p + t);
            for (; t + 16 <= t1; t += 16) {
                const uint32_t tn = (t + 32 <= t1) ? t + 16 : t;
                const uint4 nv = *reinterpret_cast<const uint4 *>(p + tn);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++) f(t + k, (int)((w[k >> 2] >> (8 * (k & 3))) & 7u));
                v = nv;
            }
        }
        while (t < t1) { f(t, (int)(p[t] & 7u)); t++; }
    } else {
        const uint32_t *p = st.list;
        while (t < t1 && (t & 3u)) { const uint32_t e = p[t]; f(e & 0x7FFFFFFFu, (int)(e >> 31)); t++; }
        if (t + 16 <= t1) {                                      // (a 64-byte line per step, the next one in flight: see above)
            uint4 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const uint4 *>(p + t + 4 * q);
            for (; t + 16 <= t1; t += 16) {
                const uint32_t tn = (t + 32 <= t1) ? t + 16 : t;
                uint4 nv[4];
#pragma unroll
                for (int q = 0; q < 4; q++) nv[q] = *reinterpret_cast<const uint4 *>(p + tn + 4 * q);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    f(v[q].x & 0x7FFFFFFFu, (int)(v[q].x >> 31));
                    f(v[q].y & 0x7FFFFFFFu, (int)(v[q].y >> 31));
                    f(v[q].z & 0x7FFFFFFFu, (int)(v[q].z >> 31));
                    f(v[q].w & 0x7FFFFFFFu, (int)(v[q].w >> 31));
                }
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = nv[q];
            }
        }
        if (t + 4 <= t1) {
            uint4 v = *reinterpret_cast<const uint4 *>(p + t);
            for (; t + 4 <= t1; t += 4) {
                const uint32_t tn = (t + 8 <= t1) ? t + 4 : t;
                const uint4 nv = *reinterpret_cast<const uint4 *>(p + tn);
                f(v.x & 0x7FFFFFFFu, (int)(v.x >> 31));
                f(v.y & 0x7FFFFFFFu, (int)(v.y >> 31));
                f(v.z & 0x7FFFFFFFu, (int)(v.z >> 31));
                f(v.w & 0x7FFFFFFFu, (int)(v.w >> 31));
                v = nv;
            }
        }
        while (t < t1) { const uint32_t e = p[t]; f(e & 0x7FFFFFFFu, (int)(e >> 31)); t++; }
    }
}

// run one exact trajectory over the items [t0,t1) writing the model outputs (ans.cpp:159-176).
// Exponent entries: the entry's value BEFORE every symbol goes to its own history row hist[t] -- sixteen values per two 16-byte
// stores, no condition and no branch in the loop; k_pairs picks entry e (low) and entry e + 1 (high) of its symbol from the seven
// rows.  (Round 2 stored low / high per symbol from whichever lane matched the symbol's class: two compares, two exec-masked
// 2-byte stores and their branches per symbol and lane -- twelve of the eighteen instructions of the loop.)
__device__ __forceinline__ int32_t ad_run_write(const AdRec &r, const AdStream &st, uint32_t t0, uint32_t t1, int32_t x,
                                                uint16_t *__restrict__ hist, uint32_t *__restrict__ ma)
{
    if (r.exp) {
        const int i = r.i;
        const uint8_t *p = st.c8;
        uint32_t t = t0;
        while (t < t1 && (t & 15u)) { hist[t] = (uint16_t)x; x = adapt_step(x, i, (int)(p[t] & 7u), 8); t++; }
        if (t + 64 <= t1) {                                      // a 64-byte line of class bytes per step, the next one in flight (see ad_for_each)
            uint4 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const uint4 *>(p + t + 16 * q);
            for (; t + 64 <= t1; t += 64) {
                const uint32_t tn = (t + 128 <= t1) ? t + 64 : t;
                uint4 nv[4];
#pragma unroll
                for (int q = 0; q < 4; q++) nv[q] = *reinterpret_cast<const uint4 *>(p + tn + 16 * q);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
                    uint32_t o[8];
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        if (k & 1) o[k >> 1] |= (uint32_t)x << 16;
                        else o[k >> 1] = (uint32_t)x & 0xffffu;
                        x = adapt_step(x, i, (int)((w[k >> 2] >> (8 * (k & 3))) & 7u), 8);
                    }
                    uint4 *qq = reinterpret_cast<uint4 *>(hist + t + 16 * q);
                    qq[0] = make_uint4(o[0], o[1], o[2], o[3]);
                    qq[1] = make_uint4(o[4], o[5], o[6], o[7]);
                }
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = nv[q];
            }
        }
        if (t + 16 <= t1) {
            uint4 v = *reinterpret_cast<const uint4 *>(p + t);
            for (; t + 16 <= t1; t += 16) {
                const uint32_t tn = (t + 32 <= t1) ? t + 16 : t;
                const uint4 nv = *reinterpret_cast<const uint4 *>(p + tn);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t o[8];
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    if (k & 1) o[k >> 1] |= (uint32_t)x << 16;
                    else o[k >> 1] = (uint32_t)x & 0xffffu;
                    x = adapt_step(x, i, (int)((w[k >> 2] >> (8 * (k & 3))) & 7u), 8);
                }
                uint4 *q = reinterpret_cast<uint4 *>(hist + t);
                q[0] = make_uint4(o[0], o[1], o[2], o[3]);
                q[1] = make_uint4(o[4], o[5], o[6], o[7]);
                v = nv;
            }
        }
        while (t < t1) { hist[t] = (uint16_t)x; x = adapt_step(x, i, (int)(p[t] & 7u), 8); t++; }
    } else {
        ad_for_each(r, st, t0, t1, [&](uint32_t t, int m) {
            const uint32_t l0 = m ? (uint32_t)x : 0u, fr = m ? 65536u - (uint32_t)x : (uint32_t)x;
            ma[t] = l0 | (fr << 16);
            x = adapt_step(x, 1, m, 2);
        });
    }
    return x;
}

struct AdArgs {
    const uint8_t *cls8; const uint32_t *clist; size_t rle_stride; const uint32_t *rlen; const uint32_t *clstotal;
    const uint32_t *clsbase;                // [chunk][tile][8]: symbols of every class in front of the tile (k_cls_prefix)
    uint16_t *exph; uint32_t *mantad;       // exph: [chunk][7 exponent entries][rle_stride] history of every entry
    uint32_t warm;                          // warm-up items in front of a segment (AD_WARM_DEFAULT)
    uint32_t *seg_flag; int32_t *seg_lo, *seg_end, *seg_start; uint16_t *seg_tab;
    uint16_t *seg_miss, *seg_reach;         // per segment: items from its start whose outputs k_adapt_c still owes; of those, items in front of the first symbol that moves a plateau lane
};

// lanes = 64 consecutive segments of ONE recurrence (grid y): the exponent / mantissa code paths and the item widths differ, a wave
// that mixed recurrences would walk both paths one after the other with half its lanes off.
// One walk per segment: the warm-up with the two extreme states, then on into the segment itself -- with both ends while any lane
// of the wave is still open (wave-uniform control, one ballot per 64 class bytes / 16 list entries), then ad_run_write with the one
// state that is left.  A lane that is a single state when a group of sixteen items starts stores that group's outputs; the groups
// in front of it are what seg_miss counts and k_adapt_c writes.
__global__ __launch_bounds__(64) void k_adapt_a(EncDims d, AdArgs a)
{
    const uint32_t c = chunk_of(d, blockIdx.z), rec = blockIdx.y;
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    const AdRec r(rec);
    const AdStream st = ad_stream(d, r, c, a.cls8, a.clist, a.rle_stride, a.rlen, a.clstotal);
    const uint32_t nt = (st.n + ATILE - 1) / ATILE;
    const bool valid = k < nt;                                 // (no early return: the walk below is wave-uniform)
    const uint32_t t0 = valid ? k * ATILE : 0u, t1 = !valid ? 0u : (t0 + ATILE < st.n) ? t0 + ATILE : st.n;
    const uint32_t len = t1 - t0;
    const int i = r.i, A = r.A;
    int32_t lo = r.init(), hi = lo;
    if (valid && k != 0) {
        lo = r.smin(); hi = r.smax();
        ad_for_each(r, st, t0 - a.warm, t0, [&](uint32_t, int sy) { lo = adapt_step(lo, i, sy, A); hi = adapt_step(hi, i, sy, A); });
    }
    const size_t so = ((size_t)c * 9 + rec) * d.tpc + k;
    const int32_t lo0 = lo, hi0 = hi;
    // An open lane is usually an exponent entry above every class that occurs (rare large classes): its mix is smax at every step, hi
    // never left smax (one other step would have dropped it for good: nothing climbs back to smax from below), lo stalled at
    // smax - 31, and all 32 states in between are fixed points of that step -- a plateau lane.  If no symbol of the segment reaches
    // the entry either, the segment's transfer is the identity and its history row a constant: no walk at all (flag 2).  Otherwise
    // nothing moves before the first symbol that does reach it: seg_reach = the whole groups of sixteen in front of that symbol.
    const bool plat = valid && r.exp && lo != hi && hi == r.smax() && lo == r.smax() - 31;
    bool ident = false;
    if (plat) {
        const uint32_t *cb = a.clsbase + ((size_t)c * d.tpc + k) * 8;
        uint32_t reach = 0;                                    // symbols of the segment with class >= i
        for (int e = r.i; e < 8; e++) reach += ((k + 1 < nt) ? cb[8 + e] : a.clstotal[(size_t)c * 8 + e]) - cb[e];
        ident = reach == 0;
    }
    const bool walk = valid && !ident;
    bool open = walk && lo != hi, quiet = plat;
    uint32_t miss = 0, fr = 0, u = 0;                          // u: items of the segment done, the same in every lane that walks
    uint16_t *hist = a.exph + 7 * sym_base(d, c, a.rle_stride) + (size_t)(rec < 7 ? rec : 0) * sym_stride(d, c, a.rle_stride);
    uint32_t *ma = a.mantad + sym_base(d, c, a.rle_stride);
    if (r.exp) {
        const uint8_t *p = st.c8 + t0;
        const int32_t top = r.smax();
        uint4 v[4];
        if (__ballot(open && 64u <= len)) {
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const uint4 *>(p + ((walk && 64u <= len) ? 16 * q : 0));
        }
        while (__ballot(open && u + 64 <= len)) {
            const bool in = walk && u + 64 <= len;             // lanes whose segment has ended sit the rest out
            const uint32_t un = (in && u + 128 <= len) ? u + 64 : (in ? u : 0u);
            uint4 nv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) nv[q] = *reinterpret_cast<const uint4 *>(p + un + 16 * q);
            if (in) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
                    const bool one = lo == hi;
                    uint32_t o[8];
#pragma unroll
                    for (int j = 0; j < 16; j++) {
                        if (j & 1) o[j >> 1] |= (uint32_t)lo << 16;
                        else o[j >> 1] = (uint32_t)lo & 0xffffu;
                        const int sy = (int)((w[j >> 2] >> (8 * (j & 3))) & 7u);
                        lo = adapt_step(lo, i, sy, 8);
                        hi = adapt_step(hi, i, sy, 8);
                    }
                    if (one) {
                        uint4 *qq = reinterpret_cast<uint4 *>(hist + t0 + u + 16 * q);
                        qq[0] = make_uint4(o[0], o[1], o[2], o[3]);
                        qq[1] = make_uint4(o[4], o[5], o[6], o[7]);
                    }
                    if (quiet) { if (hi == top) fr = u + 16 * q + 16; else quiet = false; }
                    if (open && lo == hi) { open = false; miss = u + 16 * q + 16; }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = nv[q];
            u += 64;
        }
        if (walk && u > (len & ~63u)) u = len & ~63u;
    } else {
        const uint32_t *p = st.list + t0;
        uint4 v[4];
        if (__ballot(open && 16u <= len)) {
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const uint4 *>(p + ((walk && 16u <= len) ? 4 * q : 0));
        }
        while (__ballot(open && u + 16 <= len)) {
            const bool in = walk && u + 16 <= len;
            const uint32_t un = (in && u + 32 <= len) ? u + 16 : (in ? u : 0u);
            uint4 nv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) nv[q] = *reinterpret_cast<const uint4 *>(p + un + 4 * q);
            if (in) {
                const bool one = lo == hi;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int m = (int)(w[j] >> 31);
                        if (one) {
                            const uint32_t l0 = m ? (uint32_t)lo : 0u, f = m ? 65536u - (uint32_t)lo : (uint32_t)lo;
                            ma[w[j] & 0x7FFFFFFFu] = l0 | (f << 16);
                        }
                        lo = adapt_step(lo, 1, m, 2);
                        hi = adapt_step(hi, 1, m, 2);
                    }
                }
                if (open && lo == hi) { open = false; miss = u + 16; }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = nv[q];
            u += 16;
        }
        if (walk && u > (len & ~15u)) u = len & ~15u;
    }
    if (!valid) return;
    if (ident) {
        a.seg_flag[so] = 2u;
        return;
    }
    if (open) {
        // less than one group left and still two states (the last segment of a stream): the ends may yet meet, but then the whole
        // segment is k_adapt_c's
        ad_for_each(r, st, t0 + u, t1, [&](uint32_t, int sy) { lo = adapt_step(lo, i, sy, A); hi = adapt_step(hi, i, sy, A); });
        a.seg_miss[so] = (uint16_t)len;
        a.seg_reach[so] = (uint16_t)fr;
        if (lo == hi) { a.seg_flag[so] = 3u; a.seg_end[so] = lo; }
        else { a.seg_flag[so] = 0u; a.seg_lo[so] = lo0; a.seg_end[so] = hi0; }      // k_adapt_tab: the 32 candidates lo0 .. lo0 + 31
        return;
    }
    a.seg_flag[so] = miss ? 3u : 1u;
    a.seg_miss[so] = (uint16_t)miss;
    a.seg_reach[so] = (uint16_t)fr;
    a.seg_end[so] = ad_run_write(r, st, t0 + u, t1, lo, hist, ma);
}

// transfer table of a segment that is still unresolved: 32 lanes = 32 candidate start states walk the segment together (the
// item loads are wave-uniform), instead of one lane walking it 32 times
__global__ __launch_bounds__(64) void k_adapt_tab(EncDims d, AdArgs a)
{
    const uint32_t c = chunk_of(d, blockIdx.z), rec = blockIdx.y;
    const uint32_t k = blockIdx.x * 2 + (threadIdx.x >> 5);
    const int q = threadIdx.x & 31;
    const AdRec r(rec);
    const AdStream st = ad_stream(d, r, c, a.cls8, a.clist, a.rle_stride, a.rlen, a.clstotal);
    const uint32_t nt = (st.n + ATILE - 1) / ATILE;
    if (k >= nt) return;
    const size_t so = ((size_t)c * 9 + rec) * d.tpc + k;
    if (a.seg_flag[so]) return;
    const uint32_t t0 = k * ATILE, t1 = (t0 + ATILE < st.n) ? t0 + ATILE : st.n;
    const int32_t lo = a.seg_lo[so], hi = a.seg_end[so];
    int32_t x = (lo + q < hi) ? lo + q : hi;
    const int i = r.i, A = r.A;
    ad_for_each(r, st, t0, t1, [&](uint32_t, int sy) { x = adapt_step(x, i, sy, A); });
    a.seg_tab[so * 32 + q] = (uint16_t)(x - 1);     // states are in [1, 65535]
}

__global__ __launch_bounds__(64) void k_adapt_b(EncDims d, AdArgs a)
{
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    const uint32_t rec = g & 15u;
    if ((g >> 4) >= d.ncl || rec >= 9) return;
    const uint32_t c = chunk_of(d, g >> 4);
    const AdRec r(rec);
    const AdStream st = ad_stream(d, r, c, a.cls8, a.clist, a.rle_stride, a.rlen, a.clstotal);
    const uint32_t nt = (st.n + ATILE - 1) / ATILE;
    int32_t x = r.init();
    for (uint32_t k = 0; k < nt; k++) {
        const size_t so = ((size_t)c * 9 + rec) * d.tpc + k;
        const uint32_t flag = a.seg_flag[so];
        if (flag == 1u) x = a.seg_end[so];
        else if (flag == 2u) a.seg_start[so] = x;             // identity segment: the state passes through
        else if (flag == 3u) { a.seg_start[so] = x; x = a.seg_end[so]; }      // constant transfer
        else {
            a.seg_start[so] = x;
            int q = x - a.seg_lo[so];
            q = q < 0 ? 0 : (q > 31 ? 31 : q);
            x = (int32_t)a.seg_tab[so * 32 + q] + 1;
        }
    }
}

__global__ __launch_bounds__(64) void k_adapt_c(EncDims d, AdArgs a)
{
    const uint32_t c = chunk_of(d, blockIdx.z), rec = blockIdx.y;
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    const AdRec r(rec);
    const AdStream st = ad_stream(d, r, c, a.cls8, a.clist, a.rle_stride, a.rlen, a.clstotal);
    const uint32_t nt = (st.n + ATILE - 1) / ATILE;
    if (k >= nt) return;
    const size_t so = ((size_t)c * 9 + rec) * d.tpc + k;
    const uint32_t flag = a.seg_flag[so];
    if (flag == 1u) return;
    const uint32_t t0 = k * ATILE, t1 = (t0 + ATILE < st.n) ? t0 + ATILE : st.n;
    // what k_adapt_a left out: [t0, t0 + miss), of which [t0, t0 + fr) is a constant row (an identity segment: all of it; a plateau
    // lane: up to the first symbol that reaches the entry; fr is a multiple of 16 there, and t0 one of ATILE: 16-byte stores)
    const uint32_t miss = flag == 2u ? t1 - t0 : a.seg_miss[so], fr = flag == 2u ? t1 - t0 : a.seg_reach[so];
    uint16_t *hist = a.exph + 7 * sym_base(d, c, a.rle_stride) + (size_t)(rec < 7 ? rec : 0) * sym_stride(d, c, a.rle_stride);
    const int32_t x0 = a.seg_start[so];
    if (fr) {
        const uint32_t x = (uint32_t)x0 & 0xffffu, xx = x | (x << 16);
        uint32_t t = t0;
        for (; t + 8 <= t0 + fr; t += 8) *reinterpret_cast<uint4 *>(hist + t) = make_uint4(xx, xx, xx, xx);
        for (; t < t0 + fr; t++) hist[t] = (uint16_t)x;
    }
    if (fr < miss) ad_run_write(r, st, t0 + fr, t0 + miss, x0, hist, a.mantad + sym_base(d, c, a.rle_stride));
}

}  // namespace

namespace jpk_enc {

int run_model(jpk_ctx *ctx, const uint16_t *d_rle, const uint32_t *d_rlen, const EncDims &d, EncBufs &b)
{
    const size_t stride = d.chunk;
    JPK_LAUNCH(ctx, PROF_ENC_CLASS, 0, k_cls_count, dim3(d.tpc, d.ncl), dim3(TB), d_rle, stride, d, d_rlen, b.clscnt);
    JPK_LAUNCH(ctx, PROF_ENC_CLASS, 0, k_cls_prefix, dim3(jpk_grid((size_t)d.ncl * 8, 64)), dim3(64), d, d_rlen, b.clscnt, b.clstotal);
    JPK_LAUNCH(ctx, PROF_ENC_CLASS, 0, k_cls_ord, dim3(d.tpc, d.ncl), dim3(TB), d_rle, stride, d, d_rlen, b.clscnt, b.ord, b.qhist, b.cls8, b.clist);
    JPK_LAUNCH(ctx, PROF_ENC_CLASS, 0, k_quasi_build, dim3(NQ, 6, d.ncl), dim3(64), d, b.clstotal, b.qhist, b.qcdf);
    AdArgs aa;
    aa.cls8 = b.cls8; aa.clist = b.clist; aa.rle_stride = stride; aa.rlen = d_rlen; aa.clstotal = b.clstotal; aa.clsbase = b.clscnt;
    aa.exph = b.exph; aa.mantad = b.mantad;
    aa.warm = AD_WARM_DEFAULT;
    aa.seg_flag = b.seg_flag; aa.seg_lo = b.seg_lo; aa.seg_end = b.seg_end; aa.seg_start = b.seg_start; aa.seg_tab = b.seg_tab;
    aa.seg_miss = b.seg_miss; aa.seg_reach = b.seg_reach;
    JPK_LAUNCH(ctx, PROF_ENC_ADAPTIVE, 0, k_adapt_a, dim3((d.tpc + 63) / 64, 9, d.ncl), dim3(64), d, aa);
    JPK_LAUNCH(ctx, PROF_ENC_ADAPTIVE, 0, k_adapt_tab, dim3((d.tpc + 1) / 2, 9, d.ncl), dim3(64), d, aa);
    JPK_LAUNCH(ctx, PROF_ENC_ADAPTIVE, 0, k_adapt_b, dim3(jpk_grid((size_t)d.ncl * 16, 64)), dim3(64), d, aa);
    JPK_LAUNCH(ctx, PROF_ENC_ADAPTIVE, 0, k_adapt_c, dim3((d.tpc + 63) / 64, 9, d.ncl), dim3(64), d, aa);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

}  // namespace jpk_enc
