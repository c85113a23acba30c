// checksum.hip -- Checksum::IntegrityCheck (checksum.cpp:12-36) on gfx950, for the block container
// (Jampack::Comp / Decomp, jampack.cpp:29-60: the crc of the block is taken before the first stage and checked
// after the last one).
//
// The reference keeps four 32-bit lanes S = {3,0,0,0}; every 16-byte round feeds big-endian word k into lane k,
//     S[k] ^= (w + (1 << (S[k] & 7))) * 0x9E3779B1,
// while j + 16 < size; the remaining 1..16 bytes go one at a time into lane 0 the same way, and the result is
// the XOR of the lanes.  A lane is sequential only through the three low bits of its state, and because the
// multiplier is 1 mod 8 those bits evolve as s' = s ^ ((w + (1 << s)) & 7): a map on eight states.  So a run of
// rounds is summarised, per lane, by  (end state, XOR of the injected terms)  for each of the eight possible
// start states, and two summaries compose associatively:  h[s] = g[f[s]],  Xh[s] = Xf[s] ^ Xg[f[s]].
// k_chk_segments summarises 64 rounds per thread and tree-reduces the 64 segments of a workgroup in order;
// k_chk_fold reduces the workgroup summaries the same way, applies the start states {3,0,0,0}, runs the byte
// tail and writes the crc.  One streaming read of the block, no atomics, bit-exact for every length.
// A batch of segments (jpk_checksums_device) is one grid of each: every workgroup finds its segment in a prefix table of the
// segments' workgroup counts, and k_chk_fold runs one workgroup per segment; a single block is the batch of one.
#include <vector>

#include "common.hpp"


namespace {

constexpr int TB = 256;
constexpr int SEG = 64;                    // rounds per thread
constexpr int SEGS = TB / 4;               // segments per workgroup (4 lanes each)
constexpr uint32_t PRIME = 0x9E3779B1u;
constexpr uint32_t IDENT = 0xFAC688u;      // packed identity map: 3 bits per start state, state s -> s

struct Summary {           // one lane over a run of rounds
    uint32_t map;          // 8 x 3 bits: end state for start state s at bits 3s..3s+2
    uint32_t x[8];         // XOR of injected terms for start state s
};

__device__ __forceinline__ void compose(Summary &f, const Summary &g)   // f := f then g
{
    uint32_t m = 0;
    uint32_t nx[8];
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const uint32_t mid = (f.map >> (3 * s)) & 7u;
        uint32_t gx = g.x[0];
#pragma unroll
        for (int t = 1; t < 8; t++) gx = (mid == (uint32_t)t) ? g.x[t] : gx;
        nx[s] = f.x[s] ^ gx;
        m |= ((g.map >> (3 * mid)) & 7u) << (3 * s);
    }
    f.map = m;
#pragma unroll
    for (int s = 0; s < 8; s++) f.x[s] = nx[s];
}

__device__ __forceinline__ uint32_t be_word(const uint8_t *p, bool aligned)
{
    if (aligned) return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(p));
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// ordered tree reduction of `count` (<= SEGS, padded with identities) summaries per lane held in LDS
__device__ __forceinline__ void tree_reduce(Summary (*sm)[4], int seg, int k)
{
    for (int stride = 1; stride < SEGS; stride <<= 1) {
        __syncthreads();
        if ((seg & (2 * stride - 1)) == 0) {
            Summary a = sm[seg][k];
            compose(a, sm[seg + stride][k]);
            sm[seg][k] = a;
        }
    }
    __syncthreads();
}

// One segment of a batch: SEGS * SEG rounds per workgroup, its workgroups at [wg_base, wg_base + nblk) of the grid.
struct ChkSeg {
    const uint8_t *p;
    uint32_t size, rounds;  // bytes; rounds taken while j + 16 < size
    uint32_t wg_base, nblk;
};
// the segment table: `segs` in HBM, or (n == 1, no table to upload) the single segment by value
struct ChkTab {
    const ChkSeg *segs;
    ChkSeg one;
    uint32_t n;
};

__device__ __forceinline__ ChkSeg seg_at(const ChkTab &t, uint32_t i) { return t.segs ? t.segs[i] : t.one; }

// the segment whose workgroups hold grid block `bid`: the last one with wg_base <= bid (segments without rounds own no workgroup)
__device__ __forceinline__ uint32_t seg_of(const ChkTab &t, uint32_t bid)
{
    if (!t.segs) return 0;
    uint32_t lo = 0, hi = t.n;                  // invariant: segs[lo].wg_base <= bid, answer in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t.segs[mid].wg_base <= bid) lo = mid; else hi = mid;
    }
    return lo;
}

// grid x: the workgroups of all segments.  out[block][lane] = summary of the workgroup's rounds of its segment
__global__ __launch_bounds__(TB) void k_chk_segments(ChkTab tab, Summary *__restrict__ out)
{
    __shared__ Summary sm[SEGS][4];
    const int k = threadIdx.x & 3, seg = threadIdx.x >> 2;
    const ChkSeg S = seg_at(tab, seg_of(tab, blockIdx.x));
    const uint8_t *__restrict__ in = S.p;
    const uint32_t rounds = S.rounds;
    const uint32_t r0 = ((uint32_t)(blockIdx.x - S.wg_base) * SEGS + seg) * SEG;
    const bool aligned = ((uintptr_t)in & 3u) == 0;
    uint32_t st[8], x[8];
#pragma unroll
    for (int s = 0; s < 8; s++) { st[s] = s; x[s] = 0; }
    const uint32_t r1 = min(rounds, r0 + SEG);
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t w = be_word(in + (size_t)r * 16 + 4 * k, aligned);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const uint32_t t = (w + (1u << st[s])) * PRIME;
            x[s] ^= t;
            st[s] = (st[s] ^ t) & 7u;
        }
    }
    Summary me;
    me.map = 0;
#pragma unroll
    for (int s = 0; s < 8; s++) { me.map |= st[s] << (3 * s); me.x[s] = x[s]; }
    sm[seg][k] = me;
    tree_reduce(sm, seg, k);
    if (seg == 0) out[(size_t)blockIdx.x * 4 + k] = sm[0][k];
}

// one workgroup per segment: fold its workgroup summaries in order, then the byte tail; crc -> result[segment]
__global__ __launch_bounds__(TB) void k_chk_fold(ChkTab tab, const Summary *__restrict__ part_all, uint32_t *__restrict__ result)
{
    __shared__ Summary sm[SEGS][4];
    __shared__ Summary carry[4];
    const ChkSeg S = seg_at(tab, blockIdx.x);
    const uint8_t *__restrict__ in = S.p;
    const uint32_t size = S.size, rounds = S.rounds, nblk = S.nblk;
    const Summary *__restrict__ part = part_all + (size_t)S.wg_base * 4;
    const int k = threadIdx.x & 3, seg = threadIdx.x >> 2;
    if (seg == 0) {
        Summary id;
        id.map = IDENT;
#pragma unroll
        for (int s = 0; s < 8; s++) id.x[s] = 0;
        carry[k] = id;
    }
    for (uint32_t base = 0; base < nblk; base += SEGS) {
        Summary me;
        me.map = IDENT;
#pragma unroll
        for (int s = 0; s < 8; s++) me.x[s] = 0;
        if (base + seg < nblk) me = part[(size_t)(base + seg) * 4 + k];
        __syncthreads();
        sm[seg][k] = me;
        tree_reduce(sm, seg, k);
        if (seg == 0) {
            Summary c = carry[k];
            compose(c, sm[0][k]);
            carry[k] = c;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t S4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t s0 = q == 0 ? 3u : 0u;
            S4[q] = s0 ^ carry[q].x[s0];
        }
        for (uint32_t j = rounds * 16u; j < size; j++) S4[0] ^= ((uint32_t)in[j] + (1u << (S4[0] & 7u))) * PRIME;
        result[blockIdx.x] = S4[0] ^ S4[1] ^ S4[2] ^ S4[3];
    }
}

ChkSeg make_seg(const uint8_t *p, int32_t len, uint32_t wg_base)
{
    ChkSeg s;
    s.p = p;
    s.size = (uint32_t)len;
    s.rounds = s.size > 16 ? (s.size - 1) / 16 : 0;
    s.nblk = (s.rounds + SEGS * SEG - 1) / (SEGS * SEG);
    s.wg_base = wg_base;
    return s;
}

}  // namespace

// Checksum::IntegrityCheck of n segments in one pair of launches: crc of segment i lands in d_result[i] (device).  Segments of any
// length (0 .. 2^31 - 1 bytes) and start address; the grid holds the workgroups of all segments, found through the prefix table of
// their counts (wg_base).  n == 1 passes its segment by value; a larger batch uploads its table and synchronises the stream before
// it returns (the table's host copy lives here).
int jpk_checksums_device(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *len, uint32_t *d_result)
{
    if (n <= 0) return JPK_OK;
    std::vector<ChkSeg> segs((size_t)n);
    uint32_t total = 0;
    for (int i = 0; i < n; i++) { segs[(size_t)i] = make_seg(d_in[i], len[i], total); total += segs[(size_t)i].nblk; }
    ChkTab tab;
    tab.n = (uint32_t)n;
    tab.one = segs[0];
    tab.segs = nullptr;
    Arena plan(ctx, true);
    plan.get<Summary>((size_t)total * 4 + 4);
    if (n > 1) plan.get<ChkSeg>((size_t)n);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    Summary *part = real.get<Summary>((size_t)total * 4 + 4);
    if (n > 1) {
        ChkSeg *d_segs = real.get<ChkSeg>((size_t)n);
        JPK_HIP(hipMemcpyAsync(d_segs, segs.data(), (size_t)n * sizeof(ChkSeg), hipMemcpyHostToDevice, ctx->stream));
        tab.segs = d_segs;
    }
    uint64_t bytes = 0;
    for (int i = 0; i < n; i++) bytes += (uint32_t)len[i];
    if (total) JPK_LAUNCH(ctx, PROF_CHECKSUM, bytes, k_chk_segments, dim3(total), dim3(TB), tab, part);
    JPK_LAUNCH(ctx, PROF_CHECKSUM, 0, k_chk_fold, dim3((unsigned)n), dim3(TB), tab, part, d_result);
    JPK_HIP(hipGetLastError());
    if (n > 1) JPK_HIP(hipStreamSynchronize(ctx->stream));
    return JPK_OK;
}

// crc lands in d_result[0] (device); the caller reads it back with its own synchronisation
int jpk_checksum_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint32_t *d_result)
{
    return jpk_checksums_device(ctx, 1, &d_in, &len, d_result);
}
