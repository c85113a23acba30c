// bwt_fwd.hip -- forward BWT on gfx950: GPU suffix-array construction (replaces divsufsort, divsufsort.cpp:1721)
// followed by the BWT image and the 120 sampled ranks of BlockSort::Bwt::ForwardBwt (bwt.cpp:22-65).
//
// Suffix array = prefix doubling (Larsson-Sadakane ranks) with compaction of resolved suffixes:
//   round 0   key = the first symbols of the suffix in an order-preserving code of the block's alphabet, big-endian in 56 bits, zero padded:
//             a VARIABLE-LENGTH prefix code built from the block's sampled histogram (k_key_plan, k_pack_keys_var: about 56 / H0 symbols per
//             key -- 12 for English-like text over 28 byte values, 10 over enwik8's 205 -- and every group of tied suffixes carries its own
//             depth, GD) or, for flat histograms / blocks above 2^28 bytes / the comparators, a fixed-width code (D = 7 bytes for more than
//             128 byte values, 11 for 17..32, up to 56: k_pack_keys).  One LSD radix sort of all n suffixes, 7 passes (radix.hip), fed in
//             descending text position so that a short suffix -- a proper prefix of anything it ties with on the padded bits -- comes
//             first: plain suffix order even when the text contains the smallest symbol.
//   round r   unresolved suffixes only.  The active list keeps groups of equal rank contiguous and in SA order, so a group is sorted by
//             key2 = rank[sa + h] + 1 (0 past the end) independently, h = the symbols its members are known to share (the group's depth;
//             D, 2D, 4D, ... with the fixed-width code):
//               * k_gather_win   key2 of every active suffix (the round's only random READ), head flags per 1024-slot window
//               * groups of <= 1024 suffixes: k_seg_round -- one workgroup owns the groups that start in its window,
//                 stages (sa, key2, group id) in LDS, LDS radix sort, re-ranks;
//               * larger groups: segmented LSD radix sort IN PLACE on (key2, sa), tiles = the pieces a group cuts out of
//                 the windows it crosses; per-group digit-major tables laid out in window order, so one flat exclusive
//                 scan gives every piece its offsets inside its own group;
//               * new ranks go to ISA (the round's only random WRITE); a suffix that has become a group of one is
//                 finished: its BWT byte T[sa - 1] is emitted at its final SA position and it leaves the list;
//               * compaction of the survivors (count / scan of tile totals / scatter).
//   pair round  (k_pair_*, instead of a doubling round when the list stops shrinking) long repeats are resolved by induction from their
//             successors -- what divsufsort's induced sorting does -- instead of log2(LCP) doubling rounds; see the comment at k_pair_dist.
//   One ISA buffer: all reads of a round (k_gather_win) complete before its first write (kernel boundary), which is the
//   condition under which parallel Larsson-Sadakane is exact.
// Host synchronisations (since round 5, JPK_SA_WAIT_ROUND = 1): the number of active suffixes lives in device memory (SaState) and every
// kernel reads it there, but the host waits for the 20-byte copy of the previous round's counts in front of EVERY round (hipEventSynchronize:
// a few microseconds while the other blocks in flight keep the GPU busy) and enqueues exactly the grids, the large-group passes and the
// pair rounds that round needs; round 6 adds one 4-byte read back in front of round 0's pack kernel (which code k_key_final chose).
// JPK_SA_WAIT_ROUND=3 keeps rounds 1 and 2 enqueued blind, one round behind the host's knowledge (rounds 2-4).
// Every array stays in HBM: T n, ISA 4n, BWT-in-SA-order n, radix ping-pong 24n (re-used by the rounds), active list 8n.
#include "bwt_fwd.hpp"

using namespace jpk;
using namespace jpk_sa;

namespace {

// ---- BWT image (bwt.cpp:44-61) -------------------------------------------------------------------------------------
// bwt_sa[i] = T[SA[i] - 1] was emitted when suffix SA[i] was resolved; the image drops the row of suffix 0 (index idx = ISA[0])
// and starts with T[n-1]
__global__ __launch_bounds__(TB) void k_bwt_image(const uint8_t *__restrict__ T, const uint8_t *__restrict__ bwt_sa, const uint32_t *__restrict__ ISA,
                                                 uint32_t n, uint8_t *__restrict__ out)
{
    const uint32_t idx = ISA[0];
    for (uint32_t i = blockIdx.x * TB + threadIdx.x; i < n; i += gridDim.x * TB) {
        if (i == 0) out[0] = T[n - 1];
        if (i != idx) out[(i < idx) ? i + 1 : i] = bwt_sa[i];
    }
}

__global__ void k_bwt_trailer(const uint8_t *__restrict__ T, const uint32_t *__restrict__ ISA, uint32_t n, uint32_t len, uint8_t *__restrict__ out)
{
    uint32_t t = threadIdx.x;
    uint32_t step = n / JPK_BWT_UNITS;
    if (t < JPK_BWT_UNITS) {
        uint32_t v = ISA[(size_t)t * step] + 1u;
        uint8_t *p = out + len + 4 * t;
        p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
    }
    if (t < len - n) out[n + t] = T[n + t];      // raw tail (bwt.cpp:32-33), at most 119 bytes
}

// ---- host side -------------------------------------------------------------------------------------------------------
void sa_layout(Arena &a, size_t n, SaBufs &b, bool var)
{
    const size_t nwin = n / SEG_TILE + 2, ntile = n / CT + 2;
    memset(&b, 0, sizeof b);
    // (+ CT: round 0 sorts whole tiles -- the pack kernels fill the slots behind the text's end with the largest key)
    b.keysA = a.get<uint64_t>(n + CT);
    b.keysB = a.get<uint64_t>(n + CT);
    b.valsA = a.get<uint32_t>(n + CT);
    b.valsB = a.get<uint32_t>(n + CT);
    b.ISA = a.get<uint32_t>(n);
    b.a_sa = a.get<uint32_t>(n);
    b.a_grp = a.get<uint32_t>(n);
    b.bwt = a.get<uint8_t>(n + CT);
    b.a_prev = a.get<uint8_t>(n);
    b.b_prev = a.get<uint8_t>(n);
    b.p_alt = a.get<uint8_t>(n);
    b.RL = a.get<uint32_t>(n);
    if (var) {
        b.GD[0] = a.get<uint32_t>(n);
        b.GD[1] = a.get<uint32_t>(n);
        // (the slots' depths are read by the radix sort's first pass; the BWT bytes arrive from k_r0_finish on -- which, above 2^28 bytes, still reads the depths)
        b.D0 = var_tag_shift(n) < 32 ? b.bwt : a.get<uint8_t>(n + CT);
        // the context codes: sampled counts, then code | length << 27 of byte s behind byte c (rows 0..255) or behind a chosen pair of bytes
        b.ctab = a.get<uint32_t>(256 * (256 + JPK_O2_CLASSES));
        b.ctxmap = a.get<uint16_t>(65536);    // the row that codes a symbol behind the bytes c2 c1
    }
    const size_t nbmax = 256;
    b.table = a.get<uint32_t>(nbmax * 2 * nwin);
    b.partial = a.get<uint32_t>(nbmax * 2 * nwin / SC_TILE + 64);
    b.tA = a.get<uint32_t>(ntile);
    b.tB = a.get<uint32_t>(ntile);
    b.FH = a.get<uint32_t>(nwin);
    b.LH = a.get<uint32_t>(nwin);
    b.PH = a.get<uint32_t>(nwin);
    b.NH = a.get<uint32_t>(nwin);
    b.PC = a.get<uint32_t>(nwin);
    b.pLast = a.get<uint32_t>(2 * nwin);
    b.pieces = a.get<Piece>(2 * nwin);
    b.state = a.get<SaState>(1);
    b.scratch = a.get<uint32_t>(jpk_radix_scratch_words(n + CT));
}

// the planning pass of sa_layout: adds the bytes of the buffers of one sort of n bytes to plan.need
void sa_plan(Arena &plan, size_t n, bool group)
{
    SaBufs b;
    sa_layout(plan, n, b, var_keys_eligible(n, group));
}

// ... and the buffers themselves, from the start of ctx's arena, grown first when the plan asks for more
int sa_alloc(jpk_ctx *ctx, size_t n, SaBufs &b)
{
    Arena plan(ctx, true);
    sa_plan(plan, n, false);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    sa_layout(real, n, b, var_keys_eligible(n, false));
    return JPK_OK;
}

// the 20-byte copy of the counts round `round` leaves behind ({m[0], m[1], npieces, lc, nrun}) into the pinned mailbox's record
// round & 1, and the event that tells the host it has arrived
int post_counts(jpk_ctx *ctx, SaBufs &b, int round)
{
    JPK_HIP(hipMemcpyAsync(&ctx->h_mail->sa_counts[round & 1], &b.state->m[0], sizeof(uint32_t) * JpkMail::SA_COUNT_WORDS, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipEventRecord(ctx->ev_sa[round & 1], ctx->stream));
    return JPK_OK;
}

// builds the BWT-in-SA-order bytes (b.bwt), the complete inverse suffix array (b.ISA) and, if b.SA is set, the suffix array
int build_sa(jpk_ctx *ctx, const uint8_t *T, uint32_t n, SaBufs &b)
{
    ctx->stats.sa_rounds = 0;
    ctx->stats.sa_sorted_elems = 0;
    ctx->stats.sa_pair_rounds = 0;
    memset(ctx->stats.sa_round_active, 0, sizeof ctx->stats.sa_round_active);
    memset(ctx->stats.sa_round_large, 0, sizeof ctx->stats.sa_round_large);

    SaRun r;
    JPK_TRY(sa_round0_keys(ctx, T, n, b, r));
    JPK_TRY(sa_round0_sort(ctx, n, b, r));
    ctx->stats.sa_rounds = 1;
    JPK_TRY(post_counts(ctx, b, 0));
    const JpkMail::SaCounts *left = ctx->h_mail->sa_counts;      // pinned: left[r & 1] = what round r left behind
    // JPK_SA_WAIT_ROUND: the first round that is enqueued on exact counts (default 1 since the context codes: round 1 of text starts with
    // 27 M of 67 M suffixes, round 2 with 49 K -- 48 windows, no large group; enqueued blind they were 65 K / 26 K workgroups per kernel and, in
    // round 2, 23 launches for nothing.  The wait is a few microseconds in front of a round; 3 = round 4's rule)
    static const int wait_round = (int)jpk_env_long("JPK_SA_WAIT_ROUND", 1, 1, INT_MAX);
    // remaining run lengths, only if round 0 left members of runs of >= depth equal bytes behind.  The host knows (round 6: it waits for
    // round 0's counts here, where round 1 would wait a moment later): the three kernels -- 130-160 us each in the timed loop to find
    // nothing to do -- are launched only when there is (enqueued blind they return at once otherwise)
    bool runs_possible = true;
    if (wait_round <= 1) {
        JPK_HIP(hipEventSynchronize(ctx->ev_sa[0]));
        runs_possible = left[0].nrun != 0u;
    }
    if (runs_possible) sa_run_lengths(ctx, T, n, b);

    // Rounds 1 and 2 (the long ones: milliseconds each) are enqueued without waiting: the host learns the number of unresolved
    // suffixes one round late and enqueues round r with the grid bound of round r-2's result while the GPU is busy with round r-1.
    // From round 3 on the rounds are short and mostly empty, and what costs is their ~45 dependent launches each (a launch that has
    // nothing to do still waits its turn behind the other blocks' kernels: 90-190 us apiece in the timed loop): the host waits for
    // the previous round's counts first -- a few microseconds while other blocks keep the GPU busy -- and then enqueues exactly what is
    // needed: nothing when no suffix is unresolved (round 4: the trailing empty round is gone), no large-group passes (23 launches) once
    // a round has had no group above 1024 (groups only split: the count of their members never grows).
    r.bound = n;
    PairSchedule sched(n);
    uint64_t pair_mask = 0;
    for (int round = 1;; round++) {
        const int par = round & 1;
        const JpkMail::SaCounts &prev = left[par ^ 1];
        bool pair = false;
        if (round >= wait_round) {
            JPK_HIP(hipEventSynchronize(ctx->ev_sa[par ^ 1]));
            const uint32_t m_now = prev.m[par];                       // round r-1 wrote m[(r-1 & 1) ^ 1] = m[par]
            if (m_now == 0) break;                                    // nothing left: no empty round
            r.bound = m_now;
            if (round >= 2 && !r.prev_pair && prev.lc == 0) r.large_possible = false; // lc of round r-1 (a pair round does not count large groups)
            // many members of large groups ahead (round 1: run members, which round 0 counts; later: what the round before had): the full grid
            r.lg_heavy = round == 1 ? prev.nrun > n / 64u : prev.lc > (1u << 22);
            if (round == 1) r.runs_heavy = r.lg_heavy;
            ctx->stats.sa_rounds = round + 1;
            pair = sched.step(round, m_now, n, r.runs_heavy, wait_round <= 1);
        }
        r.prev_pair = pair;
        if (pair) {
            if (round < 64) pair_mask |= 1ull << round;
            JPK_TRY(sa_pair_round(ctx, n, b, r, round));
        } else {
            sa_doubling_round(ctx, T, n, b, r, round);
        }
        JPK_TRY(sa_compact(ctx, b, r, round));
        JPK_TRY(post_counts(ctx, b, round));
        if (round < wait_round) {
            // what the PREVIOUS round (or round 0) left behind: known without draining the queue
            JPK_HIP(hipEventSynchronize(ctx->ev_sa[par ^ 1]));
            const uint32_t m_start = prev.m[par];   // = the active count this round started with (round r-1 wrote m[par])
            if (m_start == 0) break;                // this round was empty: done
            ctx->stats.sa_rounds = round + 1;
            r.bound = m_start;
            sched.m_prev = m_start;
        }
        if (round >= 2 * JPK_SA_MAX_ROUNDS) return JPK_E_DEVICE;     // cannot happen: the distance doubles, every suffix is unique once it is >= n
    }
    ctx->stats.sa_pair_rounds = (int64_t)pair_mask;
    // statistics: one small copy, read by sa_collect_stats() after the caller has synchronised the stream
    JPK_HIP(hipMemcpyAsync(&ctx->h_mail->sa_stats, b.state->round_m, sizeof(JpkMail::SaStats), hipMemcpyDeviceToHost, ctx->stream));   // round_m, round_lc, bits, depth, vmode
    ctx->sa_stats_pending = true;
    return JPK_OK;
}

}  // namespace

void jpk_sa_stats_sync(jpk_ctx *ctx)
{
    if (!ctx->sa_stats_pending) return;
    ctx->sa_stats_pending = false;
    const JpkMail::SaStats &s = ctx->h_mail->sa_stats;
    const uint32_t *rm = s.round_m, *rl = s.round_lc;
    ctx->stats.sa_key_depth = (int32_t)s.depth;
    ctx->stats.sa_key_order = (int32_t)s.vmode - 1;      // vmode - 1: -1 = the fixed-width code
    for (int r = 0; r < JPK_SA_MAX_ROUNDS; r++) {
        const bool live = r < ctx->stats.sa_rounds;
        ctx->stats.sa_round_active[r] = live ? (int32_t)rm[r] : 0;
        ctx->stats.sa_round_large[r] = live ? (int32_t)rl[r] : 0;
        if (r >= 1 && live) ctx->stats.sa_sorted_elems += rm[r];
        if (r >= 1 && live && ctx->prof_on) {     // units of the round kernels are only known now
            ctx->prof_units[PROF_SA_KEYS] += rm[r];
            ctx->prof_units[PROF_SA_SEG] += rm[r] - rl[r];
            ctx->prof_units[PROF_SA_RERANK] += rm[r];
            ctx->prof_units[PROF_LG_HIST] += (uint64_t)rl[r] * 4;
            ctx->prof_units[PROF_LG_SCATTER] += (uint64_t)rl[r] * 4;
        }
    }
}

// arena bytes of one forward BWT of n sorted bytes (jpk_ctx_reserve)
size_t jpk_fwd_bwt_arena_bytes(uint32_t n)
{
    Arena plan(nullptr, true);
    sa_plan(plan, n ? n : 1, false);
    return plan.need;
}

int jpk_suffix_array_device(jpk_ctx *ctx, const uint8_t *d_t, int32_t n, int32_t *d_sa)
{
    if (n <= 0) return JPK_OK;
    SaBufs b;
    JPK_TRY(sa_alloc(ctx, (size_t)n, b));
    b.SA = reinterpret_cast<uint32_t *>(d_sa);
    return build_sa(ctx, d_t, (uint32_t)n, b);
}

// ---- group sort: the forward BWTs of several (small) blocks as ONE suffix sort ------------------------------------------------
// Jampack's default block is 8 MiB and its smallest 1 MiB (format.hpp:20-22); a block costs ~200 dependent launches whatever its
// size, so small blocks are sorted together: their sorted parts are laid end to end as one text, every suffix stops at the end of
// its own block, and the block number is the sort's most significant digit -- block b's suffixes then occupy exactly the slots
// [start_b, start_b + nlen_b) of the common suffix array, ranks and positions are global, and each block's image and trailer come
// out of its own slice (bwt.cpp:44-61 per block).  In this mode the byte that rides with every active suffix is its block number
// (the end of its block is one table lookup away), so the BWT bytes are gathered from the text at the end: T[SA[i] - 1].
namespace {
struct GroupBlk {
    const uint8_t *src;        // the block as the caller gave it
    uint8_t *img;              // where its image goes (len + 480 bytes)
    uint32_t start, nlen, len; // slice of the common text / suffix array; bytes of the block
    uint32_t pad;
};
__global__ __launch_bounds__(TB) void k_group_concat(const GroupBlk *__restrict__ gb, uint8_t *__restrict__ C, uint8_t *__restrict__ blk)
{
    const GroupBlk g = gb[blockIdx.y];
    for (uint32_t base = blockIdx.x * TB * 16; base < g.nlen; base += gridDim.x * TB * 16) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t p = base + k * TB + threadIdx.x;
            if (p < g.nlen) { C[g.start + p] = g.src[p]; blk[g.start + p] = (uint8_t)blockIdx.y; }
        }
    }
}
__global__ __launch_bounds__(TB) void k_group_image(const GroupBlk *__restrict__ gb, const uint8_t *__restrict__ C, const uint32_t *__restrict__ SA,
                                                   const uint32_t *__restrict__ ISA)
{
    const GroupBlk g = gb[blockIdx.y];
    if (blockIdx.x == 0) {
        // raw tail (bwt.cpp:32-33) and, if anything was sorted, the 120 sampled ranks (bwt.cpp:58-61); a block shorter than 120
        // bytes leaves its trailer alone (bwt.cpp:35; the caller has zeroed the image)
        const uint32_t t = threadIdx.x;
        if (t < g.len - g.nlen) g.img[g.nlen + t] = g.src[g.nlen + t];
        if (g.nlen && t < JPK_BWT_UNITS) {
            const uint32_t v = ISA[g.start + (size_t)t * (g.nlen / JPK_BWT_UNITS)] - g.start + 1u;
            uint8_t *p = g.img + g.len + 4 * t;
            p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
        }
    }
    if (g.nlen == 0) return;
    const uint32_t idx = ISA[g.start] - g.start;                     // row of the block's suffix 0: dropped, the image starts with T[nlen-1]
    for (uint32_t i = blockIdx.x * TB + threadIdx.x; i < g.nlen; i += gridDim.x * TB) {
        if (i == 0) g.img[0] = C[g.start + g.nlen - 1];
        if (i != idx) g.img[(i < idx) ? i + 1 : i] = C[SA[g.start + i] - 1];
    }
}
}  // namespace

size_t jpk_fwd_bwt_group_arena_bytes(uint32_t total_nlen, int nblk)
{
    Arena plan(nullptr, true);
    sa_plan(plan, total_nlen ? total_nlen : 1, true);
    plan.get<uint8_t>(total_nlen);            // common text
    plan.get<uint8_t>(total_nlen);            // block number per position
    plan.get<uint32_t>(total_nlen);           // suffix array (the BWT bytes are gathered through it)
    plan.get<uint32_t>((size_t)nblk + 1);
    plan.get<GroupBlk>((size_t)nblk);
    return plan.need;
}

// d_in[b] / len[b]: the blocks; d_img[b]: len[b] + 480 bytes each (zeroed by the caller when len[b] < 120).  At most 256 blocks, the
// sum of their sorted parts < 2^30.  Everything is enqueued on ctx->stream; the arena (at ctx->arena_base) must hold
// jpk_fwd_bwt_group_arena_bytes().
int jpk_fwd_bwt_group_device(jpk_ctx *ctx, int nblk, const uint8_t *const *d_in, const int32_t *len, uint8_t *const *d_img)
{
    if (nblk <= 0) return JPK_OK;
    if (nblk > 256) return JPK_E_ARG;
    // the two small tables are staged in the context's pinned page (16 KB: 256 x 32 B + 257 x 4 B), which outlives this call -- the
    // copies below are asynchronous; a context runs one call at a time and every caller synchronises before the next
    static_assert(sizeof(GroupBlk) * 256 + 4 * 257 <= 4096 * 4, "tables fit the pinned page");
    GroupBlk *gb = reinterpret_cast<GroupBlk *>(ctx->h_map);
    uint32_t *bend = ctx->h_map + sizeof(GroupBlk) * 256 / 4;
    uint64_t total = 0;
    uint32_t maxlen = 1;
    for (int b = 0; b < nblk; b++) {
        const uint32_t l = (uint32_t)len[b], nl = l - l % JPK_BWT_UNITS;
        gb[b] = GroupBlk{d_in[b], d_img[b], (uint32_t)total, nl, l, 0u};
        total += nl;
        bend[b] = (uint32_t)total;
        if (l > maxlen) maxlen = l;
    }
    if (total >= (1ull << 30)) return JPK_E_ARG;
    const uint32_t N = (uint32_t)total;
    const JpkCompressInflight inflight(ctx->device);
    SaBufs sb;
    Arena real(ctx, false);
    sa_layout(real, N ? N : 1, sb, var_keys_eligible(N ? N : 1, true));
    uint8_t *C = real.get<uint8_t>(N);
    uint8_t *blk = real.get<uint8_t>(N);
    uint32_t *SA = real.get<uint32_t>(N);
    uint32_t *d_bend = real.get<uint32_t>((size_t)nblk + 1);
    GroupBlk *d_gb = real.get<GroupBlk>((size_t)nblk);
    if (ctx->arena_off > ctx->arena_cap) return JPK_E_ALLOC;
    JPK_HIP(hipMemcpyAsync(d_bend, bend, sizeof(uint32_t) * (size_t)nblk, hipMemcpyHostToDevice, ctx->stream));
    JPK_HIP(hipMemcpyAsync(d_gb, gb, sizeof(GroupBlk) * (size_t)nblk, hipMemcpyHostToDevice, ctx->stream));
    const unsigned gx = cap_grid(maxlen, TB * 16, 1024);
    if (N) {
        hipLaunchKernelGGL(k_group_concat, dim3(gx, nblk), dim3(TB), 0, ctx->stream, d_gb, C, blk);
        sb.SA = SA;
        sb.blk = blk;
        sb.bend = d_bend;
        JPK_TRY(build_sa(ctx, C, N, sb));
    }
    JPK_LAUNCH(ctx, PROF_BWT_GATHER, N, k_group_image, dim3(cap_grid(maxlen, TB * 4, 4096), nblk), dim3(TB), d_gb, C, SA, sb.ISA);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

int jpk_fwd_bwt_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out)
{
    // ranks keep bit 30 and bit 31 for flags (above): a block of 2^30 bytes or more is refused, not sorted wrongly.  The format's largest
    // block (JPK_MAX_BLOCKSIZE = 1000 MiB, format.hpp:22) is below that
    if (len < 0 || (uint32_t)len >= JPK_FWD_BWT_LIMIT) return JPK_E_ARG;
    const JpkCompressInflight inflight(ctx->device);      // counted while this block is in its suffix sort
    const int32_t rem = len % JPK_BWT_UNITS, nlen = len - rem;
    if (nlen <= 0) {
        // bwt.cpp:29-35: only the raw tail is produced; the 480 trailer bytes are left untouched
        if (rem > 0) JPK_HIP(hipMemcpyAsync(d_out, d_in, (size_t)rem, hipMemcpyDeviceToDevice, ctx->stream));
        return JPK_OK;
    }
    SaBufs b;
    JPK_TRY(sa_alloc(ctx, (size_t)nlen, b));
    JPK_TRY(build_sa(ctx, d_in, (uint32_t)nlen, b));
    JPK_LAUNCH(ctx, PROF_BWT_GATHER, nlen, k_bwt_image, dim3(cap_grid((size_t)nlen, TB * 16, 4096)), dim3(TB), d_in, b.bwt, b.ISA, (uint32_t)nlen, d_out);
    hipLaunchKernelGGL(k_bwt_trailer, dim3(1), dim3(128), 0, ctx->stream, d_in, b.ISA, (uint32_t)nlen, (uint32_t)len, d_out);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}
