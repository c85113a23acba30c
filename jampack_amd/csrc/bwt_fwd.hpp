// bwt_fwd.hpp -- what the translation units of the forward BWT's suffix sort share (bwt_fwd.hip and bwt_fwd_*.hip only; the algorithm
// overview is at the top of bwt_fwd.hip): tile constants, the device-resident state, the buffers, the small device helpers, and the host
// steps build_sa is made of.  Every kernel is defined in one unit, in its anonymous namespace, and launched only from that unit; what
// crosses a unit boundary lives in namespace jpk_sa.
#pragma once
#include "common.hpp"
#include "prims.hpp"

namespace jpk_sa {
using namespace jpk;

constexpr int TB = 256;
constexpr int WAVES = TB / 64;
constexpr uint32_t DONE = 0x80000000u;
constexpr uint32_t NONE = 0xFFFFFFFFu;
// Bit 30 of a group rank in the active list (ranks are SA positions < n <= JPK_MAX_BLOCKSIZE < 2^30): the suffix starts inside a run
// of >= D equal bytes (D = round 0's key depth).  Such suffixes do not double their way through the run (log2(run / D) rounds, each over every member of the
// run: an all-zero 64 MiB block took 25 rounds): round 1 sorts their group by (does the run end in a smaller or a larger byte, run
// length) -- the complete order among suffixes that start with the same byte repeated, see k_gather_win -- and from round 2 on they
// compare at the END of their run (distance = remaining run length, uniform inside the group by then) instead of at distance h.
constexpr uint32_t RUNF = 0x40000000u;
static_assert((uint64_t)JPK_MAX_BLOCKSIZE < (1ull << 30), "bit 30 of a rank is free");
static_assert(JPK_FWD_BWT_LIMIT == (1u << 30) && (uint64_t)JPK_MAX_BLOCKSIZE < JPK_FWD_BWT_LIMIT, "jpk_fwd_bwt_device refuses what would need bit 30");

constexpr int CT = 4096;                   // slots per tile of the streaming kernels (count / scatter), 16 per thread
constexpr int CT_ITEMS = CT / TB;          // 16: slot(w, k, l) = tile * CT + w * 1024 + k * 64 + l  -> ballot = one 64-bit word
constexpr int SEG_TILE = 1024;             // a workgroup owns the groups that START in its SEG_TILE window
constexpr int SEG_SPAN = 2 * SEG_TILE;     // ... and therefore sees at most this many elements
constexpr int SEG_ITEMS = SEG_SPAN / TB;   // 8
constexpr int SEG_DBITS = 9;               // digit width of the LDS sort: (<= 31-bit rank, 10-bit local group) = at most 5 passes
constexpr int SEG_DIGITS = 1 << SEG_DBITS;
constexpr int WIN_ITEMS = SEG_TILE / TB;   // 4: slot(w, k, l) = window * 1024 + w * 256 + k * 64 + l
static_assert(SEG_DIGITS == 2 * TB, "two digits per thread in the digit scan");

// device-resident bookkeeping of one suffix sort (lives in the arena; the host reads it asynchronously)
struct SaState {
    uint32_t m[2];                         // unresolved suffixes: round r reads m[r & 1] and writes m[(r + 1) & 1]
    uint32_t npieces;                      // pieces of large groups in the current round
    uint32_t lc;                           // members of large groups in the current round
    uint32_t nrun;                         // unresolved suffixes after round 0 that start inside a run of >= depth equal bytes
    uint32_t pair_steps;                   // k_pair_repair: positions walked so far in this pair round (its work is capped at 8 n)
    uint32_t round_m[JPK_SA_MAX_ROUNDS];   // per round: unresolved suffixes when it starts
    uint32_t round_lc[JPK_SA_MAX_ROUNDS];  // per round: of those, members of groups > SEG_TILE
    // round 0's key (k_key_plan): the text's bytes renumbered 0..sigma-1 in byte order, `bits` bits each, `depth` of them in 56 bits
    uint32_t bits, depth;
    uint32_t vmode;                        // 0: that fixed-width code; 1 / 2 / 3: the variable-length code of order 0 / 1 / 2 (below; k_key_final)
    uint64_t rep;                          // the key field of "code 1 repeated depth times": code * rep = a run of that code
    uint32_t present[256];                 // byte value occurs in the text
    uint8_t lut[256];                      // byte -> code
    // variable-length keys (vmode, round 5): an order-preserving PREFIX code of the block's bytes -- weight-balanced on a sampled
    // histogram -- instead of the fixed-width one: a key holds as many symbols as fit its 56 bits (about 56 / H0: ten for enwik8's 205
    // byte values where the fixed code holds seven) and every group of tied suffixes carries its own depth (GD, see build_sa)
    uint32_t tag_shift, tag_max;           // a key's depth rides in the sorted value's bits from tag_shift up: at most tag_max (26 and 63 up to 2^26 bytes)
    uint32_t cnt[256];                     // sampled byte counts (k_sym_present: every sixteenth 16-byte vector)
    uint32_t vcode[256];                   // code of byte b, right-justified in vlen[b] bits
    uint8_t vlen[256];
    uint8_t vrun_d[256];                   // symbols of a run of byte b that one key holds: 56 / vlen[b]
    uint16_t vtop[256];                    // the byte whose code (of at most 8 bits) starts these 8 bits, 0xFFFF: none
    uint64_t vrunkey[256];                 // the 56-bit key of a run of byte b
    // vmode 2 (order-1 code): every symbol but a key's first is coded in the context of the byte in front of it (256 alphabetic codes, one
    // per context, from sampled pair counts -- k_pair_counts / k_ctx_plan); what k_key_final decides on:
    uint32_t v0_ok, sigma, v0_wl, v0_wtot; // the order-0 code is usable (no code above 27 bits); its weighted length and weight
    uint32_t o1_w, o1_wl, o1_maxlen;       // sampled pairs, their weighted length under the context codes, the longest context code
    // vmode 3 (order-2 code): a key's symbols from the third on are coded in the context of the TWO bytes in front of them when that pair
    // is one of the `nclass` <= 1024 most frequent ones (k_ctx_select; its own row of the code table), behind the one byte otherwise
    uint32_t nclass, o2_w, o2_wl, o2_maxlen;
};
static_assert(offsetof(SaState, vmode) == offsetof(SaState, round_m) + sizeof(uint32_t) * (2 * JPK_SA_MAX_ROUNDS + 2), "the statistics copy takes round_m, round_lc, bits, depth, vmode in one piece");

// one piece of a large group: the part of the group that lies inside one 1024-slot window of the active list
struct Piece {
    uint32_t begin, count;                 // slots [begin, begin + count) of the active list
    uint32_t gs, ge;                       // the group: slots [gs, ge)
    uint32_t fp, nt, tl, pad;              // index of the group's first piece, pieces in the group, this piece's ordinal
};

__device__ __forceinline__ uint64_t mask_below(int l) { return (1ull << l) - 1ull; }              // lanes < l
__device__ __forceinline__ uint64_t mask_upto(int l) { return (l >= 63) ? ~0ull : ((2ull << l) - 1ull); }   // lanes <= l
__device__ __forceinline__ uint32_t top_bit(uint64_t v) { return 63u - (uint32_t)__clzll((long long)v); }   // v != 0

// ---- single-workgroup scans over small per-tile / per-window arrays (1024 threads) -----------------------------------
// (256 threads x 32 items since round 6 -- rounds 1-5: 1024 x 8.  A workgroup of 1024 needs sixteen free wave slots on ONE CU at the same
// moment; among the blocks in flight of the timed loop these kernels waited 100-500 us for that -- k_win_scan1 211 us on average for 3.5 us
// of work, profiles/r05_kernel_stats_bench_loop.txt -- and every kernel behind them on the block's stream with them.)
constexpr int WG1 = 256;
constexpr int WG1_ITEMS = 32;
// out[i] = scan of in[0..i] (inclusive) or in[0..i-1] (exclusive) starting from `init`; REV walks the array backwards
// (suffix scan).  Returns the reduction of everything (all threads).  in == out is allowed.
template <class Op, bool EXCL, bool REV>
__device__ __forceinline__ uint32_t wg_scan(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t init, uint32_t *sm)
{
    uint32_t carry = init;
    for (uint32_t c0 = 0; c0 < n; c0 += WG1 * WG1_ITEMS) {
        const uint32_t i0 = c0 + threadIdx.x * WG1_ITEMS;
        uint32_t v[WG1_ITEMS];
        uint32_t acc = Op::id();
#pragma unroll
        for (int k = 0; k < WG1_ITEMS; k++) {
            const uint32_t i = i0 + k;
            v[k] = (i < n) ? in[REV ? n - 1 - i : i] : Op::id();
            acc = Op::f(acc, v[k]);
        }
        uint32_t tot;
        const uint32_t inc = block_incl_scan<Op>(acc, sm, &tot);
        uint32_t prev = __shfl_up(inc, 1, 64);
        if (lane_id() == 0) prev = (threadIdx.x == 0) ? Op::id() : sm[(threadIdx.x >> 6) - 1];
        uint32_t run = Op::f(carry, prev);
#pragma unroll
        for (int k = 0; k < WG1_ITEMS; k++) {
            const uint32_t i = i0 + k;
            uint32_t o;
            if (EXCL) { o = run; run = Op::f(run, v[k]); }
            else { run = Op::f(run, v[k]); o = run; }
            if (i < n) out[REV ? n - 1 - i : i] = o;
        }
        carry = Op::f(carry, tot);
        __syncthreads();                    // sm is reused by the next chunk; the stores above are visible to the workgroup
    }
    return carry;
}

constexpr uint32_t JPK_O2_CLASSES = 1024;                 // order-2 contexts with a row of their own in the code table (k_ctx_select)
constexpr int SC_ITEMS = 16, SC_TILE = TB * SC_ITEMS;     // tile of the flat scan of the piece tables (k_tab_*)

// what the copies into the pinned mailbox (common.hpp JpkMail) assume
static_assert(offsetof(SaState, m) == offsetof(JpkMail::SaCounts, m) && offsetof(SaState, npieces) == offsetof(JpkMail::SaCounts, npieces) &&
              offsetof(SaState, lc) == offsetof(JpkMail::SaCounts, lc) && offsetof(SaState, nrun) == offsetof(JpkMail::SaCounts, nrun) &&
              offsetof(SaState, nrun) == 16 && sizeof(uint32_t) * JpkMail::SA_COUNT_WORDS == 20, "the rounds' copy takes m[2], npieces, lc, nrun in one piece");
static_assert(offsetof(SaState, round_lc) - offsetof(SaState, round_m) == offsetof(JpkMail::SaStats, round_lc) &&
              offsetof(SaState, bits) - offsetof(SaState, round_m) == offsetof(JpkMail::SaStats, bits) &&
              offsetof(SaState, depth) - offsetof(SaState, round_m) == offsetof(JpkMail::SaStats, depth) &&
              offsetof(SaState, vmode) - offsetof(SaState, round_m) == offsetof(JpkMail::SaStats, vmode) &&
              sizeof(JpkMail::SaStats) == sizeof(uint32_t) * (2 * JPK_SA_MAX_ROUNDS + 3), "the statistics copy lands member on member");

// ---- host side -------------------------------------------------------------------------------------------------------
struct SaBufs {
    uint64_t *keysA, *keysB;
    uint32_t *valsA, *valsB, *ISA, *SA, *a_sa, *a_grp, *b_sa, *b_grp, *k2, *k2alt, *sa_alt, *table;
    uint32_t *tA, *tB;          // per-tile scalars
    uint32_t *FH, *LH, *PH, *NH, *PC, *pLast, *partial, *scratch;
    uint8_t *bwt;
    uint8_t *a_prev, *b_prev, *p_alt;      // T[sa - 1] of every active suffix: travels with (sa, rank) through the rounds
    uint32_t *RL;                          // remaining run length per text position (written only when round 0 leaves run members behind)
    uint32_t *GD[2] = {nullptr, nullptr};  // variable-length keys: depth of every unresolved group by its rank, read side / write side of a round
    uint8_t *D0 = nullptr;                 // ... and the depth of every slot's key (rides through the radix sort in the value's upper bits up to 2^28 bytes)
    uint32_t *ctab = nullptr;              // ... and the table of the context codes (256 bytes + 1024 pairs of bytes, 256 codes each)
    uint16_t *ctxmap = nullptr;
    const uint8_t *blk = nullptr;          // group sort: block number of every text position, and where every block ends (device)
    const uint32_t *bend = nullptr;
    Piece *pieces;
    SaState *state;
};

// One workgroup per tile / window / piece of the host's (one round old) upper bound; the surplus workgroups of a shrunken
// list read the true count and leave.  Not persistent on purpose: a workgroup that has issued its random stores exits and
// its slot is refilled at once, whereas a grid-stride loop would wait for those stores at its next barrier (measured:
// k_seg_round 9.5 ms persistent against 8.1 ms).  The loops inside the kernels only matter beyond 2^20 tiles.
constexpr unsigned CAP = 1u << 20;
constexpr unsigned CAP_SEG = 1u << 20;

inline unsigned cap_grid(size_t work, unsigned per_block, unsigned cap)
{
    size_t g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}

// What the host knows while it enqueues one suffix sort: build_sa owns it, the steps below read and update it.
struct SaRun {
    uint32_t vmode_h = 0;                  // the code k_key_final chose (SaState::vmode), read back in front of the pack kernel
    uint64_t *ks = nullptr;                // round 0's sorted pairs sit in (ks, vs), one of the two pairs of radix buffers
    uint32_t *vs = nullptr;
    const uint8_t *Dx = nullptr;           // blocks above 2^28 bytes: the slots' depths, which nothing carries in the sorted value (r0_short)
    uint32_t bound = 0;                    // upper bound of the active count of the round being enqueued
    bool large_possible = true;            // a group above 1024 members may still exist
    bool lg_heavy = false;                 // many members of large groups ahead: the large-group kernels get the full grid
    bool runs_heavy = false;               // ... in round 1, where they are run members: the block is mostly runs
    int hshift = 0;                        // the next doubling round compares at distance depth << hshift
    int gd = 0;                            // variable-length keys: GD[gd] holds the groups' depths, the next doubling round writes GD[gd ^ 1]
    bool prev_pair = false;                // the round in front of this one was a pair round
};

// ---- the host steps of build_sa, each in the unit that owns its kernels; all enqueue on ctx->stream ------------------
// bwt_fwd_keys.hip -- round 0's keys: k_sym_present through the pack kernel, with the one 4-byte read back of the chosen code (-> r.vmode_h)
int sa_round0_keys(jpk_ctx *ctx, const uint8_t *T, uint32_t n, SaBufs &b, SaRun &r);
bool var_keys_eligible(size_t n, bool group);   // sa_layout's `var`
int var_tag_shift(size_t n);
// bwt_fwd_r0.hip -- round 0's sort and finish: the radix sort, the free ping-pong pair for the rounds' buffers, k_r0_finish
int sa_round0_sort(jpk_ctx *ctx, uint32_t n, SaBufs &b, SaRun &r);
void sa_run_lengths(jpk_ctx *ctx, const uint8_t *T, uint32_t n, SaBufs &b);
// bwt_fwd_rounds.hip -- one doubling round with its large-group passes; the compaction behind either kind of round
void sa_doubling_round(jpk_ctx *ctx, const uint8_t *T, uint32_t n, SaBufs &b, SaRun &r, int round);
int sa_compact(jpk_ctx *ctx, SaBufs &b, const SaRun &r, int round);
void sa_win_scan1(jpk_ctx *ctx, SaBufs &b, int par);      // k_win_scan1, which a pair round needs too
// bwt_fwd_pair.hip -- one pair round, and the host's rule for when a round is one
int sa_pair_round(jpk_ctx *ctx, uint32_t n, SaBufs &b, SaRun &r, int round);

// When a round is a pair round: the host's rule as a function of what it knows -- the list every round started with -- so that the CPU suite can
// run it on recorded lists (jpk_debug_pair_schedule, tests/test_abi_and_host.py).  `step` is called once per round >= 1 whose list size is known
// before it is enqueued, in order.
struct PairSchedule {
    int last_pair = -8;
    int gap;                            // rounds from the last pair round to the next: doubles (+ 1) behind one that did not pay (pair_rule_keep)
    bool prev_pair = false;
    uint32_t m_prev;                    // the list the previous round started with
    explicit PairSchedule(uint32_t n);
    bool step(int round, uint32_t m_now, uint32_t n, bool runs_heavy, bool exact_from_round_1);
};

}  // namespace jpk_sa
