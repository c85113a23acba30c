// bwt_fwd_pair.hip -- forward BWT, the pair rule: the round that resolves long repeats by induction from their successors, and the host's
// rule for when a round is one (PairSchedule) (overview: bwt_fwd.hip).
#include "bwt_fwd.hpp"

using namespace jpk;
using namespace jpk_sa;

namespace {

// ---- the pair rule: long repeats do not double their way out (round 5) --------------------------------------------------------
// A repeat T[u .. u+L) == T[v .. v+L) leaves L groups {u+q, v+q} that doubling resolves only once its distance exceeds L - q:
// log2(L) rounds over all of them (a 1 MiB segment repeated: 24 rounds; divsufsort.cpp:1427-1520 has no such cliff -- it induces the
// order of most suffixes from their successors).  This is that induction step on the active list, between two doubling rounds.
// Members of a group sit in DESCENDING text position (round 0 is a stable sort fed in descending position, every later sort is
// stable).  For a member s that is not the first of its group let P[s] = s' - s, s' = the member in front of it; P = 0 elsewhere.
// s and s + P[s] are in one group, so they share their first byte, so  order(s, s + p) = order(s + 1, s + 1 + p).  Along a maximal
// stretch of positions [a, x] with one non-zero P = p the argument repeats: every pair (y, y + p) of the stretch is ordered like
// (x + 1, x + 1 + p), and THAT pair is decided now if the two suffixes lie in different groups (their ranks compare) or x + 1 + p is
// the end of the text / block (the empty suffix is the smaller one), or -- in a second pass over the stretches -- if they lie in one group
// and the neighbouring pairs between them all carry one verdict.  A group all of whose neighbouring pairs carry the same decided
// verdict is totally ordered by position: its members are finished with ranks G, G + 1, ...; every other group stays exactly as it
// was (the doubling distance does not change).  p = 1 is the run rule's case.  tests/pair_rule_model.py states the same in Python and
// tests/test_pair_rule_model.py checks it against a brute-force suffix sort on repeat-heavy texts.
//   k_pair_dist    P[s] (random 4-byte store per member), FH / LH of every window
//   k_pair_first / k_pair_scan / k_pair_fill   first stretch end at or after every position (the k_run_* scheme on P instead of T),
//                  verdict of that end -> V[y] for every y with P[y] != 0   (1: the lower position is smaller, 2: the higher, 0: open)
//   k_pair_mark    VL[j] = verdict of list slot j (0xFF for a group's first member); BAD[G] = 1 for a group with an open or a
//                  dissenting pair (G = the group's rank: the list is in rank order, so these accesses walk BAD upwards)
//   k_pair_finish  members of the other groups: rank -> ISA, BWT byte, DONE; everything to the b-list; compaction follows as in a round
constexpr uint8_t PV_HEAD = 0xFF;
constexpr uint32_t PREP = 0x80000000u;      // P[z]: the stretch was carried THROUGH z by k_pair_repair (z's own neighbour is nearer): distances are < 2^30
__global__ __launch_bounds__(TB) void k_pair_dist(const uint32_t *__restrict__ a_sa, const uint32_t *__restrict__ a_grp, const SaState *__restrict__ st, int par,
                                                 uint32_t *__restrict__ P, uint32_t *__restrict__ FH, uint32_t *__restrict__ LH)
{
    __shared__ uint64_t H[16];
    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    for (uint32_t win = blockIdx.x; win < nwin; win += gridDim.x) {
        const uint32_t base = win * SEG_TILE;
        __syncthreads();
        uint32_t s[WIN_ITEMS], sp[WIN_ITEMS], gj[WIN_ITEMS], gp[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l, jc = j < m ? j : m - 1, jp = jc ? jc - 1 : 0;
            s[k] = a_sa[jc];
            sp[k] = a_sa[jp];
            gj[k] = a_grp[jc];
            gp[k] = a_grp[jp];
        }
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l;
            bool head = false;
            if (j < m) {
                head = (j == 0) || (gj[k] != gp[k]);
                if (!head) P[s[k]] = sp[k] - s[k];
            }
            const uint64_t b = __ballot(head);
            if (l == 0) H[w * WIN_ITEMS + k] = b;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const uint64_t hv = (l < 16) ? H[l] : 0ull;
            uint32_t first = hv ? base + l * 64 + (uint32_t)__builtin_ctzll(hv) + 1u : NONE;
            uint32_t last = hv ? base + l * 64 + top_bit(hv) + 1u : 0u;
            first = wave_incl_min(first);
            last = wave_incl_max(last);
            if (l == 63) { FH[win] = (first == NONE) ? 0u : first; LH[win] = last; }
        }
    }
}

// A group that mixes two repeats cuts the stretches of BOTH: its members' neighbours are nearer than the repeats' distance p, so the
// positions of an inner repeat (a phrase that occurs twice inside a segment that is itself repeated) end every stretch that reaches them
// in an open pair -- and a segment with a thousand inner repeats has a thousand stretch pieces, all but the last open.  But the
// induction only needs T[z] = T[z + p], and z and z + p ARE in one group there: the thread of a stretch end walks on through such
// positions and writes p (with PREP) over their own distance until the stretch's own distance returns, the two suffixes part, or
// the text ends.  The walk reads consecutive ranks (z and z + p advance together).  A position that was walked through gives up its own
// pair (V = 0: its group, a mixed one, waits for the doubling rounds).  Inner repeats start walks of their own through the same positions:
// the largest distance wins (atomicMax; PREP is the top bit, so any carried distance beats a position's own) -- the outer repeat's
// stretch is the long one.  Any winner is a true same-group distance.
constexpr int PAIR_WALK_MAX = 2048;
__global__ __launch_bounds__(TB) void k_pair_repair(uint32_t *P, uint32_t n, const uint32_t *__restrict__ ISA, const uint8_t *__restrict__ blk,
                                                   const uint32_t *__restrict__ bend, SaState *__restrict__ st, uint32_t budget)
{
    for (uint32_t x = blockIdx.x * TB + threadIdx.x; x + 1u < n; x += gridDim.x * TB) {
        const uint32_t p = P[x];
        if (p == 0u || (p & PREP)) continue;
        if ((P[x + 1u] & ~PREP) == p) continue;                   // not a stretch end
        const uint32_t lim = bend ? bend[blk[x]] : n;
        uint32_t z = x + 1u;
        for (int step = 0; step < PAIR_WALK_MAX; step++, z++) {
            // (all walks of a pair round together stay below 8 n positions: an input built to make every position a stretch end with a long
            // walk behind it costs a bounded pass, and the stretches it leaves cut wait for the doubling rounds)
            if ((step & 31) == 31 && atomicAdd(&st->pair_steps, 32u) > budget) break;
            if ((uint64_t)z + p >= lim) break;                    // the pair behind the stretch reaches the end of the text: decided there
            if ((P[z] & ~PREP) == p) break;                       // the stretch's own distance again: it runs on by itself
            if (ISA[z] != ISA[z + p]) break;                      // the two suffixes part: decided by their ranks
            atomicMax(&P[z], p | PREP);                            // the LARGEST distance carried through z wins: the outer repeat, not an inner one
        }
    }
}

// P has n + 1 entries, P[n] = 0: position x ends a stretch when P[x] != P[x + 1] (distances compared without PREP)
__global__ __launch_bounds__(TB) void k_pair_first(const uint32_t *__restrict__ P, uint32_t n, uint32_t *__restrict__ tFirst)
{
    __shared__ uint32_t sm[TB / 64 + 1];
    const uint32_t ntiles = (n + CT - 1) / CT;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * CT;
        uint32_t pa[CT_ITEMS], pb[CT_ITEMS];
#pragma unroll
        for (int k = 0; k < CT_ITEMS; k++) {
            const uint32_t i = base + k * TB + threadIdx.x, ic = i < n ? i : n - 1;
            pa[k] = P[ic] & ~PREP;
            pb[k] = P[ic + 1] & ~PREP;
        }
        uint32_t first = NONE;
#pragma unroll
        for (int k = CT_ITEMS - 1; k >= 0; k--) {
            const uint32_t i = base + k * TB + threadIdx.x;
            if (i < n && pa[k] != pb[k]) first = i;
        }
        uint32_t tot;
        block_incl_scan<OpMin>(first, sm, &tot);
        if (threadIdx.x == 0) tFirst[tile] = tot;
        __syncthreads();
    }
}
__global__ __launch_bounds__(WG1) void k_pair_scan(uint32_t *__restrict__ tFirst, uint32_t n)
{
    __shared__ uint32_t sm[WG1 / 64 + 1];
    wg_scan<OpMin, true, true>(tFirst, tFirst, (n + CT - 1) / CT, NONE, sm);      // first stretch end in any LATER tile
}
// verdict of the stretch that ends at x with distance p: the pair (x + 1, x + 1 + p).  When the two lie in ONE group with other
// members between them (x + 1 belongs to a group that mixes two repeats: its neighbour is nearer than p), the pair stays open (0).
__device__ __forceinline__ uint32_t pair_verdict(uint32_t x, uint32_t p, const uint32_t *__restrict__ ISA, uint32_t n, const uint8_t *__restrict__ blk,
                                                 const uint32_t *__restrict__ bend)
{
    const uint32_t lim = bend ? bend[blk[x]] : n;
    const uint64_t b = (uint64_t)x + 1u + p;                     // x + p is a member's position (< lim), so b <= lim
    if (b >= lim) return 2u;
    const uint32_t ra = ISA[x + 1u], rb = ISA[b];
    if (ra != rb) return ra < rb ? 1u : 2u;
    return 0u;
}
__global__ __launch_bounds__(TB) void k_pair_fill(const uint32_t *__restrict__ P, uint32_t n, const uint32_t *__restrict__ tAfter, const uint32_t *__restrict__ ISA,
                                                 uint8_t *V, const uint8_t *__restrict__ blk, const uint32_t *__restrict__ bend)
{
    __shared__ uint32_t sm[TB / 64 + 1];
    __shared__ uint32_t rv[TB];
    const uint32_t ntiles = (n + CT - 1) / CT;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * CT, p0 = base + threadIdx.x * CT_ITEMS;        // blocked: sixteen consecutive positions per thread
        uint32_t pv[CT_ITEMS + 1];
#pragma unroll
        for (int k = 0; k <= CT_ITEMS; k++) { const uint32_t i = p0 + k; pv[k] = P[i < n ? i : n]; }
        uint32_t bits = 0, first = NONE, any = 0, rep = 0;
#pragma unroll
        for (int k = CT_ITEMS - 1; k >= 0; k--) {
            const uint32_t i = p0 + k;
            if (i < n) {
                any |= pv[k];
                if (pv[k] & PREP) rep |= 1u << k;
                if ((pv[k] & ~PREP) != (pv[k + 1] & ~PREP)) { bits |= 1u << k; first = i; }
            }
        }
#pragma unroll
        for (int k = 0; k <= CT_ITEMS; k++) pv[k] &= ~PREP;
        __syncthreads();                                                              // rv of the previous tile has been read
        rv[TB - 1 - threadIdx.x] = first;
        __syncthreads();
        const uint32_t rinc = block_incl_scan<OpMin>(rv[threadIdx.x], sm, nullptr);   // index u: min over the threads >= TB - 1 - u
        __syncthreads();
        rv[threadIdx.x] = rinc;
        __syncthreads();
        uint32_t nb = (threadIdx.x == TB - 1) ? NONE : rv[TB - 2 - threadIdx.x];
        if (nb == NONE) nb = tAfter[tile];
        if (!any) continue;                                                           // (nothing of mine is a member; the barriers above are behind us)
        uint32_t vnb = NONE;                                                          // verdict of the stretch end nb: not computed yet
#pragma unroll
        for (int k = CT_ITEMS - 1; k >= 0; k--) {
            const uint32_t i = p0 + k;
            if (i < n) {
                const uint32_t p = pv[k];
                if (bits & (1u << k)) { nb = i; vnb = p ? pair_verdict(i, p, ISA, n, blk, bend) : 0u; }
                if (p) {
                    if (vnb == NONE) vnb = pair_verdict(nb, p, ISA, n, blk, bend);   // the stretch runs on into a later thread: P[nb] == p
                    V[i] = (rep & (1u << k)) ? (uint8_t)0 : (uint8_t)vnb;      // a position the stretch was carried through: ITS pair stays open
                }
            }
        }
    }
}

__global__ __launch_bounds__(TB) void k_pair_mark(const uint32_t *__restrict__ a_sa, const uint32_t *__restrict__ a_grp, const SaState *__restrict__ st, int par,
                                                 const uint8_t *__restrict__ V, uint8_t *__restrict__ VL, uint8_t *__restrict__ BAD)
{
    __shared__ uint8_t cs[SEG_TILE + 1];       // cs[q + 1] = code of local slot q (verdict, PV_HEAD for a group's first member); cs[0]: the slot in front of the window
    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    for (uint32_t win = blockIdx.x; win < nwin; win += gridDim.x) {
        const uint32_t base = win * SEG_TILE;
        __syncthreads();
        uint32_t s[WIN_ITEMS], gj[WIN_ITEMS], gp[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l, jc = j < m ? j : m - 1;
            s[k] = a_sa[jc];
            gj[k] = a_grp[jc];
            gp[k] = a_grp[jc ? jc - 1 : 0];
        }
        uint8_t c[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l;
            const bool head = (j == 0) || (gj[k] != gp[k]);
            c[k] = PV_HEAD;
            if (j < m && !head) c[k] = V[s[k]];
        }
        if (threadIdx.x == 0) {
            uint8_t c0 = PV_HEAD;
            if (base >= 2u && a_grp[base - 1] == a_grp[base - 2]) c0 = V[a_sa[base - 1]];
            cs[0] = c0;
        }
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t q = w * (64 * WIN_ITEMS) + k * 64 + l;
            cs[q + 1] = c[k];
            if (base + q < m) VL[base + q] = c[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t q = w * (64 * WIN_ITEMS) + k * 64 + l;
            if (base + q < m && c[k] != PV_HEAD) {
                const uint8_t pc = cs[q];
                if (c[k] == 0 || (pc != PV_HEAD && pc != c[k])) BAD[gj[k] & ~(RUNF | DONE)] = 1;      // (same value from every writer)
            }
        }
    }
}

__global__ __launch_bounds__(TB) void k_pair_finish(const uint32_t *__restrict__ a_sa, const uint32_t *__restrict__ a_grp, const uint8_t *__restrict__ a_prev,
                                                   const SaState *__restrict__ st, int par, const uint32_t *__restrict__ PH, const uint32_t *__restrict__ NH,
                                                   const uint8_t *__restrict__ VL, const uint8_t *__restrict__ BAD,
                                                   uint32_t *__restrict__ ISA, uint8_t *__restrict__ bwt, uint32_t *__restrict__ SA,
                                                   uint32_t *__restrict__ b_sa, uint32_t *__restrict__ b_grp, uint8_t *__restrict__ b_prev)
{
    __shared__ uint64_t H[16];
    __shared__ uint32_t LHW[16];               // 1 + last head position at or before the end of word l (carry included)
    __shared__ uint32_t NHW[16];               // first head position in a word AFTER word l (the next window's included)
    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    for (uint32_t win = blockIdx.x; win < nwin; win += gridDim.x) {
        const uint32_t base = win * SEG_TILE;
        __syncthreads();
        uint32_t s[WIN_ITEMS], gj[WIN_ITEMS], gp[WIN_ITEMS];
        uint8_t pv[WIN_ITEMS], cj[WIN_ITEMS], cn[WIN_ITEMS], bad[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l, jc = j < m ? j : m - 1;
            s[k] = a_sa[jc];
            gj[k] = a_grp[jc];
            gp[k] = a_grp[jc ? jc - 1 : 0];
            pv[k] = a_prev[jc];
            cj[k] = VL[jc];
            cn[k] = VL[jc + 1 < m ? jc + 1 : jc];
        }
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) bad[k] = BAD[gj[k] & ~(RUNF | DONE)];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l;
            const bool head = j < m && ((j == 0) || (gj[k] != gp[k]));
            const uint64_t b = __ballot(head);
            if (l == 0) H[w * WIN_ITEMS + k] = b;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const uint64_t hv = (l < 16) ? H[l] : 0ull;
            const uint32_t carry = win ? PH[win - 1] : 0u;
            uint32_t last = hv ? base + l * 64 + top_bit(hv) + 1u : 0u;
            last = wave_incl_max(last);
            if (l < 16) LHW[l] = last > carry ? last : carry;
            // first head in the words after l: inclusive min-scan over the words in reverse order, shifted by one
            const int rl = 15 - l;                                                  // lane l holds word 15 - l
            const uint64_t hr = (l < 16) ? H[rl] : 0ull;
            uint32_t firstr = hr ? base + rl * 64 + (uint32_t)__builtin_ctzll(hr) : NONE;
            firstr = wave_incl_min(firstr);                                          // lane l: min over words >= 15 - l
            const uint32_t after = NH[win];
            const uint32_t prevlane = __shfl_up(firstr, 1, 64);                      // word x = 15 - l wants the min over words > x = lane l - 1's value
            if (l < 16) {
                uint32_t v = (l == 0) ? NONE : prevlane;
                if (v == NONE) v = after;
                NHW[rl] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const int word = w * WIN_ITEMS + k;
            const uint32_t j = base + word * 64 + l;
            if (j < m) {
                const uint64_t hv = H[word];
                const bool head = (hv >> l) & 1ull;
                const uint32_t G = gj[k] & ~(RUNF | DONE);
                uint32_t out_g = gj[k];
                if (!bad[k]) {
                    const uint64_t le = hv & mask_upto(l);
                    const uint32_t gs = le ? base + word * 64 + top_bit(le) : (word ? LHW[word - 1] : (win ? PH[win - 1] : 0u)) - 1u;
                    const uint64_t gt = (l < 63) ? (hv >> (l + 1)) : 0ull;
                    uint32_t ge = gt ? j + 1u + (uint32_t)__builtin_ctzll(gt) : NHW[word];
                    if (ge > m) ge = m;
                    const uint8_t v = head ? cn[k] : cj[k];              // a group has at least two members: the slot behind a head is its pair
                    const uint32_t r = (v == 2) ? G + (j - gs) : G + (ge - 1u - j);
                    if (r != G) ISA[s[k]] = r;
                    bwt[r] = pv[k];
                    if (SA) SA[r] = s[k];
                    out_g = r | DONE;
                }
                b_sa[j] = s[k];
                b_grp[j] = out_g;
                b_prev[j] = pv[k];
            }
        }
    }
}

}  // namespace

namespace jpk_sa {

namespace {
// JPK_PAIR_SHIFT: a round from the third on is a pair round (k_pair_*) when at least n >> shift suffixes are unresolved (default 6);
// negative = never (the comparator: plain prefix doubling)
int pair_rule_shift()
{
    static const int v = (int)jpk_env_long("JPK_PAIR_SHIFT", 6, INT_MIN, 31);
    return v;
}
// the first round that may be a pair round.  2 measured worse: a 4 KiB period 17.2 -> 13.5 ms, but the silesia-like block 11.9 -> 16.6, long
// runs 18.9 -> 40.5 ms -- after one doubling round the groups of a repeat still mix everything that shares 30 symbols.  Round 1 has to be a
// doubling round in any case: it is the one that spreads the run members
constexpr int PAIR_FROM = 3;
// JPK_PAIR_EARLY=0: no pair round at round 2 for lists that round 1 left as they were (comparator)
bool pair_rule_early()
{
    static const bool v = jpk_env_long("JPK_PAIR_EARLY", 1) != 0;
    return v;
}
// JPK_PAIR_MIN: ... and at least this many (default 4096; the tests lower it so that tiny inputs take the path);
// JPK_PAIR_GAP: rounds from one pair round to the next (default 3 = two doubling rounds in between, at least 2)
uint32_t pair_rule_min()
{
    static const uint32_t v = (uint32_t)jpk_env_long("JPK_PAIR_MIN", 4096, 2);
    return v;
}
// JPK_PAIR_RATIO: ... and the previous round left at least this percentage of ITS list unresolved -- 0 = whatever the previous round did.
// Default 90 since the end of round 6 (60 before): what the rule is for -- exact repeats, periodic data, a block that holds a file twice --
// keeps 99-100 % of its list through a doubling round (tools/pair_yield.py) and a pair round then resolves 84-100 % of it; REAL trees of
// near-duplicate files (64 MiB of this image's Python and ROCm sources: 16 rounds, each leaving 60-85 %) crossed the old threshold three
// times, every pair round there left 74-90 % of its list and cost 4 ms (k_pair_repair's walks): 35.0 against 22.9 ms per block without them.
uint32_t pair_rule_ratio()
{
    static const uint32_t v = (uint32_t)jpk_env_long("JPK_PAIR_RATIO", 90, 0, 100);
    return v;
}
// positions all walks of k_pair_repair together may visit in one pair round, in eighths of n (8 n until the end of round 6: no block whose
// pair rounds pay notices the difference, a pair round that does not pay costs 7 ms less on 64 MiB of real binaries)
constexpr uint32_t PAIR_BUDGET_EIGHTHS = 1;
uint32_t pair_rule_budget(uint32_t n) { return (uint32_t)((uint64_t)n * PAIR_BUDGET_EIGHTHS / 8u); }
// JPK_PAIR_KEEP: a pair round that leaves more than this percentage of its list did not pay (default 50; 100 = every one pays): the next one
// waits twice as long (two doubling rounds, then six, fourteen, thirty).  The Fibonacci word took nine pair rounds that resolved NOTHING, every
// one a round in which the doubling distance stands still (105 -> 60 ms per 32 MiB); a block that holds a real tree TWICE -- near-duplicate files
// inside an exact copy -- takes pair rounds that leave 93-100 % until doubling has dissolved the inner repeats, and then one that leaves nothing
// (round 12-15 of 23): giving up after the first would cost such a block its best round (tools/pair_yield.py, profiles/r06_real_files_pair_rounds.txt).
uint32_t pair_rule_keep()
{
    static const uint32_t v = (uint32_t)jpk_env_long("JPK_PAIR_KEEP", 50, 0, 100);
    return v;
}
int pair_rule_gap()
{
    static const int v = (int)jpk_env_long("JPK_PAIR_GAP", 3, 2, INT_MAX);
    return v;
}
}  // namespace

PairSchedule::PairSchedule(uint32_t n) : gap(pair_rule_gap()), m_prev(n) {}

bool PairSchedule::step(int round, uint32_t m_now, uint32_t n, bool runs_heavy, bool exact_from_round_1)
{
    if (prev_pair) gap = ((uint64_t)m_now * 100u > (uint64_t)m_prev * pair_rule_keep()) ? 2 * gap + 1 : pair_rule_gap();
    const bool sizeable = pair_rule_shift() >= 0 && m_now >= pair_rule_min() && m_now >= (uint32_t)((uint64_t)n >> pair_rule_shift());
    bool pair = sizeable && round >= PAIR_FROM && round - last_pair >= gap && (uint64_t)m_now * 100u >= (uint64_t)m_prev * pair_rule_ratio();
    // ... and round 2 already when round 1 resolved next to nothing (99 % of its list is still there: periodic data, a block
    // that holds everything twice -- doubling is futile) unless the block is mostly runs, whose groups the run rule is splitting
    if (!pair && round == 2 && exact_from_round_1 && pair_rule_early() && sizeable && !runs_heavy && (uint64_t)m_now * 100u >= (uint64_t)m_prev * 99u) pair = true;
    m_prev = m_now;
    prev_pair = pair;
    if (pair) last_pair = round;
    return pair;
}

// The pair rule (k_pair_*): from round 3 on -- the host knows the exact count there -- a round whose list is still a sizeable share
// of the block is a pair round instead of a doubling round; the doubling distance stays where it was.  Two doubling rounds lie
// between two pair rounds (a group with dissenting pairs has to split before the rule can say more about it).
int sa_pair_round(jpk_ctx *ctx, uint32_t n, SaBufs &b, SaRun &r, int round)
{
    hipStream_t st = ctx->stream;
    const int par = round & 1;
    const unsigned g_win = cap_grid(r.bound, SEG_TILE, CAP);
    // P lives in the sorted suffix numbers of round 0 (read for the last time by k_r0_finish), V | BAD | VL in the key2 buffer
    // (no gather in this round)
    uint32_t *P = r.vs;
    uint8_t *V = reinterpret_cast<uint8_t *>(b.k2), *BAD = V + n, *VL = V + 2 * (size_t)n;
    JPK_HIP(hipMemsetAsync(P, 0, sizeof(uint32_t) * ((size_t)n + 1), st));
    JPK_HIP(hipMemsetAsync(BAD, 0, n, st));
    JPK_HIP(hipMemsetAsync(&b.state->pair_steps, 0, sizeof(uint32_t), st));
    JPK_LAUNCH(ctx, PROF_SA_KEYS, 0, k_pair_dist, dim3(g_win), dim3(TB), b.a_sa, b.a_grp, b.state, par, P, b.FH, b.LH);
    sa_win_scan1(ctx, b, par);
    JPK_LAUNCH(ctx, PROF_SA_KEYS, 0, k_pair_repair, dim3(cap_grid(n, TB * 4, 8192)), dim3(TB), P, n, b.ISA, b.blk, b.bend, b.state, pair_rule_budget(n));
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_pair_first, dim3(cap_grid(n, CT, 4096)), dim3(TB), P, n, b.tB);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_pair_scan, dim3(1), dim3(WG1), b.tB, n);
    JPK_LAUNCH(ctx, PROF_SA_KEYS, 0, k_pair_fill, dim3(cap_grid(n, CT, CAP)), dim3(TB), P, n, b.tB, b.ISA, V, b.blk, b.bend);
    JPK_LAUNCH(ctx, PROF_SA_KEYS, 0, k_pair_mark, dim3(g_win), dim3(TB), b.a_sa, b.a_grp, b.state, par, V, VL, BAD);
    JPK_LAUNCH(ctx, PROF_SA_RERANK, 0, k_pair_finish, dim3(g_win), dim3(TB), b.a_sa, b.a_grp, b.a_prev, b.state, par, b.PH, b.NH, VL, BAD, b.ISA, b.bwt, b.SA,
               b.b_sa, b.b_grp, b.b_prev);
    return JPK_OK;
}

}  // namespace jpk_sa

// host-logic probe (include/jampack_abi.h): the pair-round schedule on recorded lists
extern "C" JPK_API int jpk_debug_pair_schedule(int64_t n, int32_t nrounds, const uint32_t *list, int32_t runs_heavy, int32_t *is_pair)
{
    if (n <= 0 || n >= (int64_t)JPK_FWD_BWT_LIMIT || nrounds < 1 || !list || !is_pair) return JPK_E_ARG;
    PairSchedule sched((uint32_t)n);
    int count = 0;
    is_pair[0] = 0;
    for (int r = 1; r < nrounds; r++) {
        is_pair[r] = list[r] ? (sched.step(r, list[r], (uint32_t)n, runs_heavy != 0, true) ? 1 : 0) : 0;
        count += is_pair[r];
    }
    return count;
}
