// bwt_fwd_rounds.hip -- forward BWT, the doubling rounds: key2 of every active suffix, the window / piece bookkeeping, the LDS sort of the
// groups of up to 1024, the segmented radix sort of the larger ones, and the compaction of the survivors (overview: bwt_fwd.hip).
#include "bwt_fwd.hpp"

using namespace jpk;
using namespace jpk_sa;

namespace {

// ---- doubling rounds -------------------------------------------------------------------------------------------------
// key2 of every active suffix + head words per window -> FH / LH = 1 + first / last head position of the window (0: none)
// Run members (RUNF, see the constant).  Among suffixes that start with the same byte c repeated, the order is
//   [run ends in a byte < c, or at the end of the text: ascending run length]  <  [run ends in a byte > c: descending run length]
// (A = c^a x.., B = c^b y.. with a < b differ at offset a: x against c), ties = same kind and length, decided by the suffix behind
// the run.  The invariant of prefix doubling -- at the start of the round with distance h every group shares its first h bytes,
// so every rank read at distance h resolves h more -- must hold for them too:
//   round 1 (h = D, round 0's depth; the group is everything that starts with c^D): the ordinary key2 = rankD(s + D) + 1 already places
//     the members with fewer than 2D equal bytes; those with 2D or more all read the rank G of their own group there.  They get
//     G + 1 + (L for the first kind, 2n - L for the second), keys above G + 1 move up by 2n: one key, every group 2D-ordered.
//   later rounds: a group of run members with L >= 2D has one kind and one run length, so it may compare at distance max(h, L)
//     -- the rank of the suffix behind the run, whatever the run's length: it shares L >= that many bytes (L > h) or is h-ordered
//     like everybody else, and gains >= h either way.  An all-zero block is sorted after round 1.
__global__ __launch_bounds__(TB) void k_gather_win(const uint32_t *__restrict__ a_sa, const uint32_t *__restrict__ a_grp, const SaState *__restrict__ st,
                                                  int par, uint32_t n, int hshift, const uint32_t *__restrict__ ISA, uint32_t *__restrict__ k2,
                                                  uint32_t *__restrict__ FH, uint32_t *__restrict__ LH,
                                                  const uint8_t *__restrict__ T, const uint32_t *__restrict__ RL, int first_round,
                                                  const uint8_t *__restrict__ a_blk, const uint32_t *__restrict__ bend, const uint32_t *__restrict__ GDr)
{
    __shared__ uint64_t H[16];
    const uint32_t m = st->m[par];
    // vmode (variable-length keys; GDr = the depth of every unresolved group by its rank): a group compares at ITS OWN depth -- the
    // symbols its members are known to share -- instead of the round's common distance.  The run rule needs no later-round case then:
    // round 1 gives the members it spreads by (kind, run length) the depth L (k_seg_round / k_lg_finish), so they read the suffix
    // behind their run like everybody reads the suffix behind its depth.
    const bool vmode = GDr != nullptr && st->vmode != 0u;
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    // the round's distance: round 0 resolved `depth` bytes (k_key_plan), every round doubles it
    const uint32_t D = st->depth;
    const uint64_t h64 = (uint64_t)D << hshift;
    const uint32_t h = (hshift < 32 && h64 < n) ? (uint32_t)h64 : n;
    for (uint32_t win = blockIdx.x; win < nwin; win += gridDim.x) {
        const uint32_t base = win * SEG_TILE;
        __syncthreads();
        // every load of the window is issued without a branch around it (clamped indices, results masked afterwards), so that
        // the list reads and then the rank gathers are all in flight together
        uint32_t s[WIN_ITEMS], gj[WIN_ITEMS], gp[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l, jc = j < m ? j : m - 1;
            s[k] = a_sa[jc];
            gj[k] = a_grp[jc];
            gp[k] = a_grp[jc ? jc - 1 : 0];
        }
        uint32_t kv[WIN_ITEMS], lim[WIN_ITEMS];
        bool anyrun = false;
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) lim[k] = n;
        if (bend) {                          // group sort: a suffix ends with its block (the block number rides in the byte array)
#pragma unroll
            for (int k = 0; k < WIN_ITEMS; k++) {
                const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l;
                lim[k] = bend[a_blk[j < m ? j : m - 1]];
            }
        }
        uint32_t hk[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) hk[k] = vmode ? GDr[gj[k] & ~(RUNF | DONE)] : h;      // (vmode: ascending ranks along the list, neighbours share the word)
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint64_t s2 = (uint64_t)s[k] + hk[k];
            kv[k] = ISA[s2 < lim[k] ? s2 : 0];
            kv[k] = (s2 < lim[k]) ? kv[k] + 1u : 0u;
            anyrun |= (gj[k] & RUNF) != 0u;
        }
        if (__ballot(anyrun)) {                                      // wave-uniform and rare: text has few runs of `depth` equal bytes
#pragma unroll
            for (int k = 0; k < WIN_ITEMS; k++) {
                const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l;
                if (j < m && (gj[k] & RUNF)) {
                    const uint32_t G1 = (gj[k] & ~(RUNF | DONE)) + 1u;  // key2 of "the suffix D further is still in my group": 2D equal bytes
                    if (first_round) {
                        // every key keeps its place relative to the group's own rank; the members with >= 2D equal bytes, which
                        // all tie there, are spread over the 2n values behind it by (kind, run length)
                        if (kv[k] == G1) {
                            const uint32_t L = RL[s[k]];
                            const uint64_t e = (uint64_t)s[k] + L;  // first position behind the run
                            const bool down = e >= lim[k] || T[e] < T[s[k]];
                            kv[k] = G1 + (down ? L : 2u * n - L);    // L in [2D, n]: the kinds cannot collide (2n - L >= n >= L, equal only for L = n: one suffix)
                        } else if (kv[k] > G1) kv[k] += 2u * n;
                    } else if (!vmode) {
                        const uint32_t L = RL[s[k]];
                        if (L >= 2u * D && L > h) {                  // (a descendant of a c^D group with a shorter run is an ordinary suffix)
                            const uint64_t e = (uint64_t)s[k] + L;
                            kv[k] = e < lim[k] ? ISA[e] + 1u : 0u;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t j = base + w * (64 * WIN_ITEMS) + k * 64 + l;
            bool head = false;
            if (j < m) {
                head = (j == 0) || (gj[k] != gp[k]);
                k2[j] = kv[k];
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

// Geometry of the (at most two) pieces that groups larger than SEG_TILE cut out of window w: A = the tail of the group that
// spills in, B = the head of the window's last group.  PH = 1 + last head at or before the end of window w, NH = first head
// position after window w (m if none).
__device__ __forceinline__ void win_geometry(uint32_t w, uint32_t m, const uint32_t *FH, const uint32_t *LH, const uint32_t *PH, const uint32_t *NH,
                                             bool &hasA, uint32_t &a_end, uint32_t &a_gs, uint32_t &a_ge, bool &hasB, uint32_t &b_gs, uint32_t &b_ge)
{
    const uint32_t base = w * SEG_TILE;
    const uint32_t wend = (base + SEG_TILE < m) ? base + SEG_TILE : m;
    const uint32_t fh = FH[w], lh = LH[w];
    hasA = (fh != base + 1u);                         // the first slot of the window is not a head (then w > 0: slot 0 is one)
    a_gs = 0; a_ge = 0; a_end = 0;
    if (hasA) {
        a_gs = PH[w - 1] - 1u;
        a_end = fh ? fh - 1u : wend;
        a_ge = fh ? fh - 1u : NH[w];
        hasA = (a_ge - a_gs > (uint32_t)SEG_TILE);
    }
    hasB = (lh != 0u);
    b_gs = 0; b_ge = 0;
    if (hasB) {
        b_gs = lh - 1u;
        b_ge = NH[w];
        hasB = (b_ge - b_gs > (uint32_t)SEG_TILE);
    }
}

// window metadata in four small kernels: (1) one workgroup: PH, NH by scans; (2) all windows: piece counts; (3) one workgroup:
// exclusive prefix of the counts; (4) all windows: piece descriptors
__global__ __launch_bounds__(WG1) void k_win_scan1(const uint32_t *__restrict__ FH, const uint32_t *__restrict__ LH, uint32_t *PH, uint32_t *NH,
                                                  SaState *__restrict__ st, int par)
{
    __shared__ uint32_t sm[WG1 / 64 + 1];
    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    if (threadIdx.x == 0) { st->npieces = 0; st->lc = 0; }
    if (nwin == 0) return;
    wg_scan<OpMax, false, false>(LH, PH, nwin, 0u, sm);
    // NH: exclusive suffix min of the first-head positions (FH holds position + 1, 0 = none)
    for (uint32_t w = threadIdx.x; w < nwin; w += WG1) NH[w] = FH[w] ? FH[w] - 1u : NONE;
    __syncthreads();
    wg_scan<OpMin, true, true>(NH, NH, nwin, m, sm);
}

__global__ __launch_bounds__(TB) void k_win_count(const uint32_t *__restrict__ FH, const uint32_t *__restrict__ LH, const uint32_t *__restrict__ PH,
                                                 const uint32_t *__restrict__ NH, uint32_t *__restrict__ PC, SaState *__restrict__ st, int par)
{
    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    uint32_t lsum = 0;
    for (uint32_t w = blockIdx.x * TB + threadIdx.x; w < nwin; w += gridDim.x * TB) {
        bool hasA, hasB;
        uint32_t a_end, a_gs, a_ge, b_gs, b_ge;
        win_geometry(w, m, FH, LH, PH, NH, hasA, a_end, a_gs, a_ge, hasB, b_gs, b_ge);
        const uint32_t base = w * SEG_TILE;
        const uint32_t wend = (base + SEG_TILE < m) ? base + SEG_TILE : m;
        PC[w] = (hasA ? 1u : 0u) + (hasB ? 1u : 0u);
        lsum += (hasA ? a_end - base : 0u) + (hasB ? wend - b_gs : 0u);
    }
    lsum = wave_sum(lsum);
    if (lane_id() == 0 && lsum) atomicAdd(&st->lc, lsum);
}

__global__ __launch_bounds__(WG1) void k_win_scan2(uint32_t *PC, SaState *__restrict__ st, int par, int round)
{
    __shared__ uint32_t sm[WG1 / 64 + 1];
    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    const uint32_t np = wg_scan<OpSum, true, false>(PC, PC, nwin, 0u, sm);
    if (threadIdx.x == 0) {
        st->npieces = np;
        if (round < JPK_SA_MAX_ROUNDS) st->round_lc[round] = st->lc;
    }
}

__global__ __launch_bounds__(TB) void k_win_pieces(const uint32_t *__restrict__ FH, const uint32_t *__restrict__ LH, const uint32_t *__restrict__ PH,
                                                  const uint32_t *__restrict__ NH, const uint32_t *__restrict__ PC, Piece *__restrict__ pieces,
                                                  const SaState *__restrict__ st, int par)
{
    if (st->npieces == 0) return;
    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    for (uint32_t w = blockIdx.x * TB + threadIdx.x; w < nwin; w += gridDim.x * TB) {
        bool hasA, hasB;
        uint32_t a_end, a_gs, a_ge, b_gs, b_ge;
        win_geometry(w, m, FH, LH, PH, NH, hasA, a_end, a_gs, a_ge, hasB, b_gs, b_ge);
        const uint32_t base = w * SEG_TILE;
        const uint32_t wend = (base + SEG_TILE < m) ? base + SEG_TILE : m;
        uint32_t p = PC[w];
        if (hasA) {
            // the group's first piece is piece B of the window that holds its head
            const uint32_t w0 = a_gs / SEG_TILE;
            bool hA0, hB0;
            uint32_t t0, t1, t2, t3, t4;
            win_geometry(w0, m, FH, LH, PH, NH, hA0, t0, t1, t2, hB0, t3, t4);
            Piece q;
            q.begin = base; q.count = a_end - base; q.gs = a_gs; q.ge = a_ge;
            q.fp = PC[w0] + (hA0 ? 1u : 0u);
            q.nt = (a_ge - 1u) / SEG_TILE - w0 + 1u;
            q.tl = w - w0;
            q.pad = 0;
            pieces[p++] = q;
        }
        if (hasB) {
            Piece q;
            q.begin = b_gs; q.count = wend - b_gs; q.gs = b_gs; q.ge = b_ge;
            q.fp = p;
            q.nt = (b_ge - 1u) / SEG_TILE - w + 1u;
            q.tl = 0;
            q.pad = 0;
            pieces[p] = q;
        }
    }
}

// vmode: the symbols the members of a NEW group share = the old group's depth + the depth of the group their common key2 names (they all
// read the same rank at the old depth: Larsson-Sadakane's invariant per group instead of per round).  Exceptions, round 1 only, in a
// group of run members (RUNF): k_gather_win spread the members with >= 2 d equal bytes over G + 1 + (L | 2n - L) -- such a group shares
// its run, depth L -- and moved the ordinary keys above G + 1 up by 2n.  (A group of one needs no depth; key2 = 0 is always alone.)
__device__ __forceinline__ uint32_t new_group_depth(const uint32_t *__restrict__ GDr, uint32_t G, bool runf, uint32_t key2, bool first_round, uint32_t n)
{
    const uint32_t own = GDr[G];
    uint32_t tr = key2 - 1u;
    if (first_round && runf) {
        const uint32_t G1 = G + 1u;
        if (key2 > G1 && key2 - G1 <= 2u * n) {
            const uint32_t x = key2 - G1;
            return x <= n ? x : 2u * n - x;
        }
        if (key2 > G1) tr -= 2u * n;
    }
    const uint64_t d = (uint64_t)own + GDr[tr];
    return d > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)d;
}

// the sort / re-rank of all groups of <= SEG_TILE elements, one window per workgroup iteration
__global__ __launch_bounds__(TB) void k_seg_round(const uint32_t *__restrict__ a_sa, const uint32_t *__restrict__ a_grp, const uint32_t *__restrict__ k2g,
                                                 const SaState *__restrict__ st, int par, int key_bits, const uint32_t *__restrict__ PH,
                                                 const uint8_t *__restrict__ a_prev, uint32_t *__restrict__ ISA, uint8_t *__restrict__ bwt, uint32_t *__restrict__ SA,
                                                 uint32_t *__restrict__ b_sa, uint32_t *__restrict__ b_grp, uint8_t *__restrict__ b_prev,
                                                 const uint32_t *__restrict__ GDr, uint32_t *__restrict__ GDw, int first_round, uint32_t n)
{
    // LDS diet (30 KB, five workgroups per CU instead of three): the group ranks g[] are only needed while the group boundaries
    // are worked out and share their 8 KB with the two index permutations of the sort; the suffix numbers and the group rank of
    // the final positions are re-read from the (L2-resident) window instead of being kept; the scratch of the boundary scans
    // shares the digit counters' space.
    __shared__ uint32_t u_g_idx[SEG_SPAN];    // phase 1: g[] = group rank per loaded element; afterwards: idxA | idxB (uint16 each)
    __shared__ uint32_t k2[SEG_SPAN];         // sort key of the owned elements
    __shared__ uint16_t gsl[SEG_SPAN];        // group start (local position) per loaded element, 0xFFFF = spill-in
    __shared__ uint16_t lgid[SEG_SPAN];       // local group id of the owned elements
    __shared__ uint16_t cnt[TB / 64][SEG_DIGITS];
    __shared__ uint32_t dbase[SEG_DIGITS];    // also fz | rz of the boundary scans (2 x TB words)
    __shared__ uint32_t sm[TB / 64 + 1];
    __shared__ uint32_t s_fo, s_oe;
    __shared__ uint8_t firstflag[TB + 1];
    uint32_t *const g = u_g_idx;
    uint16_t *const idxA = reinterpret_cast<uint16_t *>(u_g_idx), *const idxB = idxA + SEG_SPAN;
    uint32_t *const fz = dbase, *const rz = dbase + TB;
    static_assert(SEG_DIGITS >= 2 * TB, "fz | rz live in dbase");

    const uint32_t m = st->m[par];
    const uint32_t nwin = (m + SEG_TILE - 1) / SEG_TILE;
    const int tid = threadIdx.x;
    for (uint32_t win = blockIdx.x; win < nwin; win += gridDim.x) {
        __syncthreads();                      // the LDS of the previous window is free
        const uint32_t base = win * SEG_TILE;
        const uint32_t avail = (m - base < (uint32_t)SEG_SPAN) ? m - base : (uint32_t)SEG_SPAN;
        const bool list_ends = (base + avail == m);

        {   // the span's eight loads per thread in flight together (clamped; only slots < avail are kept)
            uint32_t gl[SEG_ITEMS];
#pragma unroll
            for (int k = 0; k < SEG_ITEMS; k++) { const uint32_t p = tid + k * TB; gl[k] = a_grp[base + (p < avail ? p : avail - 1)]; }
#pragma unroll
            for (int k = 0; k < SEG_ITEMS; k++) { const uint32_t p = tid + k * TB; if (p < avail) g[p] = gl[k]; }
        }
        const uint32_t gprev = (base > 0) ? a_grp[base - 1] : 0xFFFFFFFFu;
        if (tid == 0) { s_fo = 0xFFFFFFFFu; s_oe = 0; }
        __syncthreads();

        // ---- group starts (max-scan of head positions) and group ends (next head), blocked 8 per thread ----
        const uint32_t p0 = tid * SEG_ITEMS;
        uint32_t hd = 0;                           // head bits of my 8 positions
        uint32_t lasth = 0;                        // 1 + last head position in my segment
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; k++) {
            uint32_t p = p0 + k;
            if (p < avail) {
                bool head = (p == 0) ? (base == 0 || g[0] != gprev) : (g[p] != g[p - 1]);
                if (head) { hd |= 1u << k; lasth = p + 1; }
            }
        }
        uint32_t incl = block_incl_scan<OpMax>(lasth, sm, nullptr);
        uint32_t prev = __shfl_up(incl, 1, 64);
        if (lane_id() == 0) prev = (tid == 0) ? 0u : sm[(tid >> 6) - 1];
        // next head after my segment: suffix-min over the first-head positions of later threads
        uint32_t firsth = 0xFFFFFFFFu;
#pragma unroll
        for (int k = SEG_ITEMS - 1; k >= 0; k--)
            if (hd & (1u << k)) firsth = p0 + k;
        fz[tid] = firsth;
        __syncthreads();
        uint32_t rv = fz[TB - 1 - tid];
        uint32_t rinc = block_incl_scan<OpMin>(rv, sm, nullptr);
        rz[tid] = rinc;
        __syncthreads();
        uint32_t after = (tid == TB - 1) ? 0xFFFFFFFFu : rz[TB - 2 - tid];
        // per position: group start / end
        uint32_t ge[SEG_ITEMS];
        {
            uint32_t nn = after;
#pragma unroll
            for (int k = SEG_ITEMS - 1; k >= 0; k--) {
                ge[k] = nn;                        // first head strictly after position p0+k (or none)
                if (hd & (1u << k)) nn = p0 + k;
            }
            uint32_t run = prev;                   // 1 + start of the current group, 0 = spill-in
#pragma unroll
            for (int k = 0; k < SEG_ITEMS; k++) {
                uint32_t p = p0 + k;
                if (hd & (1u << k)) run = p + 1;
                if (p < avail) gsl[p] = run ? (uint16_t)(run - 1) : (uint16_t)0xFFFF;
            }
        }
        __syncthreads();
        // ---- classify: size of the group of each position; owned = starts in my window and size <= SEG_TILE.  A group whose
        // end lies beyond the loaded span is larger than SEG_TILE by construction (it starts inside the first half) ----
        const uint32_t ph = (win > 0) ? PH[win - 1] : 0u;                              // 1 + last head before my window
        const uint32_t spill_start = ph > 0 ? ph - 1 : 0u;                              // global index
        uint32_t my_fo = 0xFFFFFFFFu, my_oe = 0;
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; k++) {
            uint32_t p = p0 + k;
            if (p < avail) {
                const uint32_t gs = gsl[p];
                uint32_t end = ge[k];
                bool end_known = true;
                if (end == 0xFFFFFFFFu) { end = avail; end_known = list_ends; }
                uint32_t size;
                if (!end_known) size = 0xFFFFFFFFu;
                else if (gs == 0xFFFFu) size = base + end - spill_start;
                else size = end - gs;
                const bool large = size > (uint32_t)SEG_TILE;
                if (gs != 0xFFFFu && gs < (uint32_t)SEG_TILE && !large) {
                    if (p < my_fo) my_fo = p;
                    if (p + 1 > my_oe) my_oe = p + 1;
                }
            }
        }
        if (my_fo != 0xFFFFFFFFu) { atomicMin(&s_fo, my_fo); atomicMax(&s_oe, my_oe); }
        __syncthreads();
        const uint32_t fo = s_fo, oe = s_oe;
        if (fo == 0xFFFFFFFFu) continue;           // nothing owned (uniform)
        const uint32_t no = oe - fo;               // owned elements: a contiguous range of whole groups

        // ---- stage owned elements: suffix, key2, local group id ----
        // local group id = number of heads in [fo, p] - 1  (block scan over head counts, blocked layout)
        uint32_t hc = 0;
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; k++) {
            uint32_t p = p0 + k;
            if (p >= fo && p < oe && (hd & (1u << k))) hc++;
        }
        uint32_t hinc = block_incl_scan<OpSum>(hc, sm, nullptr);
        {
            uint32_t run = hinc - hc;
#pragma unroll
            for (int k = 0; k < SEG_ITEMS; k++) {
                uint32_t p = p0 + k;
                if (p >= fo && p < oe) {
                    if (hd & (1u << k)) run++;
                    lgid[p - fo] = (uint16_t)(run - 1);
                }
            }
        }
        uint32_t kmax = 0;                         // the window's largest key2: the sort only needs passes over the bits it has
        {
            uint32_t kl[SEG_ITEMS];
#pragma unroll
            for (int k = 0; k < SEG_ITEMS; k++) { const uint32_t q = tid + k * TB; kl[k] = k2g[base + fo + (q < no ? q : no - 1)]; }
#pragma unroll
            for (int k = 0; k < SEG_ITEMS; k++) {
                const uint32_t q = tid + k * TB;
                if (q < no) {
                    k2[q] = kl[k];
                    kmax |= kl[k];
                    idxA[q] = (uint16_t)q;    // g[] is dead from here on (last read: the classification above)
                }
            }
        }
        {
            uint32_t kall;
            block_incl_scan<OpMax>(kmax, sm, &kall);                  // (an OR would do; the maximum of the ORs has the same top bit)
            kmax = kall;
        }
        __syncthreads();
        // key2 <= n needs 27 bits on a 64 MiB block, the host's bound (3 n: round 1 spreads run members) 28 -- and with ten bits of group
        // number that is a fifth 9-bit pass which the window's own largest key usually does not need
        const int key_bits_w = kmax ? 32 - __clz((int)kmax) : 1;
        const int kbw = key_bits_w < key_bits ? key_bits_w : key_bits;
        const uint32_t ngroups = (uint32_t)lgid[no - 1] + 1u;

        // ---- LSD radix sort of the index permutation by the composite key (lgid << kbw) | key2, 9 bits per pass ----
        uint16_t *src = idxA, *dst = idxB;
        const int w = tid >> 6, l = tid & 63;
        const uint64_t lt = lanemask_lt();
        const int gbits = (ngroups > 1u) ? 32 - __clz((int)(ngroups - 1u)) : 0;
        const int npass = (kbw + gbits + SEG_DBITS - 1) / SEG_DBITS;
        // each wave ranks a contiguous quarter of the owned range: only ceil(no / 256) iterations of 64 are live
        const int nit = (int)((no + TB - 1) / TB);
        const uint32_t wspan = (uint32_t)nit * 64u;
        for (int pass = 0; pass < npass; pass++) {
            const int shift = SEG_DBITS * pass;
            const int part = (shift + SEG_DBITS <= kbw) ? 0 : (shift >= kbw ? 2 : 1);   // digit from key2 / both / group id
            for (int i = tid; i < (TB / 64) * SEG_DIGITS / 2; i += TB) reinterpret_cast<uint32_t *>(&cnt[0][0])[i] = 0;
            __syncthreads();
            uint32_t rk[SEG_ITEMS], dg[SEG_ITEMS];
#pragma unroll
            for (int it = 0; it < SEG_ITEMS; it++) {
                if (it >= nit) break;
                const uint32_t q = w * wspan + it * 64 + l;
                const bool valid = q < no;
                const uint32_t id = valid ? src[q] : 0u;
                uint32_t d;
                if (part == 0) d = k2[id] >> shift;
                else if (part == 2) d = (uint32_t)lgid[id] >> (shift - kbw);
                else d = (k2[id] >> shift) | ((uint32_t)lgid[id] << (kbw - shift));
                d = valid ? (d & (uint32_t)(SEG_DIGITS - 1)) : 0u;
                dg[it] = d | (id << SEG_DBITS);
                const uint64_t mm = match_any<SEG_DBITS>(d, valid);
                const uint32_t below = (uint32_t)__popcll(mm & lt);
                const uint32_t c = valid ? cnt[w][d] : 0u;
                rk[it] = c + below;
                if (valid && below == 0) cnt[w][d] = (uint16_t)(c + (uint32_t)__popcll(mm));
            }
            __syncthreads();
            {   // per digit: exclusive over waves, then exclusive over digits (two digits per thread, in digit order)
                uint32_t s2[2];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int d = 2 * tid + e;
                    uint32_t s = 0;
#pragma unroll
                    for (int k = 0; k < TB / 64; k++) { uint32_t t = cnt[k][d]; cnt[k][d] = (uint16_t)s; s += t; }
                    s2[e] = s;
                }
                const uint32_t inc = block_incl_scan<OpSum>(s2[0] + s2[1], sm, nullptr);
                dbase[2 * tid] = inc - s2[0] - s2[1];
                dbase[2 * tid + 1] = inc - s2[1];
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < SEG_ITEMS; it++) {
                if (it >= nit) break;
                const uint32_t q = w * wspan + it * 64 + l;
                if (q < no) {
                    const uint32_t d = dg[it] & (uint32_t)(SEG_DIGITS - 1);
                    dst[dbase[d] + cnt[w][d] + rk[it]] = (uint16_t)(dg[it] >> SEG_DBITS);
                }
            }
            __syncthreads();
            uint16_t *t = src; src = dst; dst = t;
        }

        // ---- re-rank (blocked 8 per thread over the sorted order) ----
        uint32_t ap[SEG_ITEMS], nh[SEG_ITEMS];
        uint32_t hmax = 0;
        // the eight suffixes (and their carried BWT bytes) this thread will place, and the old ranks of its eight positions: all
        // loads issued here, in flight together (clamped), used after the scan below
        uint32_t sv[SEG_ITEMS], og[SEG_ITEMS];
        uint8_t pvv[SEG_ITEMS];
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; k++) {
            const uint32_t q = p0 + k, qc = q < no ? q : no - 1;
            const uint32_t from = base + fo + src[qc];
            sv[k] = a_sa[from];
            pvv[k] = a_prev[from];                                  // T[s - 1] travels with the suffix: no gather from the text
            og[k] = a_grp[base + fo + qc];
        }
        uint32_t rf[SEG_ITEMS];                                     // run-member flag of the group at my positions (rides with the rank)
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; k++) { rf[k] = og[k] & RUNF; og[k] &= ~RUNF; }
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; k++) {
            const uint32_t q = p0 + k;
            ap[k] = 0; nh[k] = 0;
            if (q < no) {
                const uint32_t id = src[q];
                const uint32_t pos = fo + q;                        // groups keep their positions through the sort
                ap[k] = og[k] + (pos - (uint32_t)gsl[pos]);
                bool head = (q == 0);
                if (!head) {
                    const uint32_t pid = src[q - 1];
                    head = (lgid[pid] != lgid[id]) || (k2[pid] != k2[id]);
                }
                nh[k] = head ? 1u : 0u;
                if (head) hmax = ap[k];
            }
        }
        uint32_t rincl = block_incl_scan<OpMax>(hmax, sm, nullptr);
        uint32_t rprev = __shfl_up(rincl, 1, 64);
        if (lane_id() == 0) rprev = (tid == 0) ? 0u : sm[(tid >> 6) - 1];
        // next-head flag of the element after my segment
        firstflag[tid] = (uint8_t)(nh[0] | (p0 >= no ? 1u : 0u));
        if (tid == 0) firstflag[TB] = 1;
        __syncthreads();
        uint32_t run = rprev;
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; k++) {
            const uint32_t q = p0 + k;
            if (q < no) {
                if (nh[k]) run = ap[k];
                const bool next_head = (q + 1 >= no) ? true : (k + 1 < SEG_ITEMS ? (nh[k + 1] != 0) : (firstflag[tid + 1] != 0));
                const bool single = nh[k] && next_head;
                const uint32_t s = sv[k];
                const uint8_t pv = pvv[k];
                if (GDw && nh[k] && !single) GDw[run] = new_group_depth(GDr, og[k], rf[k] != 0u, k2[src[q]], first_round != 0, n);   // vmode: the depth of the new group
                if (run != og[k]) ISA[s] = run;                     // the sub-group that sorts first keeps the old group's rank: no store
                if (single) {
                    bwt[ap[k]] = pv;
                    if (SA) SA[ap[k]] = s;
                }
                b_sa[base + fo + q] = s;
                b_grp[base + fo + q] = run | (single ? DONE : 0u) | rf[k];
                b_prev[base + fo + q] = pv;
            }
        }
    }
}

// ---- large groups: segmented LSD radix sort in place on (key2, sa), tiles = pieces -----------------------------------------
// table layout: entry of (group, digit d, piece t of the group) = fp * NB + d * nt + t  -- group-major in list order, so the flat
// exclusive scan S gives  S[entry] - S[fp * NB] = offset inside the group
template <int DB>
__global__ __launch_bounds__(TB) void k_lg_hist(const uint32_t *__restrict__ key, const Piece *__restrict__ pieces, const SaState *__restrict__ st, int shift,
                                               uint32_t *__restrict__ table)
{
    constexpr int NB = 1 << DB;
    // the members of one group share the upper digits of their keys (ranks inside one old group): counted by wave match -- the
    // lanes with equal digits are found by ballots and one of them adds their number to the wave's counter (plain LDS
    // read-modify-write, one lane per address) -- instead of LDS atomics that serialise on the shared bins
    __shared__ uint32_t h[WAVES * NB];
    const uint32_t np = st->npieces;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    uint32_t *mine = h + w * NB;
    const uint64_t lt = lanemask_lt();
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const Piece q = pieces[p];
        __syncthreads();
        for (int i = threadIdx.x; i < WAVES * NB; i += TB) h[i] = 0;
        __syncthreads();
        uint32_t kv[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {                // loads first (clamped), then the LDS atomics
            const uint32_t e = w * (64 * WIN_ITEMS) + k * 64 + l;
            kv[k] = key[q.begin + (e < q.count ? e : q.count - 1)];
        }
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t e = w * (64 * WIN_ITEMS) + k * 64 + l;
            const bool valid = e < q.count;
            const uint32_t d = (kv[k] >> shift) & (uint32_t)(NB - 1);
            const uint64_t m = match_any<DB>(d, valid);
            if (valid && (m & lt) == 0ull) mine[d] += (uint32_t)__popcll(m);
        }
        __syncthreads();
        for (int d = threadIdx.x; d < NB; d += TB) {
            uint32_t s = 0;
#pragma unroll
            for (int k = 0; k < WAVES; k++) s += h[k * NB + d];
            table[(size_t)q.fp * NB + (size_t)d * q.nt + q.tl] = s;
        }
    }
}

template <int DB>
__global__ __launch_bounds__(TB) void k_lg_scatter(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin, const uint8_t *__restrict__ pin,
                                                  uint32_t *__restrict__ kout, uint32_t *__restrict__ vout, uint8_t *__restrict__ pout,
                                                  const Piece *__restrict__ pieces, const SaState *__restrict__ st, int shift, const uint32_t *__restrict__ S)
{
    constexpr int NB = 1 << DB;
    __shared__ uint32_t cnt[WAVES][NB];
    __shared__ uint32_t gbase[NB];
    const uint32_t np = st->npieces;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint64_t lt = lanemask_lt();
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const Piece q = pieces[p];
        __syncthreads();
        for (int i = threadIdx.x; i < WAVES * NB; i += TB) (&cnt[0][0])[i] = 0;
        const uint32_t s0 = S[(size_t)q.fp * NB];
        for (int d = threadIdx.x; d < NB; d += TB) gbase[d] = q.gs + (S[(size_t)q.fp * NB + (size_t)d * q.nt + q.tl] - s0);
        __syncthreads();
        uint32_t key[WIN_ITEMS], val[WIN_ITEMS], rnk[WIN_ITEMS];
        uint8_t prv[WIN_ITEMS];                      // the suffix's BWT byte rides along (third member of the sorted record)
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {                // the piece's loads in flight together (clamped; masked by `valid` below)
            const uint32_t e = w * (64 * WIN_ITEMS) + k * 64 + l, ec = q.begin + (e < q.count ? e : q.count - 1);
            key[k] = kin[ec];
            val[k] = vin[ec];
            prv[k] = pin[ec];
        }
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t e = w * (64 * WIN_ITEMS) + k * 64 + l;
            const bool valid = e < q.count;
            if (!valid) key[k] = 0u;
            const uint32_t d = (key[k] >> shift) & (uint32_t)(NB - 1);
            const uint64_t mm = match_any<DB>(d, valid);
            const uint32_t below = (uint32_t)__popcll(mm & lt);
            const uint32_t c = valid ? cnt[w][d] : 0u;
            rnk[k] = c + below;
            if (valid && below == 0) cnt[w][d] = c + (uint32_t)__popcll(mm);
        }
        __syncthreads();
        for (int d = threadIdx.x; d < NB; d += TB) {
            uint32_t s = 0;
#pragma unroll
            for (int k = 0; k < WAVES; k++) { uint32_t t = cnt[k][d]; cnt[k][d] = s; s += t; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const uint32_t e = w * (64 * WIN_ITEMS) + k * 64 + l;
            if (e < q.count) {
                const uint32_t d = (key[k] >> shift) & (uint32_t)(NB - 1);
                const uint32_t dst = gbase[d] + cnt[w][d] + rnk[k];
                kout[dst] = key[k];
                vout[dst] = val[k];
                pout[dst] = prv[k];
            }
        }
    }
}

// head words of a piece in the sorted order: a new group starts where key2 changes (and at the group's first slot);
// H[16] bit 0 = the slot after the piece starts a group (or the old group ends there)
__device__ __forceinline__ void lg_piece_heads(const uint32_t *__restrict__ key, const Piece &q, uint64_t *H)
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    uint32_t kj[WIN_ITEMS], kp[WIN_ITEMS];
#pragma unroll
    for (int k = 0; k < WIN_ITEMS; k++) {                    // loads first (clamped), all in flight
        const uint32_t e = w * (64 * WIN_ITEMS) + k * 64 + l, j = q.begin + (e < q.count ? e : q.count - 1);
        kj[k] = key[j];
        kp[k] = key[j > q.gs ? j - 1 : j];
    }
#pragma unroll
    for (int k = 0; k < WIN_ITEMS; k++) {
        const uint32_t e = w * (64 * WIN_ITEMS) + k * 64 + l;
        bool head = false;
        if (e < q.count) {
            const uint32_t j = q.begin + e;
            head = (j == q.gs) || (kj[k] != kp[k]);
        }
        const uint64_t b = __ballot(head);
        if (l == 0) H[w * WIN_ITEMS + k] = b;
    }
    if (threadIdx.x == 0) {
        const uint32_t jn = q.begin + q.count;
        H[16] = (jn >= q.ge || key[jn] != key[jn - 1]) ? 1ull : 0ull;
    }
}

// 1 + position of the last new head inside every piece (0: none)
__global__ __launch_bounds__(TB) void k_lg_heads(const uint32_t *__restrict__ key, const Piece *__restrict__ pieces, const SaState *__restrict__ st,
                                                uint32_t *__restrict__ pLast)
{
    __shared__ uint64_t H[17];
    const uint32_t np = st->npieces;
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const Piece q = pieces[p];
        __syncthreads();
        lg_piece_heads(key, q, H);
        __syncthreads();
        if (threadIdx.x < 64) {
            const int l = threadIdx.x;
            const uint64_t hv = (l < 16) ? H[l] : 0ull;
            uint32_t last = hv ? q.begin + l * 64 + top_bit(hv) + 1u : 0u;
            last = wave_incl_max(last);
            if (l == 63) pLast[p] = last;
        }
    }
}

__global__ __launch_bounds__(WG1) void k_lg_scan(uint32_t *__restrict__ pLast, const SaState *__restrict__ st)
{
    __shared__ uint32_t sm[WG1 / 64 + 1];
    wg_scan<OpMax, true, false>(pLast, pLast, st->npieces, 0u, sm);
}

// new ranks of the members of large groups -> ISA, finished suffixes -> BWT byte, everything back to the b-list
__global__ __launch_bounds__(TB) void k_lg_finish(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, const uint8_t *__restrict__ prv,
                                                 const uint32_t *__restrict__ a_grp,
                                                 const Piece *__restrict__ pieces, const SaState *__restrict__ st, const uint32_t *__restrict__ pCarry,
                                                 uint32_t *__restrict__ ISA, uint8_t *__restrict__ bwt, uint32_t *__restrict__ SA,
                                                 uint32_t *__restrict__ b_sa, uint32_t *__restrict__ b_grp, uint8_t *__restrict__ b_prev,
                                                 const uint32_t *__restrict__ GDr, uint32_t *__restrict__ GDw, int first_round, uint32_t n)
{
    __shared__ uint64_t H[17];
    __shared__ uint32_t LHW[16];
    const uint32_t np = st->npieces;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const Piece q = pieces[p];
        __syncthreads();
        lg_piece_heads(key, q, H);
        __syncthreads();
        const uint32_t carry = pCarry[p];
        if (threadIdx.x < 64) {
            const uint64_t hv = (l < 16) ? H[l] : 0ull;
            uint32_t last = hv ? q.begin + l * 64 + top_bit(hv) + 1u : 0u;
            last = wave_incl_max(last);
            if (l < 16) LHW[l] = last > carry ? last : carry;
        }
        __syncthreads();
        const uint32_t G0 = a_grp[q.gs];
        const uint32_t G = G0 & ~(DONE | RUNF);            // rank of the old group = SA position of its first member
        const uint32_t rf = G0 & RUNF;                     // run-member flag: rides with the rank
        uint32_t sl[WIN_ITEMS];
        uint8_t pl[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {              // the piece's loads in flight together (clamped)
            const uint32_t e = (w * WIN_ITEMS + k) * 64 + l, j = q.begin + (e < q.count ? e : q.count - 1);
            sl[k] = val[j];
            pl[k] = prv[j];
        }
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; k++) {
            const int word = w * WIN_ITEMS + k;
            const uint32_t e = word * 64 + l;
            if (e < q.count) {
                const uint32_t j = q.begin + e;
                const uint64_t hv = H[word];
                const uint64_t le = hv & mask_upto(l);
                const uint32_t hp = le ? q.begin + word * 64 + top_bit(le) : (word ? LHW[word - 1] : carry) - 1u;
                const uint32_t rank = G + (hp - q.gs);
                const bool head = (hv >> l) & 1ull;
                bool nh;
                if (e + 1 == q.count) nh = H[16] & 1ull;
                else nh = (l < 63) ? ((hv >> (l + 1)) & 1ull) : (H[word + 1] & 1ull);
                const bool single = head && nh;
                const uint32_t s = sl[k];
                const uint8_t pv = pl[k];
                if (GDw && head && !single) GDw[rank] = new_group_depth(GDr, G, rf != 0u, key[j], first_round != 0, n);   // vmode: the depth of the new group
                if (hp != q.gs) ISA[s] = rank;                      // the first sub-group keeps the old group's rank
                if (single) {
                    const uint32_t ap = G + (j - q.gs);
                    bwt[ap] = pv;
                    if (SA) SA[ap] = s;
                }
                b_sa[j] = s;
                b_grp[j] = rank | (single ? DONE : 0u) | rf;
                b_prev[j] = pv;
            }
        }
    }
}

// ---- flat exclusive scan of the piece tables (size known on the device only) ---------------------------------------------
__global__ __launch_bounds__(TB) void k_tab_reduce(const uint32_t *__restrict__ in, const SaState *__restrict__ st, uint32_t nb, uint32_t *__restrict__ partial)
{
    __shared__ uint32_t sm[TB / 64 + 1];
    const size_t n = (size_t)st->npieces * nb;
    const size_t ntiles = (n + SC_TILE - 1) / SC_TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t base = tile * SC_TILE + (size_t)threadIdx.x * SC_ITEMS;
        uint32_t acc = 0;
        if (base + SC_ITEMS <= n) {
            const uint4 *p = reinterpret_cast<const uint4 *>(in + base);
#pragma unroll
            for (int k = 0; k < SC_ITEMS / 4; k++) { uint4 v = p[k]; acc += v.x + v.y + v.z + v.w; }
        } else {
            for (int k = 0; k < SC_ITEMS; k++) if (base + k < n) acc += in[base + k];
        }
        uint32_t tot;
        block_incl_scan<OpSum>(acc, sm, &tot);
        if (threadIdx.x == 0) partial[tile] = tot;
        __syncthreads();
    }
}
__global__ __launch_bounds__(WG1) void k_tab_partials(uint32_t *__restrict__ partial, const SaState *__restrict__ st, uint32_t nb)
{
    __shared__ uint32_t sm[WG1 / 64 + 1];
    const size_t n = (size_t)st->npieces * nb;
    wg_scan<OpSum, true, false>(partial, partial, (uint32_t)((n + SC_TILE - 1) / SC_TILE), 0u, sm);
}
__global__ __launch_bounds__(TB) void k_tab_down(const uint32_t *in, uint32_t *out, const SaState *__restrict__ st, uint32_t nb, const uint32_t *__restrict__ partial)
{
    __shared__ uint32_t sm[TB / 64 + 1];
    const size_t n = (size_t)st->npieces * nb;
    const size_t ntiles = (n + SC_TILE - 1) / SC_TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t base = tile * SC_TILE + (size_t)threadIdx.x * SC_ITEMS;
        uint32_t v[SC_ITEMS];
        if (base + SC_ITEMS <= n) {
            const uint4 *p = reinterpret_cast<const uint4 *>(in + base);
#pragma unroll
            for (int k = 0; k < SC_ITEMS / 4; k++) { uint4 q = p[k]; v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w; }
        } else {
#pragma unroll
            for (int k = 0; k < SC_ITEMS; k++) v[k] = (base + k < n) ? in[base + k] : 0u;
        }
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < SC_ITEMS; k++) acc += v[k];
        const uint32_t inc = block_incl_scan<OpSum>(acc, sm, nullptr);
        uint32_t prev = __shfl_up(inc, 1, 64);
        if (lane_id() == 0) prev = (threadIdx.x == 0) ? 0u : sm[(threadIdx.x >> 6) - 1];
        uint32_t run = partial[tile] + prev;
        uint32_t o[SC_ITEMS];
#pragma unroll
        for (int k = 0; k < SC_ITEMS; k++) { o[k] = run; run += v[k]; }
        if (base + SC_ITEMS <= n) {
            uint4 *p = reinterpret_cast<uint4 *>(out + base);
#pragma unroll
            for (int k = 0; k < SC_ITEMS / 4; k++) p[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < SC_ITEMS; k++) if (base + k < n) out[base + k] = o[k];
        }
        __syncthreads();
    }
}

// ---- compaction of a round's output: the unresolved suffixes, in order, become the next round's active list -------------
__global__ __launch_bounds__(TB) void k_cmp_count(const uint32_t *__restrict__ b_grp, const SaState *__restrict__ st, int par, uint32_t *__restrict__ tSurv)
{
    const uint32_t m = st->m[par];
    const uint32_t ntiles = (m + CT - 1) / CT;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __shared__ uint32_t ws[WAVES];
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * CT;
        uint32_t c = 0;
        uint32_t gv[CT_ITEMS];
#pragma unroll
        for (int k = 0; k < CT_ITEMS; k++) {                // loads first, all in flight (clamped, masked below)
            const uint32_t j = base + w * (64 * CT_ITEMS) + k * 64 + l;
            gv[k] = b_grp[j < m ? j : m - 1];
        }
#pragma unroll
        for (int k = 0; k < CT_ITEMS; k++) {
            const uint32_t j = base + w * (64 * CT_ITEMS) + k * 64 + l;
            c += (j < m && !(gv[k] & DONE)) ? 1u : 0u;
        }
        c = wave_sum(c);
        __syncthreads();
        if (l == 0) ws[w] = c;
        __syncthreads();
        if (threadIdx.x == 0) tSurv[tile] = ws[0] + ws[1] + ws[2] + ws[3];
    }
}
__global__ __launch_bounds__(WG1) void k_cmp_scan(uint32_t *__restrict__ tSurv, SaState *__restrict__ st, int par, int round)
{
    __shared__ uint32_t sm[WG1 / 64 + 1];
    const uint32_t m = st->m[par];
    const uint32_t total = wg_scan<OpSum, true, false>(tSurv, tSurv, (m + CT - 1) / CT, 0u, sm);
    if (threadIdx.x == 0) {
        st->m[par ^ 1] = total;
        if (round + 1 < JPK_SA_MAX_ROUNDS) st->round_m[round + 1] = total;
    }
}
__global__ __launch_bounds__(TB) void k_cmp_scatter(const uint32_t *__restrict__ b_sa, const uint32_t *__restrict__ b_grp, const uint8_t *__restrict__ b_prev,
                                                   const SaState *__restrict__ st, int par, const uint32_t *__restrict__ tOff,
                                                   uint32_t *__restrict__ a_sa, uint32_t *__restrict__ a_grp, uint8_t *__restrict__ a_prev)
{
    __shared__ uint64_t SV[64];
    __shared__ uint32_t SW[64];
    const uint32_t m = st->m[par];
    const uint32_t ntiles = (m + CT - 1) / CT;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * CT;
        __syncthreads();
        uint32_t gv[CT_ITEMS], sv[CT_ITEMS];
        uint8_t pv[CT_ITEMS];
#pragma unroll
        for (int k = 0; k < CT_ITEMS; k++) {                // every load of the tile in flight at once (clamped, masked below)
            const uint32_t j = base + w * (64 * CT_ITEMS) + k * 64 + l, jc = j < m ? j : m - 1;
            gv[k] = b_grp[jc];
            sv[k] = b_sa[jc];
            pv[k] = b_prev[jc];
        }
#pragma unroll
        for (int k = 0; k < CT_ITEMS; k++) {
            const uint32_t j = base + w * (64 * CT_ITEMS) + k * 64 + l;
            if (j >= m) gv[k] = DONE;
            const uint64_t b = __ballot(!(gv[k] & DONE));
            if (l == 0) SV[w * CT_ITEMS + k] = b;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const uint32_t cnt = (uint32_t)__popcll(SV[l]);
            const uint32_t inc = wave_incl_sum(cnt);
            SW[l] = tOff[tile] + inc - cnt;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CT_ITEMS; k++) {
            const int word = w * CT_ITEMS + k;
            if (!(gv[k] & DONE)) {
                const uint32_t pos = SW[word] + (uint32_t)__popcll(SV[word] & mask_below(l));
                a_sa[pos] = sv[k];
                a_grp[pos] = gv[k];
                a_prev[pos] = pv[k];
            }
        }
    }
}

}  // namespace

namespace jpk_sa {

namespace {
int lg_digit_bits(uint32_t n, int *npass)
{
    const int kbits = jpk_bits_for(3u * n);        // key2 <= n, or <= 3n in a group of run members in round 1
    int np = (kbits + 7) / 8;
    if (np < 1) np = 1;
    int db = (kbits + np - 1) / np;
    if (db < 4) db = 4;
    *npass = np;
    return db;                                     // 4..8
}

template <int DB>
void launch_lg_pass(jpk_ctx *ctx, SaBufs &b, const uint32_t *kin, const uint32_t *vin, const uint8_t *pin, uint32_t *kout, uint32_t *vout, uint8_t *pout, int shift,
                    unsigned gp, unsigned gt)
{
    constexpr uint32_t NB = 1u << DB;
    JPK_LAUNCH(ctx, PROF_LG_HIST, 0, (k_lg_hist<DB>), dim3(gp), dim3(TB), kin, b.pieces, b.state, shift, b.table);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_tab_reduce, dim3(gt), dim3(TB), b.table, b.state, NB, b.partial);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_tab_partials, dim3(1), dim3(WG1), b.partial, b.state, NB);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_tab_down, dim3(gt), dim3(TB), b.table, b.table, b.state, NB, b.partial);
    JPK_LAUNCH(ctx, PROF_LG_SCATTER, 0, (k_lg_scatter<DB>), dim3(gp), dim3(TB), kin, vin, pin, kout, vout, pout, b.pieces, b.state, shift, b.table);
}
}  // namespace

void sa_win_scan1(jpk_ctx *ctx, SaBufs &b, int par)
{
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_win_scan1, dim3(1), dim3(WG1), b.FH, b.LH, b.PH, b.NH, b.state, par);
}

void sa_doubling_round(jpk_ctx *ctx, const uint8_t *T, uint32_t n, SaBufs &b, SaRun &r, int round)
{
    const int par = round & 1;
    const int kbits = jpk_bits_for(3u * n);        // key2 <= n (a rank + 1); round 1 spreads the keys of groups of run members up to 3n; group rank < n
    int lg_pass = 0;
    const int lg_db = lg_digit_bits(n, &lg_pass);
    const unsigned g_win = cap_grid(r.bound, SEG_TILE, CAP);
    const unsigned g_seg = cap_grid(r.bound, SEG_TILE, CAP_SEG);
    const size_t pc_bound = 2 * ((size_t)r.bound / SEG_TILE + 1);
    // (the large-group kernels walk the pieces with a grid stride.  The bound is two pieces per window of the list -- 131 K workgroups
    // in round 1, of which text uses a few hundred: 21 us per launch to start and retire the rest, 0.3 ms per block.  The grid is capped
    // at JPK_LG_GRID (default 8192; 0 = the bound) unless the block is known to be mostly large groups -- runs, all-zero: there a
    // workgroup per piece is worth 4-7 %)
    static const unsigned lg_cap = [] { const long v = jpk_env_long("JPK_LG_GRID", 8192, 0); return v ? (unsigned)v : CAP; }();
    const unsigned g_pc = cap_grid(pc_bound, 1, r.lg_heavy ? CAP : lg_cap);
    const unsigned g_tab = cap_grid(pc_bound << lg_db, SC_TILE, CAP);
    // (the groups' depths exist only when k_key_final chose a variable-length code: with the fixed-width code nothing wrote GD[0], and
    // every new group would cost two random reads of uninitialised memory and a random write nobody uses -- ADVICE r5)
    const uint32_t *gdr = r.vmode_h ? b.GD[r.gd] : nullptr;
    uint32_t *gdw = r.vmode_h ? b.GD[r.gd ^ 1] : nullptr;
    JPK_LAUNCH(ctx, PROF_SA_KEYS, 0, k_gather_win, dim3(g_win), dim3(TB), b.a_sa, b.a_grp, b.state, par, n, r.hshift, b.ISA, b.k2, b.FH, b.LH, T, b.RL, round == 1 ? 1 : 0,
               b.a_prev, b.bend, gdr);
    r.hshift++;
    r.gd ^= 1;
    const unsigned g_wm = cap_grid((size_t)r.bound / SEG_TILE + 1, TB, 256);
    sa_win_scan1(ctx, b, par);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_win_count, dim3(g_wm), dim3(TB), b.FH, b.LH, b.PH, b.NH, b.PC, b.state, par);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_win_scan2, dim3(1), dim3(WG1), b.PC, b.state, par, round);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_win_pieces, dim3(g_wm), dim3(TB), b.FH, b.LH, b.PH, b.NH, b.PC, b.pieces, b.state, par);
    JPK_LAUNCH(ctx, PROF_SA_SEG, 0, k_seg_round, dim3(g_seg), dim3(TB), b.a_sa, b.a_grp, b.k2, b.state, par, kbits, b.PH, b.a_prev, b.ISA, b.bwt, b.SA,
               b.b_sa, b.b_grp, b.b_prev, gdr, gdw, round == 1 ? 1 : 0, n);
    if (r.large_possible) {   // large groups: lg_pass LSD passes over (key2, sa), ping-pong between (k2, a_sa) and (k2alt, sa_alt)
        uint32_t *kin = b.k2, *vin = b.a_sa, *kout = b.k2alt, *vout = b.sa_alt;
        uint8_t *pin = b.a_prev, *pout = b.p_alt;
        for (int p = 0; p < lg_pass; p++) {
            const int shift = p * lg_db;
            switch (lg_db) {
            case 4: launch_lg_pass<4>(ctx, b, kin, vin, pin, kout, vout, pout, shift, g_pc, g_tab); break;
            case 5: launch_lg_pass<5>(ctx, b, kin, vin, pin, kout, vout, pout, shift, g_pc, g_tab); break;
            case 6: launch_lg_pass<6>(ctx, b, kin, vin, pin, kout, vout, pout, shift, g_pc, g_tab); break;
            case 7: launch_lg_pass<7>(ctx, b, kin, vin, pin, kout, vout, pout, shift, g_pc, g_tab); break;
            default: launch_lg_pass<8>(ctx, b, kin, vin, pin, kout, vout, pout, shift, g_pc, g_tab); break;
            }
            uint32_t *tk = kin; kin = kout; kout = tk;
            uint32_t *tv = vin; vin = vout; vout = tv;
            uint8_t *tp = pin; pin = pout; pout = tp;
        }
        JPK_LAUNCH(ctx, PROF_SA_RERANK, 0, k_lg_heads, dim3(g_pc), dim3(TB), kin, b.pieces, b.state, b.pLast);
        JPK_LAUNCH(ctx, PROF_SCAN, 0, k_lg_scan, dim3(1), dim3(WG1), b.pLast, b.state);
        JPK_LAUNCH(ctx, PROF_SA_RERANK, 0, k_lg_finish, dim3(g_pc), dim3(TB), kin, vin, pin, b.a_grp, b.pieces, b.state, b.pLast, b.ISA, b.bwt, b.SA, b.b_sa,
                   b.b_grp, b.b_prev, gdr, gdw, round == 1 ? 1 : 0, n);
    }
}

// compaction of the survivors of either kind of round: the b-list back into the a-list
int sa_compact(jpk_ctx *ctx, SaBufs &b, const SaRun &r, int round)
{
    const int par = round & 1;
    const unsigned g_cmp = cap_grid(r.bound, CT, CAP);
    JPK_LAUNCH(ctx, PROF_SA_RERANK, 0, k_cmp_count, dim3(g_cmp), dim3(TB), b.b_grp, b.state, par, b.tA);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_cmp_scan, dim3(1), dim3(WG1), b.tA, b.state, par, round);
    JPK_LAUNCH(ctx, PROF_SA_RERANK, 0, k_cmp_scatter, dim3(g_cmp), dim3(TB), b.b_sa, b.b_grp, b.b_prev, b.state, par, b.tA, b.a_sa, b.a_grp, b.a_prev);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

}  // namespace jpk_sa
