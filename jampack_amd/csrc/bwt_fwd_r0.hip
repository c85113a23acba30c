// bwt_fwd_r0.hip -- forward BWT, round 0's sort and finish: the radix sort of the packed keys, the kernels that turn the sorted pairs into
// ranks and the first active list, and the run rule's remaining run lengths (overview: bwt_fwd.hip).
#include "bwt_fwd.hpp"

using namespace jpk;
using namespace jpk_sa;

namespace {

// ---- round 0 ---------------------------------------------------------------------------------------------------------
// Round 0 sorts slot j = suffix n-1-j by key = first D bytes (as codes, see above), big-endian in bits 63..8, zero padded past the
// end of the text (k_pack_keys built the keys).  The LSD sort is stable, so suffixes that tie on the padded
// bytes come out in DESCENDING text position, i.e. a short suffix (a proper prefix of everything it ties with) lands in
// front -- plain suffix order even when the text contains 0x00 -- and the low byte of the key needs no sort pass.

// head of an equal-key run; a suffix with fewer than D bytes is always a group of its own
// Group sort (bend != null: several blocks sorted as one text, the key's low byte = block number, see radix.hip): the whole key
// takes part in the comparison, and a suffix is "short" when fewer than D bytes are left in ITS block.
__device__ __forceinline__ uint32_t r0_end(uint64_t key, uint32_t n, const uint32_t *__restrict__ bend) { return bend ? bend[(uint32_t)key & 255u] : n; }
// vmode (variable-length keys): the sorted value carries the key's depth in its upper bits (from SaState::tag_shift up) and a
// suffix is "short" (a group of its own) when its depth reaches the end of the text: every symbol it has is in the key
// (in vmode the parameter D of the helpers below is the tag shift, not a depth)
// Blocks above 2^28 bytes (round 6; format.hpp:22 allows 1000 MiB): a 29- or 30-bit suffix number leaves no room for a depth, so the tag
// shift is 32 -- nothing rides in the value -- and the depth of suffix s is read from the slots' own array, Dx[n - 1 - s] (slot j holds
// suffix n - 1 - j; sa_layout gives the array a buffer of its own there).  Only a suffix within 63 symbols of its end can be short, so
// the heads cost no extra read; what does is the depth of every unresolved group (one random byte per group head, k_r0_finish).
__device__ __forceinline__ bool r0_short(uint32_t v, uint64_t key, uint32_t n, const uint32_t *__restrict__ bend, uint32_t D, bool vmode,
                                         const uint8_t *__restrict__ Dx = nullptr)
{
    if (vmode && Dx) {
        const uint32_t e = r0_end(key, n, bend);
        return (uint64_t)v + 63u >= e && v + Dx[n - 1u - v] >= e;
    }
    return vmode ? (v & ((1u << D) - 1u)) + (v >> D) >= r0_end(key, n, bend) : v + D > r0_end(key, n, bend);
}
__device__ __forceinline__ bool r0_head(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sa, uint32_t j, uint32_t n, const uint32_t *__restrict__ bend,
                                        uint32_t D, bool vmode, const uint8_t *__restrict__ Dx)
{
    if (j == 0) return true;
    const uint64_t a = keys[j], b = keys[j - 1];
    return ((a ^ b) >> (bend ? 0 : 8)) != 0ull || r0_short(sa[j], a, n, bend, D, vmode, Dx) || r0_short(sa[j - 1], b, n, bend, D, vmode, Dx);   // bits 7..0 carry T[sa-1], not key
}

// head words of one 4096-slot tile: HE[word] = heads | slots past the end (so that "the next slot is a head" is one shift),
// HE[64] bit 0 = head flag of the first slot of the next tile.  Every thread loads its sixteen (key, suffix) pairs ONCE, all loads
// in flight together (clamped indices, no branch around a load), and hands them back to the caller; the key in front of a slot
// comes from the neighbouring lane (DPP wave shift; lane 0: lane 63 of the row before, the wave's first row: one extra load),
// and "the suffix in front is shorter than D bytes" is the shifted ballot of the row's own "short" bits.
// (vmode: sj[] comes back WITH the depth tag in its upper bits)
__device__ __forceinline__ void r0_tile_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sa, uint32_t n, uint32_t base, uint64_t *HE,
                                              uint64_t (&kj)[CT_ITEMS], uint32_t (&sj)[CT_ITEMS], const uint32_t *__restrict__ bend, uint32_t D, bool vmode,
                                              const uint8_t *__restrict__ Dx)
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint32_t j0 = base + w * (64 * CT_ITEMS);
#pragma unroll
    for (int k = 0; k < CT_ITEMS; k++) {
        const uint32_t j = j0 + k * 64 + l, jc = j < n ? j : n - 1;
        kj[k] = keys[jc];
        sj[k] = sa[jc];
    }
    // the pair in front of the wave's first slot (uniform)
    const uint32_t jb = (j0 && j0 <= n) ? j0 - 1 : 0;
    const uint64_t kb = keys[jb];
    const uint32_t sb = sa[jb];
    uint32_t plo = (uint32_t)kb, phi = (uint32_t)(kb >> 32);
    uint64_t carry_short = (j0 && r0_short(sb, kb, n, bend, D, vmode, Dx)) ? 1ull : 0ull;
    const int low_shift = bend ? 0 : 8;                                              // bits 7..0 carry T[sa-1], not key -- or the block number, which is key
#pragma unroll
    for (int k = 0; k < CT_ITEMS; k++) {
        const uint32_t j = j0 + k * 64 + l;
        const uint32_t lo = (uint32_t)kj[k], hi = (uint32_t)(kj[k] >> 32);
        const uint32_t qlo = (uint32_t)__builtin_amdgcn_update_dpp((int)plo, (int)lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        const uint32_t qhi = (uint32_t)__builtin_amdgcn_update_dpp((int)phi, (int)hi, 0x138, 0xf, 0xf, false);
        const bool differs = (((lo ^ qlo) >> low_shift) | (hi ^ qhi)) != 0u;
        const uint64_t S = __ballot(r0_short(sj[k], kj[k], n, bend, D, vmode, Dx));      // a suffix with fewer than `depth` bytes is a group of its own
        const uint64_t b = __ballot(differs || j >= n || j == 0) | S | (S << 1) | carry_short;
        if (l == 0) HE[w * CT_ITEMS + k] = b;
        carry_short = S >> 63;
        plo = (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
        phi = (uint32_t)__builtin_amdgcn_readlane((int)hi, 63);
    }
    if (threadIdx.x == 0) {
        const uint32_t jn = base + CT;
        HE[64] = (jn >= n || r0_head(keys, sa, jn, n, bend, D, vmode, Dx)) ? 1ull : 0ull;
    }
}
__device__ __forceinline__ uint64_t valid_word(uint32_t word_base, uint32_t n)
{
    if (word_base >= n) return 0ull;
    const uint32_t left = n - word_base;
    return left >= 64u ? ~0ull : ((1ull << left) - 1ull);
}

// per tile: 1 + position of its last head (0: none), number of suffixes that stay unresolved
__global__ __launch_bounds__(TB) void k_r0_count(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sa, uint32_t n,
                                                uint32_t *__restrict__ tLast, uint32_t *__restrict__ tSurv, const uint32_t *__restrict__ bend,
                                                const SaState *__restrict__ st, const uint8_t *__restrict__ Dx)
{
    __shared__ uint64_t HE[65];
    const uint32_t ntiles = (n + CT - 1) / CT;
    const bool vmode = st->vmode != 0u;
    const uint32_t D = vmode ? st->tag_shift : st->depth;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * CT;
        __syncthreads();
        uint64_t kj[CT_ITEMS];
        uint32_t sj[CT_ITEMS];
        r0_tile_heads(keys, sa, n, base, HE, kj, sj, bend, D, vmode, Dx);
        __syncthreads();
        if (threadIdx.x < 64) {
            const int l = threadIdx.x;
            const uint64_t he = HE[l], vm = valid_word(base + l * 64, n);
            const uint64_t hv = he & vm;
            const uint64_t nexth = (he >> 1) | (HE[l + 1] << 63);
            const uint64_t single = hv & nexth;
            uint32_t cnt = (uint32_t)__popcll(vm & ~single);
            uint32_t last = hv ? base + l * 64 + top_bit(hv) + 1u : 0u;
            cnt = wave_sum(cnt);
            last = wave_incl_max(last);
            if (l == 63) { tSurv[tile] = cnt; tLast[tile] = last; }
        }
    }
}

// one workgroup: carry-in head per tile (exclusive prefix max), output offset per tile (exclusive prefix sum), total -> state
__global__ __launch_bounds__(WG1) void k_r0_scan(uint32_t *__restrict__ tLast, uint32_t *__restrict__ tSurv, uint32_t n, SaState *__restrict__ st)
{
    __shared__ uint32_t sm[WG1 / 64 + 1];
    const uint32_t ntiles = (n + CT - 1) / CT;
    wg_scan<OpMax, true, false>(tLast, tLast, ntiles, 0u, sm);
    const uint32_t total = wg_scan<OpSum, true, false>(tSurv, tSurv, ntiles, 0u, sm);
    if (threadIdx.x == 0) {
        st->m[1] = total;
        st->round_m[0] = n;
        st->round_m[1] = total;
        st->npieces = 0;
        st->lc = 0;
    }
}

// group rank (= index of the run head) -> ISA; singletons are finished: BWT byte at their SA position (and SA itself for the
// suffix-array probe); the rest is compacted into the active list
__global__ __launch_bounds__(TB) void k_r0_finish(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sa, uint32_t n,
                                                 const uint32_t *__restrict__ tCarry, const uint32_t *__restrict__ tOff,
                                                 uint32_t *__restrict__ ISA, uint8_t *__restrict__ bwt, uint32_t *__restrict__ SA,
                                                 uint32_t *__restrict__ a_sa, uint32_t *__restrict__ a_grp, uint8_t *__restrict__ a_prev, SaState *__restrict__ st,
                                                 const uint32_t *__restrict__ bend, uint32_t *__restrict__ GD, uint64_t *lb_status, uint32_t *lb_ticket,
                                                 const uint8_t *__restrict__ Dx)
{
    // lb_status != null (round 5): ONE pass -- the tile learns the survivors in front of it and the last head in front of it by decoupled
    // look-back over the tiles before it (ticket order; one 64-bit word per tile = flag | survivors << 31 | 1 + last head, agent-scope
    // atomics; a wave looks at 64 predecessors at a time) instead of from k_r0_count + k_r0_scan, which read the sorted pairs once more.
    __shared__ uint32_t s_tile, s_carry;
    __shared__ uint64_t HE[65];
    __shared__ uint64_t runkey[256];       // vmode: the key of a run of byte b, and the byte whose code starts a key's first 8 bits
    __shared__ uint64_t runsorted[256];    // ... and the run keys of the occurring bytes in byte order = ascending (codes above 8 bits: binary search)
    __shared__ uint16_t vtop[256];
    __shared__ uint32_t s_sigma;
    __shared__ uint64_t SV[64];            // survivor bits per word
    __shared__ uint32_t LHW[64];           // 1 + last head position at or before the end of word l (carry included; the two-pass form)
    __shared__ uint32_t LHL[64];           // ... inside the tile only (0: none yet)
    __shared__ uint32_t SW[64];            // output position of the first survivor of word l
    const uint32_t ntiles = (n + CT - 1) / CT;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const bool vmode = st->vmode != 0u;
    const uint32_t D = vmode ? st->tag_shift : st->depth, code_shift = 56u - st->bits;
    const uint64_t rep = st->rep;
    const uint32_t TAGM = (vmode && !Dx) ? (1u << D) - 1u : 0xFFFFFFFFu;       // (Dx: blocks above 2^28 bytes, no tag in the value -- r0_short)
    if (vmode) {
        runkey[threadIdx.x] = st->vrunkey[threadIdx.x];
        vtop[threadIdx.x] = st->vtop[threadIdx.x];
        runsorted[threadIdx.x] = ~0ull;
        __syncthreads();
        if (st->present[threadIdx.x]) runsorted[st->lut[threadIdx.x]] = runkey[threadIdx.x];     // lut = the byte's index among the occurring ones
        if (threadIdx.x == 255) s_sigma = (uint32_t)st->lut[255] + (st->present[255] ? 1u : 0u);
    }
    constexpr uint64_t LB_AGG = 1ull << 62, LB_PFX = 2ull << 62, LB_LO = (1ull << 31) - 1ull;
    for (uint32_t it = blockIdx.x; it < ntiles; it += gridDim.x) {
        __syncthreads();                                                // (s_tile / s_carry / s_off of the previous tile have been read)
        if (lb_status && threadIdx.x == 0) s_tile = atomicAdd(lb_ticket, 1u);
        __syncthreads();
        const uint32_t tile = lb_status ? s_tile : it;                  // look-back: tiles in the order their workgroups START
        const uint32_t base = tile * CT;
        uint64_t kj[CT_ITEMS];
        uint32_t sj[CT_ITEMS];
        r0_tile_heads(keys, sa, n, base, HE, kj, sj, bend, D, vmode, Dx);
        __syncthreads();
        uint32_t carry = lb_status ? 0u : tCarry[tile];
        uint32_t nrun = 0;
        // one slot of the tile.  PHASE 0: everything at once (the two-pass comparator: carry and offsets are known up front).  Look-back form,
        // round 6: PHASE 1 = what needs nothing from the tiles in front -- the rank store (the block's one 64 Mi-element random write), the
        // BWT byte and the depth of every slot whose group's head lies INSIDE the tile -- issued while wave 0 is still looking back; PHASE 2 =
        // the rest: the survivors' list entries (their positions start at the survivors in front of the tile) and the slots in front of the
        // tile's first head (their group's head is the last head in front of the tile).
        auto slot = [&](int k, int phase) {
            const int word = w * CT_ITEMS + k;
            const uint32_t j = base + word * 64 + l;
            if (j >= n) return;
            const uint64_t hv = HE[word] & valid_word(base + word * 64, n);
            const uint64_t le = hv & mask_upto(l);
            // 1 + the head of my group if it lies inside the tile (0: in front of it)
            const uint32_t local = le ? base + word * 64 + top_bit(le) + 1u : (word ? (phase == 0 ? LHW[word - 1] : LHL[word - 1]) : 0u);
            const bool inside = phase == 0 || local != 0u;
            if (phase == 1 && !inside) return;
            const uint32_t grp = (local ? local : carry) - 1u;
            const uint32_t s = sj[k] & TAGM;                        // (loaded once, by r0_tile_heads)
            const uint8_t pv = (uint8_t)kj[k];                      // T[s - 1], carried in the key's low byte since pass 0 (group sort: the block number)
            const uint64_t sv = SV[word];
            const bool survivor = (sv >> l) & 1ull;
            if (phase != 2 || !inside) {                            // (phase 2 repeats nothing phase 1 has stored)
                ISA[s] = grp;
                if (!survivor) {
                    bwt[j] = pv;
                    if (SA) SA[j] = s;
                } else if (vmode && ((HE[word] >> l) & 1ull)) GD[grp] = Dx ? (uint32_t)Dx[n - 1u - s] : sj[k] >> D;      // the group's depth, written by its first member
            }
            if (phase == 1 || !survivor) return;
            const uint32_t pos = SW[word] + (uint32_t)__popcll(sv & mask_below(l));
            // `depth` equal bytes (a survivor has all of them: short suffixes are groups of their own): a run member
            const uint64_t k7 = kj[k] >> 8;
            bool inrun;
            if (vmode) {
                // the key of a run is a function of its byte; the byte is the one whose code starts the key: a table on the
                // key's first 8 bits for codes up to 8 bits, a binary search over the (ascending) run keys for the rare longer ones
                const uint32_t c = vtop[(uint32_t)(k7 >> 48)];
                if (c != 0xFFFFu) inrun = k7 == runkey[c];
                else {
                    uint32_t lo = 0, hi = s_sigma;
                    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (runsorted[mid] < k7) lo = mid + 1u; else hi = mid; }
                    inrun = lo < s_sigma && runsorted[lo] == k7;
                }
            } else inrun = k7 == (k7 >> code_shift) * rep;
            nrun += inrun ? 1u : 0u;
            a_sa[pos] = s;
            a_grp[pos] = grp | (inrun ? RUNF : 0u);
            a_prev[pos] = pv;
        };
        uint32_t cnt = 0, inc = 0, last = 0;                            // (wave 0: survivors of my word, their running sum, 1 + last head so far in the tile)
        if (threadIdx.x < 64) {
            const uint64_t he = HE[l], vm = valid_word(base + l * 64, n);
            const uint64_t hv = he & vm;
            const uint64_t nexth = (he >> 1) | (HE[l + 1] << 63);
            const uint64_t surv = vm & ~(hv & nexth);
            SV[l] = surv;
            cnt = (uint32_t)__popcll(surv);
            inc = wave_incl_sum(cnt);
            last = hv ? base + l * 64 + top_bit(hv) + 1u : 0u;
            last = wave_incl_max(last);
            LHL[l] = last;
        }
        if (!lb_status) {
            if (threadIdx.x < 64) {
                SW[l] = tOff[tile] + inc - cnt;
                LHW[l] = last > carry ? last : carry;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < CT_ITEMS; k++) slot(k, 0);
        } else {
            uint32_t cnt_tile = 0, last_tile = 0;
            if (threadIdx.x < 64) {                                     // the aggregate leaves before anything else
                cnt_tile = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
                last_tile = (uint32_t)__builtin_amdgcn_readlane((int)last, 63);
                const uint64_t mine = ((uint64_t)cnt_tile << 31) | last_tile;
                if (l == 0) __hip_atomic_store(lb_status + tile, (tile == 0 ? LB_PFX : LB_AGG) | mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();                                            // SV, LHL
            if (threadIdx.x < 64) {
                uint32_t o_acc = 0, c_acc = 0;
                if (tile != 0) {
                    int64_t pos = (int64_t)tile - 1;                    // lane l looks at tile pos - l
                    for (;;) {
                        const int64_t t = pos - l;
                        uint64_t wv;
                        uint64_t need;                                  // lanes up to the first prefix
                        bool found;
                        for (;;) {
                            wv = t >= 0 ? __hip_atomic_load(lb_status + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : LB_PFX;
                            const uint64_t pf = __ballot((wv >> 62) == 2ull), np = __ballot((wv >> 62) == 0ull);
                            found = pf != 0ull;
                            need = found ? mask_upto((int)__builtin_ctzll(pf)) : ~0ull;
                            if ((np & need) == 0ull) break;            // everybody between me and the first prefix has published
                            __builtin_amdgcn_s_sleep(1);
                        }
                        const bool in = (need >> l) & 1ull;
                        uint32_t so = in ? (uint32_t)((wv >> 31) & LB_LO) : 0u, sc = in ? (uint32_t)(wv & LB_LO) : 0u;
                        so = wave_sum(so);
                        sc = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(sc), 63);
                        o_acc += so;
                        c_acc = c_acc > sc ? c_acc : sc;
                        if (found) break;                              // a prefix was among them (tiles before tile 0 count as one; lane 63's too)
                        pos -= 64;
                    }
                    const uint32_t lt = c_acc > last_tile ? c_acc : last_tile;
                    if (l == 0) __hip_atomic_store(lb_status + tile, LB_PFX | ((uint64_t)(o_acc + cnt_tile) << 31) | lt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                SW[l] = o_acc + inc - cnt;
                if (l == 0) {
                    s_carry = c_acc;
                    if (tile + 1 == ntiles) {                           // the last tile knows the total: what k_r0_scan leaves in the state
                        st->m[1] = o_acc + cnt_tile;
                        st->round_m[0] = n;
                        st->round_m[1] = o_acc + cnt_tile;
                        st->npieces = 0;
                        st->lc = 0;
                    }
                }
            }
            // phase 1: waves 1..3 at once, wave 0 behind its look-back (its prefix is out before its own stores)
#pragma unroll
            for (int k = 0; k < CT_ITEMS; k++) slot(k, 1);
            __syncthreads();                                            // SW, s_carry
            carry = s_carry;
#pragma unroll
            for (int k = 0; k < CT_ITEMS; k++) slot(k, 2);
        }
        if (__ballot(nrun != 0)) {                                   // (rare: text has few runs that long)
            nrun = wave_sum(nrun);
            if (l == 0) atomicAdd(&st->nrun, nrun);
        }
    }
}

// ---- run lengths (only when round 0 left run members behind: every kernel returns at once otherwise) -------------------
// RL[i] = number of bytes equal to T[i] from i on (the remaining length of the run i lies in) = (next position whose byte differs
// from its successor) + 1 - i.  Per 4096-byte tile: first boundary position; suffix-min over the tiles; fill.
__device__ __forceinline__ bool run_ends_at(const uint8_t *__restrict__ T, const uint8_t *__restrict__ blk, uint32_t i, uint32_t n)
{
    return i + 1 == n || T[i] != T[i + 1] || (blk && blk[i] != blk[i + 1]);        // (group sort: a run stops at the end of its block)
}
__global__ __launch_bounds__(TB) void k_run_first(const uint8_t *__restrict__ T, uint32_t n, const SaState *__restrict__ st, uint32_t *__restrict__ tFirst,
                                                 const uint8_t *__restrict__ blk)
{
    if (st->nrun == 0) return;
    __shared__ uint32_t sm[TB / 64 + 1];
    const uint32_t ntiles = (n + CT - 1) / CT;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * CT;
        uint32_t first = NONE;
#pragma unroll
        for (int k = CT_ITEMS - 1; k >= 0; k--) {
            const uint32_t i = base + k * TB + threadIdx.x;
            if (i < n && run_ends_at(T, blk, i, n)) first = i;
        }
        uint32_t tot;
        block_incl_scan<OpMin>(first, sm, &tot);
        if (threadIdx.x == 0) tFirst[tile] = tot;
        __syncthreads();
    }
}
__global__ __launch_bounds__(WG1) void k_run_scan(uint32_t *__restrict__ tFirst, uint32_t n, const SaState *__restrict__ st)
{
    if (st->nrun == 0) return;
    __shared__ uint32_t sm[WG1 / 64 + 1];
    // tFirst[tile] <- first boundary in any LATER tile (exclusive suffix min); position n - 1 is always a boundary
    wg_scan<OpMin, true, true>(tFirst, tFirst, (n + CT - 1) / CT, NONE, sm);
}
__global__ __launch_bounds__(TB) void k_run_fill(const uint8_t *__restrict__ T, uint32_t n, const SaState *__restrict__ st, const uint32_t *__restrict__ tAfter,
                                                uint32_t *__restrict__ RL, const uint8_t *__restrict__ blk)
{
    if (st->nrun == 0) return;
    __shared__ uint32_t sm[TB / 64 + 1];
    const uint32_t ntiles = (n + CT - 1) / CT;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * CT, p0 = base + threadIdx.x * CT_ITEMS;        // blocked: sixteen consecutive positions per thread
        uint32_t bits = 0, first = NONE;
#pragma unroll
        for (int k = CT_ITEMS - 1; k >= 0; k--) {
            const uint32_t i = p0 + k;
            if (i < n && run_ends_at(T, blk, i, n)) { bits |= 1u << k; first = i; }
        }
        // first boundary in the segments of the threads AFTER me: inclusive min-scan over the threads in reverse order
        __shared__ uint32_t rv[TB];
        __syncthreads();                                                              // rv of the previous tile has been read
        rv[TB - 1 - threadIdx.x] = first;
        __syncthreads();
        const uint32_t rinc = block_incl_scan<OpMin>(rv[threadIdx.x], sm, nullptr);   // index u: min over the threads >= TB - 1 - u
        __syncthreads();
        rv[threadIdx.x] = rinc;
        __syncthreads();
        uint32_t nb = (threadIdx.x == TB - 1) ? NONE : rv[TB - 2 - threadIdx.x];
        if (nb == NONE) nb = tAfter[tile];
#pragma unroll
        for (int k = CT_ITEMS - 1; k >= 0; k--) {
            const uint32_t i = p0 + k;
            if (bits & (1u << k)) nb = i;
            if (i < n) RL[i] = nb + 1u - i;
        }
    }
}

}  // namespace

namespace jpk_sa {

namespace {
// JPK_R0_LOOKBACK=0: round 0's head / survivor bookkeeping in two passes (k_r0_count + k_r0_scan in front of k_r0_finish: the comparator)
bool r0_lookback()
{
    static const bool v = jpk_env_long("JPK_R0_LOOKBACK", 1) != 0;
    return v;
}
}  // namespace

int sa_round0_sort(jpk_ctx *ctx, uint32_t n, SaBufs &b, SaRun &r)
{
    hipStream_t st = ctx->stream;
    const bool var = b.GD[0] != nullptr;            // (sa_layout: var_keys_eligible)
    r.ks = b.keysA;
    r.vs = b.valsA;
    // whole tiles for the one-pass radix sort (the pack kernels have filled the pad slots): no pass needs a second, one-workgroup launch
    // for a partial last tile (seven per block, 200-360 us each in the timed loop)
    const uint32_t n_sort = jpk_radix_onesweep() ? (uint32_t)(((size_t)n + CT - 1) / CT * CT) : n;
    const bool tagless = var && var_tag_shift(n) >= 32;        // blocks above 2^28 bytes: nothing rides in the value (r0_short)
    JPK_TRY(jpk_radix_sort_slot_keys(ctx, n_sort, b.keysA, b.valsA, b.keysB, b.valsB, b.scratch, &r.ks, &r.vs, b.blk != nullptr, tagless ? (const uint8_t *)nullptr : b.D0, tagless ? 26 : var_tag_shift(n), n));
    r.Dx = tagless ? b.D0 : (const uint8_t *)nullptr;
    ctx->stats.sa_sorted_elems += n;
    // The sorted pairs sit in (ks, vs).  The other pair of radix buffers is free from here on, the pair that holds the result
    // once k_r0_finish has read it: the doubling rounds live in them.
    uint64_t *ks = r.ks;
    uint32_t *vs = r.vs;
    uint64_t *kfree = (ks == b.keysA) ? b.keysB : b.keysA;
    uint32_t *vfree = (vs == b.valsA) ? b.valsB : b.valsA;
    b.b_sa = vfree;
    b.b_grp = reinterpret_cast<uint32_t *>(kfree);
    b.k2 = reinterpret_cast<uint32_t *>(kfree) + n;
    b.k2alt = reinterpret_cast<uint32_t *>(ks);
    b.sa_alt = reinterpret_cast<uint32_t *>(ks) + n;

    const unsigned g_ct = cap_grid(n, CT, CAP);
    if (r0_lookback()) {
        // one pass over the sorted pairs: the radix sort's scratch (free from here on) holds one status word per tile and the ticket
        uint64_t *lb_status = reinterpret_cast<uint64_t *>(b.scratch);
        const size_t ntiles0 = ((size_t)n + CT - 1) / CT;
        uint32_t *lb_ticket = reinterpret_cast<uint32_t *>(lb_status + ntiles0 + 1);
        JPK_HIP(hipMemsetAsync(lb_status, 0, sizeof(uint64_t) * (ntiles0 + 2), st));
        JPK_LAUNCH(ctx, PROF_SA_RERANK, n, k_r0_finish, dim3(g_ct), dim3(TB), ks, vs, n, b.tA, b.tB, b.ISA, b.bwt, b.SA, b.a_sa, b.a_grp, b.a_prev, b.state, b.bend, b.GD[0],
                   lb_status, lb_ticket, r.Dx);
    } else {
        JPK_LAUNCH(ctx, PROF_SA_RERANK, n, k_r0_count, dim3(g_ct), dim3(TB), ks, vs, n, b.tA, b.tB, b.bend, b.state, r.Dx);
        JPK_LAUNCH(ctx, PROF_SCAN, 0, k_r0_scan, dim3(1), dim3(WG1), b.tA, b.tB, n, b.state);
        JPK_LAUNCH(ctx, PROF_SA_RERANK, n, k_r0_finish, dim3(g_ct), dim3(TB), ks, vs, n, b.tA, b.tB, b.ISA, b.bwt, b.SA, b.a_sa, b.a_grp, b.a_prev, b.state, b.bend, b.GD[0],
                   (uint64_t *)nullptr, (uint32_t *)nullptr, r.Dx);
    }
    return JPK_OK;
}

// remaining run lengths (the caller: only if round 0 left members of runs of >= depth equal bytes behind)
void sa_run_lengths(jpk_ctx *ctx, const uint8_t *T, uint32_t n, SaBufs &b)
{
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_run_first, dim3(cap_grid(n, CT, 4096)), dim3(TB), T, n, b.state, b.tA, b.blk);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_run_scan, dim3(1), dim3(WG1), b.tA, n, b.state);
    JPK_LAUNCH(ctx, PROF_SCAN, 0, k_run_fill, dim3(cap_grid(n, CT, 4096)), dim3(TB), T, n, b.state, b.tA, b.RL, b.blk);
}

}  // namespace jpk_sa
