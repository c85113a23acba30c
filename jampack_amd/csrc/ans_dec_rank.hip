// ans_dec_rank.hip -- the back of the decoder: RLE0 decode (k_dec_rle: run_rle) and the sorted-rank chains (k_dec_rank, one wave per chunk:
// run_rank).  ans_dec.hpp is what the decoder's units share; the overview and the map of the units are at the top of ans_dec.hip.
#include "ans_dec.hpp"

using namespace jpk;
using namespace jpk_dec;

namespace {

// ---------------------------------------------------------------------------------------------------------------
// RLE0 decode: one workgroup per chunk.  Output is pre-zeroed, so only symbols > 1 are written; a digit group
// contributes value-1 zeros at the position of its last digit (rle.cpp:52-74).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_dec_rle(const DecBlock *__restrict__ blocks, const ChunkInfo *__restrict__ info, uint32_t *__restrict__ status_all)
{
    const uint32_t c = blockIdx.x;
    const ChunkInfo ci = info[c];
    const DecBlock B = blocks[ci.blk];
    const uint16_t *__restrict__ rle = B.rle;
    uint8_t *__restrict__ out = B.ranks;
    uint32_t *status = status_all + ci.blk;
    const uint16_t *src = rle + ci.rle_off;
    uint8_t *dst = out + ci.out_off;
    const uint32_t rlen = ci.rlen, olen = ci.olen;
    __shared__ uint32_t sm[1024 / 64 + 1];
    __shared__ uint32_t carry_s;
    __shared__ uint32_t bad_s;
    if (threadIdx.x == 0) { carry_s = 0; bad_s = 0; }
    __syncthreads();
    for (uint32_t b0 = 0; b0 < rlen; b0 += 1024 * 4) {
        const uint32_t p0 = b0 + threadIdx.x * 4;
        uint32_t cnt[4], val[4];
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t t = p0 + k;
            cnt[k] = 0; val[k] = 0;
            if (t < rlen) {
                const uint32_t sy = src[t];
                if (sy > 256u) atomicOr(&bad_s, 1u);
                if (sy > 1u) { cnt[k] = 1; val[k] = sy - 1u; }
                else if (t + 1 >= rlen || src[t + 1] > 1u) {     // last digit of a group: gather the group backwards
                    uint32_t bits = 0, nb = 0;
                    int64_t u = t;
                    while (u >= 0 && src[u] <= 1u && nb <= 21) { bits |= (uint32_t)src[u] << nb; nb++; u--; }
                    if (nb > 20) atomicOr(&bad_s, 1u);
                    else cnt[k] = ((1u << nb) | bits) - 1u;
                }
            }
            s += cnt[k];
        }
        uint32_t tot;
        uint32_t inc = block_incl_scan<OpSum>(s, sm, &tot);
        uint32_t run = carry_s + inc - s;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (val[k]) { if (run < olen) dst[run] = (uint8_t)val[k]; else atomicOr(&bad_s, 1u); }
            run += cnt[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) carry_s += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0 && (carry_s != olen || bad_s)) atomicOr(status, ST_RLE_MISMATCH);     // rle.cpp:72 "rle mismatch!"
}

// ---------------------------------------------------------------------------------------------------------------
// sorted-rank decode (rank.cpp:96-151): one wave per chunk.
// list: positions 0..63 are one symbol per lane of register L0, so that the common update -- insert at a rank below 64 --
// is one DPP move, one select and one v_writelane.  Positions 64..255 are packed four to a lane in register P (lane l =
// positions 64 + 4l .. 67 + 4l, little endian; lanes 48.. unused): ranks >= 64 (incompressible data) pay a full shift of L0
// plus one branch-free byte shift-insert of P.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_shl1(uint32_t v)        // lane i <- lane i+1, lane 63 <- 0 (no user reads it): one DPP move
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);      // bound_ctrl: no tied old value, no copy
}

// packed register: byte positions < r take the value of position + 1; INSERT: position r takes sym.  Branch-free:
// keep = bytes of this lane at or above position r (two half shifts, so that 4 bytes below r give 0).
template <bool INSERT>
__device__ __forceinline__ uint32_t packed_shift(uint32_t v, int l, uint32_t r, uint32_t sym)
{
    const uint32_t nextv = wave_shl1(v);
    const uint32_t shifted = __builtin_amdgcn_alignbyte(nextv, v, 1);      // (v >> 8) | (nextv << 24)
    const int nb = (int)r - 4 * l;                                          // bytes of this lane below position r
    const uint32_t h = 4u * (uint32_t)(nb < 0 ? 0 : (nb > 4 ? 4 : nb));
    const uint32_t keep = (0xFFFFFFFFu << h) << h;
    uint32_t res = (v & keep) | (shifted & ~keep);
    if (INSERT) {
        const uint32_t ins = ((uint32_t)nb < 4u) ? 0xFFu << (8u * ((uint32_t)nb & 3u)) : 0u;
        res = (res & ~ins) | ((sym * 0x01010101u) & ins);
    }
    return res;
}

// positions < r take the value of position + 1; INSERT: position r takes sym (rank.cpp:131-134), else it keeps its value
// (the front drop of an exhausted bucket, rank.cpp:140-147).  r <= 255.
template <bool INSERT>
__device__ __forceinline__ void list_shift(uint32_t &L0, uint32_t &P, int l, uint32_t r, uint32_t sym)
{
    const uint32_t nxt = wave_shl1(L0);
    if (r < 64u) {
        const uint32_t res = ((uint32_t)l < r) ? nxt : L0;
        L0 = INSERT ? lane_write(res, sym, r) : res;
    } else {
        L0 = lane_write(nxt, rfl(P) & 0xffu, 63u);          // position 63 takes position 64 = byte 0 of P's lane 0
        P = packed_shift<INSERT>(P, l, r - 64u, sym);
    }
}

// Every symbol keeps the next 64 ranks of its bucket in an LDS row, one rank per byte (row[used] = the rank its next
// occurrence reads), so the serial chain never waits for HBM: a run costs one LDS round trip, one ballot and one list
// update.  A row that runs low is topped up by a direct-to-LDS load (global_load_lds_ubyte: lane j's byte lands
// zero-extended in dword j behind the M0 base, no VGPR and therefore no compiler-inserted wait).  Entries past the end of
// a bucket are 0xFF (non-zero: they end the zero run).
//
// The inner loop is the common iteration -- a non-zero rank found inside the safe part of the row, at least 64 bytes of
// output left -- and touches one counter of the row's metadata; everything else (end of a bucket, empty or low rows,
// landing a top-up, the last bytes of the chunk) goes through the general path, which also re-normalises the metadata.
struct RankMeta {
    uint32_t used;      // entries consumed by fast iterations since the last normalisation (the row is read from here on)
    uint32_t fast;      // fast iterations may consume this many entries (as of the last normalisation)
    uint32_t nv;        // known entries in the row (as of the last normalisation)
    uint32_t left;      // ranks of the bucket not yet consumed (as of the last normalisation)
};
struct RankSpan {
    uint32_t gpos;      // offset in R of the first byte not yet requested
    uint32_t gend;      // end of the bucket in R
};
constexpr uint32_t RANK_LOW = 24;          // top a row up when fewer known entries remain

typedef const __attribute__((address_space(1))) void *jpk_gptr;
typedef __attribute__((address_space(3))) void *jpk_lptr;
typedef __attribute__((address_space(1))) uint8_t *jpk_gbytes;

__device__ __forceinline__ uint32_t rank_fast_limit(uint32_t nv, uint32_t left, bool all_loaded)
{
    const uint32_t slack = all_loaded ? 64u : (nv > RANK_LOW ? nv - RANK_LOW : 0u);
    const uint32_t a = nv < left ? nv : left;
    return a < slack ? a : slack;
}

// s_waitcnt lgkmcnt(0): every LDS access issued so far has completed
__device__ __forceinline__ void lds_wait() { __builtin_amdgcn_s_waitcnt(0xc07f); }

__global__ __launch_bounds__(64) void k_dec_rank(const DecBlock *__restrict__ blocks, const ChunkInfo *__restrict__ info, const uint32_t *__restrict__ order,
                                                const int32_t *__restrict__ freq, uint32_t *__restrict__ status_all)
{
    __builtin_amdgcn_s_setprio(3);         // serial chain: win the issue arbitration on a shared SIMD
    const uint32_t c = order ? order[blockIdx.x] : blockIdx.x;
    const int l = lane_id();
    const ChunkInfo ci = info[c];
    const uint32_t len = rfl(ci.olen);
    if (len == 0) return;
    const DecBlock B = blocks[ci.blk];
    const uint8_t *R = B.ranks + ci.out_off;     // rank array
    uint8_t *T = B.out + ci.out_off;             // decoded symbols
    const jpk_gbytes Tg = (jpk_gbytes)T;
    __shared__ uint8_t rows[256][64];             // one byte per rank: 16 KiB
    __shared__ uint32_t stage[64];                // landing zone of the top-up in flight (LDS-DMA writes one dword per lane)
    __shared__ RankMeta meta[256];
    __shared__ RankSpan span[256];
    // 22 784 bytes in all: seven chains per CU (160 KiB).  The frequency table and the start list are only needed until the rows
    // are filled and live in the rows' own memory until then (with their own 2 KiB the kernel took 24.3 KiB: six per CU).
    static_assert(sizeof rows + sizeof stage + sizeof meta + sizeof span == RANK_LDS_BYTES, "RANK_LDS_BYTES (ans_dec.hpp) is this kernel's LDS");
    uint32_t *const sf = reinterpret_cast<uint32_t *>(&rows[0][0]);
    uint32_t *const lst = sf + 256;
    const int32_t *fq = freq + (size_t)c * 256;
    for (int s = l; s < 256; s += 64) { sf[s] = (uint32_t)fq[s]; lst[s] = 0; }
    __syncthreads();
    uint32_t uniq = 0;
    // bucket layout in GenerateSortedMap order; list[R[bucket start]] = symbol (rank.cpp:114-123)
    uint32_t g4[4], e4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = l + 64 * k;
        const uint32_t f = sf[s];
        uint32_t b = 0;
        for (int j = 0; j < 256; j++) { uint32_t fj = sf[j]; if (fj > f || (fj == f && j < s)) b += fj; }
        RankMeta m;
        m.used = 0; m.nv = 64; m.left = f ? f - 1 : 0;
        m.fast = rank_fast_limit(m.nv, m.left, b + 1 + 64 >= b + f);
        meta[s] = m;
        RankSpan sp;
        sp.gpos = b + 1 + 64; sp.gend = b + f;
        span[s] = sp;
        g4[k] = b + 1; e4[k] = b + f;
        if (f > 0) lst[R[b]] = (uint32_t)s;           // a corrupt stream may name a position twice: the last writer wins, as in rank.cpp
        uniq += (f > 0);
    }
    uniq = rfl(wave_sum(uniq));
    __syncthreads();
    uint32_t L0 = lst[l];
    uint32_t P = (l < 48) ? (lst[64 + 4 * l] | (lst[65 + 4 * l] << 8) | (lst[66 + 4 * l] << 16) | (lst[67 + 4 * l] << 24)) : 0u;
    __syncthreads();                               // the start list has been read: its memory becomes rows
    // first window of every bucket (the offsets come from registers so the 256 loads pipeline)
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 64; j++) {
            const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)g4[k], j), ge = (uint32_t)__builtin_amdgcn_readlane((int)e4[k], j);
            rows[j + 64 * k][l] = (g + l < ge) ? R[g + l] : (uint8_t)0xFF;
        }
    __syncthreads();
    uint32_t sym = (uint32_t)__builtin_amdgcn_readlane((int)L0, 0);
    uint32_t psym = 256;                                         // row with a top-up in flight (256 = none)
    uint32_t poff = 0, pcnt = 0;                                 // ... its entries land at rows[psym][poff .. poff + pcnt)
    uint32_t i = 0;
    const uint32_t fast_end = rfl(len >= 64u ? len - 63u : 0u);  // the inner loop stores 64 bytes at i: it runs while i < fast_end
    uint32_t rl = rows[sym][l];                                  // entry `used` is the next unread rank (no wrap between normalisations)
    RankMeta m = meta[sym];
    // The inner loop reads the next symbol's counters before it has counted the current run.  When the next symbol IS the current one
    // they are stale: fend then is 0 for one test, the loop leaves, and the counters are read again.  Only a corrupt stream gets
    // there: list positions that no bucket names hold symbol 0, a rank at or above uniq pulls them forward, and two of them reach
    // the front; in a valid stream positions 0 and 1 differ.  rank.cpp walks the same list, so the answer is defined and has to be
    // the same.  (Two scalar instructions off the chain; anything that branches inside the loop costs 7 % of the kernel.)
    uint32_t fend = fast_end;
    for (;;) {
        // ---- inner loop: z zero ranks, then the real non-zero rank; z + 1 outputs.  The row itself is not touched: these
        // iterations only advance `used` (they never look past the entries known at the last normalisation).  The row and
        // metadata of the NEXT symbol are read before the list update: a run that ends in a non-zero rank always brings the
        // second list entry to the front, whatever the rank is.
        uint32_t big_r = 0, big_sym = 0;                        // a rank >= 64 leaves the loop for its insert (L0 and P), so that
        for (;;) {                                               // the loop itself carries L0 only
            const uint32_t used = rfl(m.used), room = rfl(m.fast) - used;
            const uint64_t nz = __ballot(rl != 0) >> (used & 63u);
            uint32_t z;
            asm("s_ff1_i32_b64 %0, %1" : "=s"(z) : "s"(nz));    // no non-zero entry: -1, which fails the test below
            uint32_t lim;                                        // room, or 0 behind fast_end (select on the scalar unit, no mask logic)
            asm("s_cmp_lt_u32 %1, %2\n\ts_cselect_b32 %0, %3, 0" : "=s"(lim) : "s"(i), "s"(fend), "s"(room) : "scc");
            if (!(z < lim)) break;
            const uint32_t nsym = (uint32_t)__builtin_amdgcn_readlane((int)L0, 1);
            // the rank that ends the run is taken out of the row BEFORE the next row is loaded: the old row's register is dead by
            // then and the load can land in it (no copy per iteration)
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)rl, (int)(used + z));
            const uint32_t nrl = rows[nsym][l];
            const RankMeta nm = meta[nsym];
            // all 64 lanes store: the bytes behind the run are rewritten by the runs that own them (same wave, program order)
            // (issued as asm: the store is never waited for -- nothing in this kernel reads T -- and the compiler's wait-count
            // bookkeeping for the LDS-DMA top-ups would otherwise put a vmcnt(0) in front of the next LDS read)
            asm volatile("global_store_byte %0, %1, %2" : : "v"(i + (uint32_t)l), "v"(sym), "s"(Tg));
            const uint32_t cnt = z + 1u;
            i += cnt;
            meta[sym].used = used + cnt;                         // every lane stores the same word: cheaper than masking to one lane
            const uint32_t cur = sym;
            asm("s_cmp_eq_u32 %1, %2\n\ts_cselect_b32 %0, 0, %3" : "=s"(fend) : "s"(nsym), "s"(cur), "s"(fast_end) : "scc");
            sym = nsym; rl = nrl; m = nm;
            if (__builtin_expect(r >= 64u, 0)) { big_r = r; big_sym = cur; break; }
            const uint32_t nxt = wave_shl1(L0);
            L0 = lane_write(((uint32_t)l < r) ? nxt : L0, cur, r);
        }
        if (big_r) { list_shift<true>(L0, P, l, big_r, big_sym); continue; }
        if (i >= len) break;
        if (fend != fast_end) {                                  // the symbol followed itself: its counters, as the run left them
            fend = fast_end;
            lds_wait();
            m = meta[sym];
            continue;
        }
        // ---- general path ----
        if (psym < 256u) {                                       // land the top-up in flight and unblock its row
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if ((uint32_t)l < pcnt) rows[psym][poff + l] = (uint8_t)stage[l];
            const RankMeta pm = meta[psym];
            const RankSpan ps = span[psym];
            if (l == 0) { meta[psym].nv = 64u; meta[psym].fast = rank_fast_limit(64u, pm.left, ps.gpos >= ps.gend); }
            psym = 256u;
            lds_wait();
            rl = rows[sym][l];                                   // start over with the rows as they are now
            m = meta[sym];
            continue;
        }
        const uint32_t used = rfl(m.used);
        const uint32_t rest = len - i;
        const RankSpan sp = span[sym];
        const uint32_t gpos = rfl(sp.gpos), gend = rfl(sp.gend);
        const uint32_t nv = rfl(m.nv) - used, left = rfl(m.left) - used;
        const uint32_t rlog = rows[sym][(l + used) & 63u];                   // logical order from here on
        const uint32_t rlk = ((uint32_t)l < nv) ? rlog : 0xFFu;             // unknown entries stop the scan
        const uint64_t nzk = __ballot(rlk != 0);
        const uint32_t zk = nzk ? (uint32_t)__builtin_ctzll(nzk) : 64u;
        const bool stop = zk < nv;                                           // a known non-zero entry ended the run
        uint32_t cnt = stop ? zk + 1u : zk;                                  // outputs = ranks consumed
        if (cnt > rest) cnt = rest;
        if ((uint32_t)l < cnt) T[i + l] = (uint8_t)sym;
        i += cnt;
        // normalise: the unread entries move to the front of the row, unknown entries and the tail become 0xFF
        const uint32_t shifted = ((uint32_t)l + cnt < nv) ? rows[sym][(l + used + cnt) & 63u] : 0xFFu;
        const bool all_loaded = gpos >= gend;
        const uint32_t nv2 = all_loaded ? 64u : nv - (cnt < nv ? cnt : nv);
        const uint32_t left2 = left - (cnt < left ? cnt : left);
        const uint32_t cur = sym;
        if (stop) {
            if (zk < left) {
                const uint32_t r = __builtin_amdgcn_readlane(rlk, zk);       // the non-zero rank that ends the run
                list_shift<true>(L0, P, l, r, sym);
                sym = (uint32_t)__builtin_amdgcn_readlane((int)L0, 0);
            } else if (uniq > 0) {                                           // bucket exhausted: drop the front
                uniq--;
                const uint32_t lim = uniq > 0 ? uniq : 1u;                  // rank.cpp:140-147; executes at least once
                list_shift<false>(L0, P, l, lim, 0u);
                sym = (uint32_t)__builtin_amdgcn_readlane((int)L0, 0);
            }
        }
        rows[cur][l] = (uint8_t)shifted;
        RankMeta w;
        w.used = 0; w.nv = nv2; w.left = left2;
        if (!all_loaded && nv2 < RANK_LOW + 8u) {                            // top the row up behind the shifted entries
            const uint32_t want = 64u - nv2;
            lds_wait();                                                      // the shifted row is in LDS before the load may land
            const uint32_t avail = gend - gpos;                              // gpos < gend here
            pcnt = want < avail ? want : avail;
            poff = nv2;
            if ((uint32_t)l < pcnt)
                __builtin_amdgcn_global_load_lds((jpk_gptr)(R + gpos + l), (jpk_lptr)(&stage[0]), 1, 0, 0);
            psym = cur;
            // the known entries stay readable while the top-up is in flight (it lands behind them): the row only stops the
            // inner loop when they run out, and by then the load has had the time of ~24 of this symbol's runs
            w.fast = rank_fast_limit(nv2, left2, true);
            if (l == 0) span[cur].gpos = gpos + want;
        } else {
            w.fast = rank_fast_limit(nv2, left2, all_loaded);
        }
        if (l == 0) meta[cur] = w;
        lds_wait();                                                          // the normalised row and its metadata are in LDS
        rl = rows[sym][l];
        m = meta[sym];
    }
}

}  // namespace

namespace jpk_dec {

int run_rle(jpk_ctx *ctx, const DecBufs &b, unsigned g, uint64_t units)
{
    JPK_LAUNCH(ctx, PROF_DEC_RLE, units, k_dec_rle, dim3(g), dim3(1024), b.tab, b.info, b.status);
    return JPK_OK;
}

// the reservation on top of the kernel's own RANK_LDS_BYTES brings a chain's workgroup to chain_lds
int run_rank(jpk_ctx *ctx, const DecBufs &b, const uint32_t *order, unsigned g, uint64_t units, size_t chain_lds)
{
    const size_t more = chain_lds > RANK_LDS_BYTES ? chain_lds - RANK_LDS_BYTES : 0;
    JPK_LAUNCH_LDS(ctx, PROF_DEC_RANK, units, more, k_dec_rank, dim3(g), dim3(64), b.tab, b.info, order, b.freq, b.status);
    return JPK_OK;
}

}  // namespace jpk_dec
