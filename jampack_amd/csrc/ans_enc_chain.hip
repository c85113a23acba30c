// ans_enc_chain.hip -- rANS encoder, the back half (ans.cpp:189-208, 272-285): the step records, the four sequential chains per chunk,
// the emitted bytes and their positions, headers, output offsets and the placement of everything into the output (overview: ans_enc.hip).
#include "ans_enc.hpp"

using namespace jpk;
using namespace jpk_enc;

namespace {

// rANS records in coding order.  Pair j = 2t (exponent) / 2t+1 (mantissa) belongs to state lane j & 3; the
// records are stored lane-major (rec[lane][j >> 2]) so that every lane streams its own array.  A record is
// {low | freq << 16, Alverson reciprocal of freq}: x / freq == mulhi(x, rcp) >> (ceil(log2 freq) - 1) for x < 2^31.
// 16-byte record {xmax, rcp, bias, cmpl | shift << 20}: everything a step needs that does not depend on the state
// is computed here, in parallel (ryg's RansEncSymbolInit, rans_byte.hpp:188-246, restated for 16-bit frequencies):
//   x / freq == mulhi(x, rcp) >> shift  with rcp = ceil(2^(31+s) / freq), s = ceil(log2 freq), shift = s - 1 (x < 2^31);
//   freq == 1: rcp = 2^32 - 1, shift = 0 gives q = x - 1, compensated by bias += 65535.
// (Round 6 tried the reciprocal from a 256 KB table of the 65 536 frequencies instead of the two 32-bit divisions per record -- ~70 vector
// instructions, eight per thread of k_pairs: 133 -> 169 us per launch, profiles/r06_entropy_ab.txt.  The kernel waits for its three
// dependent waves of loads, not for its vector work; the table read is a fourth.  Not kept.)
__device__ __forceinline__ uint4 rans_record(uint32_t lo, uint32_t fr)
{
    uint32_t rcp, shift, bias = lo;
    if (fr >= 2) {
        const int sh = 32 - __clz((int)(fr - 1));
        // ceil(2^(sh+31) / fr) without a 64-bit division: D = fr << (16 - sh) lies in (2^15, 2^16], 2^(sh+31) / fr == 2^47 / D, and
        // 2^47 = 2^16 * (qh * D + rh)  =>  quotient = (qh << 16) + (rh << 16) / D   (rh < D <= 2^16: everything fits 32 bits)
        const uint32_t D = fr << (16 - sh);
        const uint32_t qh = 0x80000000u / D, rh = 0x80000000u - qh * D;
        const uint32_t ql = (rh << 16) / D, rem = (rh << 16) - ql * D;
        rcp = (qh << 16) + ql + (rem ? 1u : 0u);
        shift = (uint32_t)(sh - 1);
    } else {
        rcp = 0xFFFFFFFFu; shift = 0; bias = lo + 65535u;
    }
    return make_uint4(fr << 15, rcp, bias, (65536u - fr) | (shift << 24));
}

// Two symbols per thread (round 5): symbols 2g and 2g + 1 are the pairs 4g .. 4g + 3, i.e. index g of all four lane arrays -- a wave writes
// 1 KiB runs of each -- and the loads of the two symbols (RLE0 symbol, two history entries or a table row each) are in flight together:
// the kernel waited for its loads three quarters of the time with one symbol per thread.
__global__ __launch_bounds__(TB) void k_pairs(const uint16_t *__restrict__ rle, size_t rle_stride, EncDims d, const uint32_t *__restrict__ rlen,
                                             const uint16_t *__restrict__ exph, const uint32_t *__restrict__ mantad,
                                             const uint32_t *__restrict__ ord, const uint32_t *__restrict__ qcdf, uint4 *__restrict__ recs,
                                             uint32_t *__restrict__ pairs_plain)
{
    const uint32_t c = chunk_of(d, blockIdx.y);
    const uint32_t g = blockIdx.x * TB + threadIdx.x, t0 = 2u * g;
    const uint32_t rl = rlen[c];
    const size_t lane_stride = lane_stride_of(d, c, rle_stride), lb = lane_base(d, c, rle_stride);
    uint4 *rc = recs + lb;
    // the chain kernel walks whole rounds of its sixteen-batch ring (256 steps): steps past a chain's last pair get identity records
    // (xmax above every state, q * 0 + x + 0), so that it needs no bounds logic -- at most 271 per chain, written by the threads
    // behind the chunk's last symbol
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t t = t0 + (uint32_t)h;
        if (t >= rl) {
            const uint32_t u = t - rl;
            if (u < 4u * 288u) {
                const uint32_t np = 2u * rl, chain = u / 288u;
                const uint32_t steps_pad = np ? (((np - 1u) >> 2) / 256u + 1u) * 256u : 256u;
                const uint32_t first = (chain < np) ? ((np - 1u - chain) >> 2) + 1u : 0u;
                const uint32_t k = first + u % 288u;
                if (k < steps_pad) rc[(size_t)chain * lane_stride + k] = make_uint4(0x80000000u, 0u, 0u, 0u);
            }
        }
    }
    if (t0 >= rl) return;
    const bool two = t0 + 1u < rl;
    const size_t cs = sym_stride(d, c, rle_stride), o = sym_base(d, c, rle_stride) + t0;
    const uint16_t *hrow = exph + 7 * sym_base(d, c, rle_stride) + t0;
    uint32_t sy[2], l0[2], h0[2], l1[2], f1[2], aux[2];
    int ee[2];
    // first wave of loads: the two RLE0 symbols (one aligned word when the pair is whole)
    sy[0] = rle[(size_t)c * rle_stride + t0];
    sy[1] = two ? rle[(size_t)c * rle_stride + t0 + 1u] : 0u;
#pragma unroll
    for (int h = 0; h < 2; h++) ee[h] = sym_class(sy[h]);
    // second wave: for each symbol its two history entries (entry 0 is 0 and entry 8 is 65536 by definition) and its mantissa word or ordinal
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int e = ee[h];
        const bool live = h == 0 || two;
        l0[h] = (e == 0 || !live) ? 0u : hrow[(size_t)(e - 1) * cs + h];
        h0[h] = (e == 7 || !live) ? 65536u : (uint32_t)hrow[(size_t)e * cs + h];
        aux[h] = !live ? 0u : (e < 2 ? mantad[o + h] : ord[o + h]);
    }
    // third wave: the QuasiModel table rows of the classes >= 2
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int e = ee[h];
        const uint32_t m = sy[h] - (uint32_t)class_base(e);
        if (e < 2) { l1[h] = aux[h] & 0xffffu; f1[h] = aux[h] >> 16; }
        else {
            const int q = qinterval(aux[h]);
            const uint32_t *cdf = qcdf + (((size_t)c * 6 + (e - 2)) * NQ + q) * QSTRIDE;
            l1[h] = cdf[m];
            f1[h] = cdf[m + 1] - l1[h];
        }
    }
    // lane-major: symbol 2g -> lanes 0, 1 and symbol 2g + 1 -> lanes 2, 3, all at index g
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (h == 1 && !two) break;
        rc[(size_t)(2 * h) * lane_stride + g] = rans_record(l0[h], h0[h] - l0[h]);
        rc[(size_t)(2 * h + 1) * lane_stride + g] = rans_record(l1[h], f1[h]);
        if (pairs_plain) {
            uint32_t *out = pairs_plain + (size_t)c * 2 * rle_stride + 2 * (size_t)(t0 + h);
            out[0] = l0[h] | ((h0[h] - l0[h]) << 16);
            out[1] = l1[h] | (f1[h] << 16);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// rANS (ans.cpp:189-208): four independent sequential chains per chunk (state lane = pair index & 3), last pair
// first.  Each step records the 0..2 renormalisation bytes it emits; their stream positions are a prefix sum.
// ---------------------------------------------------------------------------------------------------------------
// emitted bytes | count << 16 of the step that started from state x with threshold xmax
__device__ __forceinline__ uint32_t emit_word(uint32_t x, uint32_t xmax)
{
    const bool b1 = x >= xmax, b2 = (x >> 8) >= xmax;
    return b2 ? ((x & 0xffffu) | (2u << 16)) : (b1 ? ((x & 0xffu) | (1u << 16)) : 0u);
}

// One encoder step on every lane at once (see k_rans_lanes): the state comes from the lane on the left (DPP row
// rotate), keep = the state this lane had to start from once its turn came (captured when `turn` selects the lane).
// Cost on one wave (tools/issuetest.hip): a VALU instruction issues every ~4.4-5 cycles whatever it does, so the step is kept to
// twelve of them, written as one block (two steps per asm statement) because the order carries the wait states gfx940+ needs and the compiler
// cannot see into asm: two between a VALU write of an SGPR mask and the VALU reading it (cmp b2 .. select u,
// cmp b1 .. select xr) and two between the write of the new state and the next step's DPP read (capture + s_nop).
// After renormalisation xr < freq << 15, so q = xr / freq < 2^15 and 65536 - freq < 2^16: the second product fits the
// 24-bit multiply-add, which also ignores the shift count kept in the top byte of r.w.
// two consecutive steps (turns ta, tb) in one block: the compiler adds a wait state after every asm statement
#define JPK_RANS_STEP_ASM(XIN, XPREV, XOUT, TURN)                                                        \
        "v_mov_b32_dpp " XIN ", " XPREV " row_ror:1 row_mask:0xf bank_mask:0xf\n\t"                       \
        "v_lshrrev_b32 %[x8], 8, " XIN "\n\t"                                                             \
        "v_cmp_ge_u32_e64 %[b2], %[x8], %[xmax]\n\t"    /* b2 = (x >> 8) >= xmax: two bytes leave (implies b1) */ \
        "v_cmp_ge_u32_e64 %[b1], " XIN ", %[xmax]\n\t"  /* b1 = x >= xmax: one byte leaves */              \
        "v_lshrrev_b32 %[x16], 16, " XIN "\n\t"                                                           \
        "v_cndmask_b32_e64 %[u], %[x8], %[x16], %[b2]\n\t"     /* u = b2 ? x >> 16 : x >> 8 */            \
        "v_cndmask_b32_e64 %[xr], " XIN ", %[u], %[b1]\n\t"    /* xr = b1 ? u : x */                      \
        "v_mul_hi_u32 %[q], %[xr], %[rcp]\n\t"                                                            \
        "v_lshrrev_b32_sdwa %[q], %[w], %[q] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD\n\t" \
        "v_add_u32 %[t], %[xr], %[bias]\n\t"                                                              \
        "v_mad_u32_u24 " XOUT ", %[q], %[w], %[t]\n\t"  /* == ((xr / freq) << 16) + xr % freq + low */     \
        "v_cndmask_b32_e64 %[keep], %[keep], " XIN ", " TURN "\n\t"  /* my turn: remember the state I started from */ \
        "s_nop 0\n\t"
__device__ __forceinline__ uint32_t rans_step_turn2(uint32_t xprev, const uint4 r, uint32_t &keep, uint64_t ta, uint64_t tb)
{
    uint32_t xin, x8, x16, u, xr, q, t, xm, xn;
    uint64_t b1, b2;
    asm(JPK_RANS_STEP_ASM("%[xin]", "%[xprev]", "%[xm]", "%[ta]")
        JPK_RANS_STEP_ASM("%[xin]", "%[xm]", "%[xn]", "%[tb]")
        : [xin] "=&v"(xin), [x8] "=&v"(x8), [x16] "=&v"(x16), [u] "=&v"(u), [xr] "=&v"(xr), [q] "=&v"(q), [t] "=&v"(t), [xm] "=&v"(xm),
          [xn] "=&v"(xn), [b1] "=&s"(b1), [b2] "=&s"(b2), [keep] "+v"(keep)
        : [xprev] "v"(xprev), [xmax] "v"(r.x), [rcp] "v"(r.y), [bias] "v"(r.z), [w] "v"(r.w), [ta] "s"(ta), [tb] "s"(tb));
    return xn;
}

// One wave per chunk.  The four chains of a chunk (pair j -> chain j & 3, ans.cpp:189-208) own one row of
// 16 lanes each; lane s of a row holds the record of step K - s of the current batch of 16 steps.  The state travels: every step
// all lanes run the same twelve instructions on the state handed over by their left neighbour (DPP row rotate, no readlane), so
// after step t lane t holds the chain's true state and the others compute values nobody uses.  A lane keeps the state it was
// handed on its own turn; per batch the wave stores those 64 states (one coalesced 4-byte store) and nothing else: the emitted
// bytes and their stream positions are a pure function of (state before the step, record) and are computed afterwards by wide
// kernels (k_emit_count / k_emit_prefix / k_put_payload).  This wave is the serial floor of the whole stage -- 13 issue slots per
// step plus ~1 per step of batch overhead.  Steps past a chain's last pair use the identity records k_pairs has written.
//
// Record prefetch, correct by construction (round 4).  Sixteen batches of records are in flight (~6 us of steps: enough to cover a
// record load while suffix-sort kernels of another block saturate the memory system).  Rounds 2-3 kept them in sixteen register
// tuples loaded from inline asm, which the compiler believed to be valid from the asm statement on: a register copy it chose to
// insert (loop back-edge, spill) before the hand-counted s_waitcnt copied stale registers -- timing-dependent wrong bytes, guarded
// only by a regex over the assembly.  Now the records land in an LDS ring (global_load_lds_dwordx4: 1 KiB per wave-instruction,
// lane l -> ring[slot][l]) and NO register holds data in flight: a record becomes a register value through an ordinary ds_read
// that the compiler tracks itself (lgkmcnt), placed behind an asm s_waitcnt with a memory clobber that it cannot be moved across.
// What remains hand-counted is vmcnt, and the count is exact by program text: every vector-memory instruction of the loop (one
// LDS-DMA load and two stores per batch: the states' low halves and, round 6, the emit masks) is issued from asm volatile, loads and stores share vmcnt and retire in order, and
// anything the compiler might add (a spill) is YOUNGER than the load being waited for or older than all of them, which can only make
// the wait stricter.  tests/test_chain_codegen.py checks the generated loop for exactly that instruction census.
// One statement per batch for the four instructions that touch vector memory or M0: the LDS-DMA load takes its LDS address from
// M0 and needs one instruction between the SALU write of M0 and itself (the stores are), and M0 is
// compiler-reserved: the kernel uses it nowhere else (tests/test_chain_codegen.py checks), so it is not saved.  Addresses: a
// wave-uniform base in SGPRs + a 32-bit lane offset + an immediate -- inside the sixteen-fold unrolled loop body nothing is computed.
// (The LDS-DMA load carries no immediate: its instruction offset moves the LDS address as well as the global one -- measured the
// hard way -- so the lane offset of the records is stepped by one v_add per batch; the store's offset is an immediate.)
#define JPK_RING_STORE_LOAD(SLOT, SOFF, MOFF)                                                                          \
    asm volatile("s_mov_b32 m0, %[slot]\n\t"                                                                           \
                 "global_store_short %[xoff], %[keep], %[xbase] offset:" #SOFF "\n\t"                                  \
                 "global_store_dword %[moff], %[mw], %[mbase] offset:" #MOFF "\n\t"                                    \
                 "global_load_lds_dwordx4 %[roff], %[rbase]"                                                           \
                 : : [slot] "s"(ring0 + (uint32_t)((SLOT) & (RANS_RING - 1)) * 1024u), [xoff] "v"(xoff), [keep] "v"(keep), [xbase] "s"(xbase), [moff] "v"(moff), [mw] "v"(mw),   \
                     [mbase] "s"(mbase), [roff] "v"(roff), [rbase] "s"(rbase)                                          \
                 : "memory")
__global__ __launch_bounds__(64) void k_rans_lanes(const uint4 *__restrict__ recs, size_t rle_stride, EncDims d, const uint32_t *__restrict__ rlen,
                                                  uint16_t *__restrict__ x16, uint32_t *__restrict__ emask, uint32_t *__restrict__ fstate,
                                                  uint64_t *__restrict__ stamp)
{
    __shared__ uint4 ring[RANS_RING][64];
    const uint64_t t0c = __builtin_amdgcn_s_memtime(), t0r = __builtin_amdgcn_s_memrealtime();
    // this wave is a long dependent chain: let it win the issue arbitration against the wide kernels of other chunks /
    // blocks that share its SIMD (priority, then age)
    __builtin_amdgcn_s_setprio(3);
    const uint32_t c = chunk_of(d, blockIdx.x);
    const int t = threadIdx.x;
    const uint32_t np = 2 * rlen[c];
    if (np == 0) {
        if (t < 4) fstate[(size_t)c * 4 + t] = RANS_L;
        if (t == 0) { stamp[2 * (size_t)c] = 0; stamp[2 * (size_t)c + 1] = 0; }
        return;
    }
    const int chain = t >> 4, s = t & 15;
    const size_t lane_stride = lane_stride_of(d, c, rle_stride), lb = lane_base(d, c, rle_stride);
    // batches of sixteen steps, rounded up to whole rounds of the ring (round 6: the padding -- identity records, k_pairs -- is walked
    // first, from the start state, and costs at most fifteen batches per chunk; the exit test behind every batch of the unrolled loop,
    // three scalar instructions of 231, is gone)
    const int32_t nbatch = (((int32_t)((np - 1) / 4) / 16 + 1) + RANS_RING - 1) & ~(RANS_RING - 1);
    const int32_t K0 = 16 * nbatch - 1 - s;                        // this lane's step index in the first batch
    uint32_t x = RANS_L;                                           // lane 15 of a row hands the start state to lane 0
    const uint32_t ring0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)&ring[0][0];     // LDS byte address
    // wave-uniform bases (SGPR pairs) and 32-bit lane offsets in bytes.  The record base sits RANS_SLACK records in front of the
    // chunk's first record, so that the offset of a prefetch past the last batch (step index down to -256) stays non-negative: those
    // loads read the slack enc_layout leaves in front of the array (or the chains of the chunk before) and nobody uses them.
    const uint4 *rbase = recs + lb - RANS_SLACK;
    uint16_t *xbase = x16 + lb;
    uint32_t *mbase = emask + (lb >> 4);                           // (lane bases and strides are multiples of 128 records)
    uint32_t roff = (uint32_t)(((size_t)chain * lane_stride + (size_t)(K0 + RANS_SLACK)) * 16u);
    uint32_t xoff = (uint32_t)(((size_t)chain * lane_stride + (size_t)K0) * 2u);
    uint32_t moff = (uint32_t)((((size_t)chain * lane_stride) >> 4) + (size_t)(nbatch - 1)) * 4u;    // the row's mask word of the first batch
    const uint32_t rowsh = 16u * (uint32_t)chain;
    // prologue: the first sixteen batches' records, all landed before the loop starts -- one memory latency per chunk -- so that
    // from here on the steady-state count below holds for every wait
#define JPK_RING_PROLOGUE(SLOT)                                                                                         \
    asm volatile("s_mov_b32 m0, %[slot]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[roff], %[rbase]"                        \
                 : : [slot] "s"(ring0 + (uint32_t)(SLOT) * 1024u), [roff] "v"(roff), [rbase] "s"(rbase) : "memory");      \
    roff -= 256u;
    JPK_RING_PROLOGUE(0)  JPK_RING_PROLOGUE(1)  JPK_RING_PROLOGUE(2)  JPK_RING_PROLOGUE(3)
    JPK_RING_PROLOGUE(4)  JPK_RING_PROLOGUE(5)  JPK_RING_PROLOGUE(6)  JPK_RING_PROLOGUE(7)
    JPK_RING_PROLOGUE(8)  JPK_RING_PROLOGUE(9)  JPK_RING_PROLOGUE(10) JPK_RING_PROLOGUE(11)
    JPK_RING_PROLOGUE(12) JPK_RING_PROLOGUE(13) JPK_RING_PROLOGUE(14) JPK_RING_PROLOGUE(15)
#undef JPK_RING_PROLOGUE
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");            // (roff now points at the lane's record sixteen batches ahead)
    uint4 cur = ring[0][t];
    // One batch: the record of the NEXT batch (slot k + 1) was requested sixteen batches ago minus one; issued after it, in program
    // order: the two stores and the load of each of 14 batches -- vmcnt(42) -- (the first fifteen batches read slots the
    // prologue has drained).  It becomes a register value through an ordinary LDS read behind the wait, used one batch later.
    // Then 16 steps of every chain on `cur`, the store of the kept states, and the request for batch + 16 into the slot `cur` came from.
#define JPK_BATCH(KSLOT, SOFF, MOFF)                                                                                    \
    {                                                                                                                   \
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(3 * (RANS_RING - 2)) : "memory");                                    \
        const uint4 nxt = ring[((KSLOT) + 1) & (RANS_RING - 1)][t];                                                     \
        _Pragma("unroll") for (int st = 0; st < 16; st += 2)                                                            \
            x = rans_step_turn2(x, cur, keep, 0x0001000100010001ull << st, 0x0001000100010001ull << (st + 1));          \
        /* what the step of every lane emitted (round 6): one byte when its start state reached xmax, two when state >> 8 did -- as a     \
           bit per lane, the sixteen lanes of a row = the sixteen steps of the row's chain in this batch (bit s <-> step K - s) */       \
        const uint64_t e1 = __ballot(keep >= cur.x), e2 = __ballot((keep >> 8) >= cur.x);                               \
        const uint32_t mw = ((uint32_t)(e1 >> rowsh) & 0xffffu) | ((uint32_t)(e2 >> rowsh) << 16);                      \
        JPK_RING_STORE_LOAD(KSLOT, SOFF, MOFF);                                                                         \
        roff -= 256u;                                                                                                   \
        cur = nxt;                                                                                                      \
    }
    uint32_t keep = 0;                                             // (every lane's turn comes once per batch and overwrites it)
    for (int32_t left = nbatch; left > 0; left -= RANS_RING) {    // whole rounds: no exit inside
        JPK_BATCH(0, 0, 0)
        JPK_BATCH(1, -32, -4)
        JPK_BATCH(2, -64, -8)
        JPK_BATCH(3, -96, -12)
        JPK_BATCH(4, -128, -16)
        JPK_BATCH(5, -160, -20)
        JPK_BATCH(6, -192, -24)
        JPK_BATCH(7, -224, -28)
        JPK_BATCH(8, -256, -32)
        JPK_BATCH(9, -288, -36)
        JPK_BATCH(10, -320, -40)
        JPK_BATCH(11, -352, -44)
        JPK_BATCH(12, -384, -48)
        JPK_BATCH(13, -416, -52)
        JPK_BATCH(14, -448, -56)
        JPK_BATCH(15, -480, -60)
        xoff -= 16u * 32u;
        moff -= 16u * 4u;
    }
#undef JPK_BATCH
#undef JPK_RING_STORE_LOAD
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");            // the prefetches of batches that do not exist must land before the LDS is released
    if (s == 15) fstate[(size_t)c * 4 + chain] = x;               // the last batch ends at step 0: lane 15 holds each chain's final state
    if (t == 0) {
        // diagnostics: shader cycles and 100 MHz ticks this chunk's chains took (jpk_stats.enc_chain_*)
        stamp[2 * (size_t)c] = __builtin_amdgcn_s_memtime() - t0c;
        stamp[2 * (size_t)c + 1] = __builtin_amdgcn_s_memrealtime() - t0r;
    }
}

// ---- emitted bytes and their positions, in parallel over all pairs ---------------------------------------------------------
// Pair j of a chunk (chain j & 3, step j >> 2) emitted 0..2 bytes; the encoder walks the pairs last to first and the stream grows
// downwards, so the bytes of pair j start  sum_{j' >= j} count(j')  bytes before the end of the chunk's payload.
// Round 6: what the emit kernels read is what the chain left behind for them -- per step the low 16 bits of the state it started
// from (the only bits a step can emit) and, per chain and batch of sixteen steps, one word of emit masks (low half: "one byte at
// least", high half: "two"; bit s <-> step 16 m + 15 - s of the chain: lane s of the chain's row, k_rans_lanes) -- 2.25 bytes per
// pair.  Rounds 2-5 kept the whole 32-bit state and a 2-byte frequency sidecar written by k_pairs and recomputed the comparison
// against x_max twice: 12 bytes read per pair to place 0.17 (profiles/r05_pmc_traffic.json: k_put_payload fetched 418 MB per launch).
// mask words of one chain that are written: one per batch of the chunk
__device__ __forceinline__ uint32_t rans_batches(uint32_t np) { return np ? ((np - 1u) >> 2) / 16u + 1u : 0u; }

__global__ __launch_bounds__(TB) void k_emit_count(const uint32_t *__restrict__ emask, size_t rle_stride, EncDims d,
                                                  const uint32_t *__restrict__ rlen, uint32_t *__restrict__ tsum, uint32_t etpc)
{
    const uint32_t c = chunk_of(d, blockIdx.y), tile = blockIdx.x;
    const uint32_t np = 2 * rlen[c];
    if (tile * ETILE >= np) return;
    const size_t lane_stride = lane_stride_of(d, c, rle_stride), cb = lane_base(d, c, rle_stride);
    // the tile's pairs are the steps [1024 tile, 1024 tile + 1024) of the four chains: 64 mask words each, one per thread
    const uint32_t chain = threadIdx.x >> 6, w = tile * (ETILE / 64) + (threadIdx.x & 63u);
    const uint32_t n = w < rans_batches(np) ? (uint32_t)__popc(emask[((cb + (size_t)chain * lane_stride) >> 4) + w]) : 0u;   // (padding steps carry identity records: no bits)
    __shared__ uint32_t sm[TB / 64 + 1];
    uint32_t tot;
    block_incl_scan<OpSum>(n, sm, &tot);
    if (threadIdx.x == 0) tsum[(size_t)c * etpc + tile] = tot;
}

// one wave per chunk: tsum -> bytes emitted by all LATER tiles (exclusive suffix sum), csize = 16 state bytes + total
__global__ __launch_bounds__(64) void k_emit_prefix(EncDims d, const uint32_t *__restrict__ rlen, uint32_t *__restrict__ tsum, uint32_t etpc,
                                                   uint32_t *__restrict__ csize)
{
    const uint32_t c = chunk_of(d, blockIdx.x);
    const uint32_t np = 2 * rlen[c];
    const int nt = (int)((np + ETILE - 1) / ETILE), l = lane_id();
    uint32_t *ts = tsum + (size_t)c * etpc;
    uint32_t carry = 0;
    for (int hi = nt; hi > 0; hi -= 64) {                 // windows of 64 tiles, last window first
        const int tIdx = hi - 1 - l;                      // lane 0 = the last tile of the window
        const uint32_t v = (tIdx >= 0) ? ts[tIdx] : 0u;
        const uint32_t inc = wave_incl_sum(v);
        if (tIdx >= 0) ts[tIdx] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (l == 0) csize[c] = 16u + carry;
}

// header bytes of one chunk per workgroup (ans.cpp:272-285): thread s encodes Freq[s], the three length fields follow
__global__ __launch_bounds__(256) void k_headers(EncDims d, const int32_t *__restrict__ freq, const uint32_t *__restrict__ csize,
                                                const uint32_t *__restrict__ rlen, uint8_t *__restrict__ hdr, uint32_t *__restrict__ hsize)
{
    __shared__ uint32_t sm[256 / 64 + 1];
    const uint32_t c = blockIdx.x;
    uint8_t *h = hdr + (size_t)c * HDR_MAX;
    uint8_t tmp[5];
    const uint32_t n = pre::leb_write((uint32_t)freq[(size_t)c * 256 + threadIdx.x], tmp);
    uint32_t tot;
    const uint32_t inc = block_incl_scan<OpSum>(n, sm, &tot);
    uint8_t *o = h + (inc - n);
    for (uint32_t k = 0; k < n; k++) o[k] = tmp[k];
    if (threadIdx.x == 0) {
        int p = (int)tot;
        p += pre::leb_write(chunk_len(d, c), h + p);
        p += pre::leb_write(csize[c], h + p);
        p += pre::leb_write(rlen[c], h + p);
        hsize[c] = (uint32_t)p;
    }
}

// output offset of every chunk, totals and the chain diagnostics -> mailbox
__global__ __launch_bounds__(64) void k_out_offsets(EncDims d, const uint32_t *__restrict__ csize, const uint32_t *__restrict__ rlen,
                                                   const uint32_t *__restrict__ hsize, uint64_t *__restrict__ outoff, uint32_t *__restrict__ mail,
                                                   const uint64_t *__restrict__ stamp)
{
    if (threadIdx.x != 0) return;
    uint64_t o = 0, rs = 0;
    uint32_t worst = 0;                      // the chunk whose chains ran longest
    for (uint32_t c = 0; c < d.nch; c++) {
        if (d.cblk && c && d.cblk[c] != d.cblk[c - 1]) o = 0;      // group encode: every block's stream starts at 0 of its own buffer
        outoff[c] = o;
        o += (uint64_t)hsize[c] + csize[c];
        rs += rlen[c];
        if (stamp[2 * (size_t)c] > stamp[2 * (size_t)worst]) worst = c;
    }
    outoff[d.nch] = o;
    mail[MAIL_TOTAL] = (uint32_t)o;
    mail[MAIL_TOTAL + 1] = (uint32_t)(o >> 32);
    mail[MAIL_RLE_SYMBOLS] = (uint32_t)rs;
    mail[MAIL_RLE_SYMBOLS + 1] = (uint32_t)(rs >> 32);
    mail[MAIL_CHAIN_CYCLES] = (uint32_t)stamp[2 * (size_t)worst]; mail[MAIL_CHAIN_CYCLES + 1] = (uint32_t)(stamp[2 * (size_t)worst] >> 32);
    mail[MAIL_CHAIN_TICKS] = (uint32_t)stamp[2 * (size_t)worst + 1]; mail[MAIL_CHAIN_TICKS + 1] = (uint32_t)(stamp[2 * (size_t)worst + 1] >> 32);
    mail[MAIL_CHAIN_RLEN] = rlen[worst];
}

__global__ __launch_bounds__(TB) void k_put_headers(EncDims d, const uint8_t *__restrict__ hdr, const uint32_t *__restrict__ hsize,
                                                   const uint64_t *__restrict__ outoff, const uint32_t *__restrict__ fstate, uint8_t *__restrict__ out)
{
    const uint32_t c = blockIdx.x;
    uint8_t *const ob = d.cblk ? d.bout[d.cblk[c]] : out;
    if (!ob) return;                        // group encode: the chunk's block does not fit its buffer (reported JPK_E_CAPACITY): nothing of it is written
    uint8_t *o = ob + outoff[c];
    const uint32_t hs = hsize[c];
    for (uint32_t i = threadIdx.x; i < hs; i += TB) o[i] = hdr[(size_t)c * HDR_MAX + i];
    if (threadIdx.x < 16) {
        // flush order R[3],R[2],R[1],R[0] downwards => forward stream R0 R1 R2 R3, little endian (ans.cpp:203-206)
        uint32_t st = fstate[(size_t)c * 4 + (threadIdx.x >> 2)];
        o[hs + threadIdx.x] = (uint8_t)(st >> (8 * (threadIdx.x & 3)));
    }
}

// payload bytes: every pair places its 0..2 bytes (offset = bytes of all later pairs, from the end of the chunk's payload)
__global__ __launch_bounds__(TB) void k_put_payload(const uint16_t *__restrict__ x16, const uint32_t *__restrict__ emask, size_t rle_stride, EncDims d,
                                                   const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ tsuf, uint32_t etpc,
                                                   const uint32_t *__restrict__ csize, const uint32_t *__restrict__ hsize, const uint64_t *__restrict__ outoff,
                                                   uint8_t *__restrict__ out)
{
    const uint32_t c = blockIdx.y, tile = blockIdx.x;
    const uint32_t np = 2 * rlen[c];
    if (tile * ETILE >= np) return;
    uint8_t *const ob = d.cblk ? d.bout[d.cblk[c]] : out;
    if (!ob) return;                        // (uniform over the workgroup; see k_put_headers)
    const size_t lane_stride = lane_stride_of(d, c, rle_stride), cb = lane_base(d, c, rle_stride);
    // thread t owns the 16 consecutive pairs [j0, j0 + 16) of the tile = the four steps [s0, s0 + 4) of the four chains (pair j: chain
    // j & 3, step j >> 2): per chain one mask word (the four steps share it) and one 8-byte load of their four 16-bit states
    const uint32_t s0 = tile * (ETILE / 4) + threadIdx.x * 4u;
    const bool live = (s0 >> 4) < rans_batches(np);
    uint32_t mw[4];
    uint2 xv[4];
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {        // loads first (a live thread's four steps lie inside the chain's batches: 16 | 4)
        const size_t o = cb + (size_t)ch * lane_stride + (live ? s0 : 0u);
        mw[ch] = live ? emask[o >> 4] : 0u;
        xv[ch] = *reinterpret_cast<const uint2 *>(x16 + o);
    }
    uint32_t e[16];
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int ch = k & 3, q = k >> 2;                           // pair j0 + k
        const uint32_t bit = 15u - ((s0 + (uint32_t)q) & 15u);
        const uint32_t cnt = ((mw[ch] >> bit) & 1u) + ((mw[ch] >> (16u + bit)) & 1u);
        const uint32_t xw = q < 2 ? xv[ch].x : xv[ch].y;
        e[k] = ((q & 1) ? xw >> 16 : xw & 0xffffu) | (cnt << 16);
        n += cnt;
    }
    // bytes emitted by the threads after me = block total - inclusive prefix
    __shared__ uint32_t sm[TB / 64 + 1];
    uint32_t tot;
    const uint32_t inc = block_incl_scan<OpSum>(n, sm, &tot);
    uint32_t after = tsuf[(size_t)c * etpc + tile] + (tot - inc);       // bytes of all pairs after my 16
    uint8_t *end = ob + outoff[c] + hsize[c] + csize[c];
#pragma unroll
    for (int k = 15; k >= 0; k--) {
        const uint32_t cnt = e[k] >> 16;
        after += cnt;
        if (cnt == 1) end[-(int64_t)after] = (uint8_t)e[k];
        else if (cnt == 2) { uint8_t *p = end - after; p[0] = (uint8_t)(e[k] >> 8); p[1] = (uint8_t)e[k]; }   // the later (lower-address) byte of a step comes first
    }
}

}  // namespace

namespace jpk_enc {

// step records of every pair, lane-major, padded with identity steps (and the plain pairs for the stand-alone probe when b.pairs is set)
int run_pairs(jpk_ctx *ctx, const uint16_t *d_rle, const uint32_t *d_rlen, const EncDims &d, EncBufs &b)
{
    const size_t stride = d.chunk;
    JPK_LAUNCH(ctx, PROF_ENC_PAIRS, 0, k_pairs, dim3(jpk_grid(stride, 2 * TB) + 3, d.ncl), dim3(TB), d_rle, stride, d, d_rlen, b.exph, b.mantad, b.ord,
                       b.qcdf, b.recs, b.pairs);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

// the chains: one wave per chunk of the launch group
int run_chain(jpk_ctx *ctx, const EncDims &d, EncBufs &b)
{
    const size_t stride = d.chunk;
    JPK_LAUNCH(ctx, PROF_ENC_RANS, 0, k_rans_lanes, dim3(d.ncl), dim3(64), b.recs, stride, d, b.rlen, b.x16, b.emask, b.fstate, b.stamp);
    return JPK_OK;
}

// bytes emitted per tile of pairs -> bytes of all later tiles, and the chunk's payload size
int run_emit_counts(jpk_ctx *ctx, const EncDims &d, EncBufs &b)
{
    const size_t stride = d.chunk;
    const uint32_t etpc = emit_tiles_per_chunk(stride);
    JPK_LAUNCH(ctx, PROF_ENC_EMIT, 0, k_emit_count, dim3(etpc, d.ncl), dim3(TB), b.emask, stride, d, b.rlen, b.etsum, etpc);
    JPK_LAUNCH(ctx, PROF_ENC_EMIT, 0, k_emit_prefix, dim3(d.ncl), dim3(64), d, b.rlen, b.etsum, etpc, b.csize);
    return JPK_OK;
}

// the tail of encode_core: every chunk's header, then the output offsets; the totals and the worst chain's stamps go to the mailbox
int run_offsets(jpk_ctx *ctx, const EncDims &d, EncBufs &b)
{
    JPK_LAUNCH(ctx, PROF_ENC_EMIT, 0, k_headers, dim3(d.nch), dim3(256), d, b.freq, b.csize, b.rlen, b.hdr, b.hsize);
    JPK_LAUNCH(ctx, PROF_ENC_EMIT, 0, k_out_offsets, dim3(1), dim3(64), d, b.csize, b.rlen, b.hsize, b.outoff, ctx->d_mail->read, b.stamp);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

// headers, final states and payload bytes of every chunk at their offsets of `d_out` (a group of blocks: of EncDims::bout, d_out null)
int run_put(jpk_ctx *ctx, const EncDims &d, EncBufs &b, uint8_t *d_out)
{
    const size_t stride = d.chunk;
    JPK_LAUNCH(ctx, PROF_ENC_EMIT, 0, k_put_headers, dim3(d.nch), dim3(TB), d, b.hdr, b.hsize, b.outoff, b.fstate, d_out);
    JPK_LAUNCH(ctx, PROF_ENC_EMIT, 0, k_put_payload, dim3(emit_tiles_per_chunk(stride), d.nch), dim3(TB), b.x16, b.emask, stride, d, b.rlen, b.etsum,
               emit_tiles_per_chunk(stride), b.csize, b.hsize, b.outoff, d_out);
    JPK_HIP(hipGetLastError());
    return JPK_OK;
}

}  // namespace jpk_enc
