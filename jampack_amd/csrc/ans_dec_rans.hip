// ans_dec_rans.hip -- the rANS + model chains of the decoder: k_dec_rans, one wave per chunk (run_rans).  ans_dec.hpp is what the decoder's
// units share; the overview and the map of the units are at the top of ans_dec.hip.
#include "ans_dec.hpp"

using namespace jpk;
using namespace jpk_dec;

namespace {

// ---------------------------------------------------------------------------------------------------------------
// rANS + model decode: one wave per chunk (ans.cpp:30-92).
//
// The loop is one long dependent chain, so it is written for the issue costs of a single gfx950 wave (measured with
// tools/issuetest.hip): a VALU or SALU instruction issues every ~5 cycles (4.4 ns-ticks at 2.4 GHz: 5.1 independent, 5-6
// in a dependent chain), a SALU instruction that reads an SGPR a VALU instruction has just written stalls ~17 cycles
// more, an LDS round trip is 52-68 cycles, a branch ~14 (not taken) to ~24 (taken) cycles, and every value that is live
// across diverging arms costs a copy at the join.  Hence:
//   * the four rANS states, the byte queue and the two alphabet-2 models are wave-uniform and live in SGPRs;
//   * the 8-symbol exponent model and the mantissa models of classes 2..5 are register resident with "lane = symbol":
//     lane j holds LO_j = cdf[j], HI_j = cdf[j+1], FR_j = HI_j - LO_j of its symbol (class e owns lanes
//     [2^e, 2^(e+1)), which is exactly the RLE0 symbol numbering, tables.hpp:10).  All lanes form their candidate
//     next state FR_j * (x >> 16) + (x & 0xffff) - LO_j at once; one v_cmp (HI_j > x & 0xffff), one s_ff1 and one
//     v_readlane pick the coded symbol and its next state: no LDS, no search loop;
//   * the rebuild countdowns of classes 2..5 live in lanes 0..3 of one VGPR (lanes 4, 5 hold a permanent 1 for classes 6
//     and 7), the output tile is collected with v_writelane and stored every 64 symbols, and ONE scalar test per symbol
//     covers "an event is due" and "a state needs bytes";
//   * payload bytes come from a 64-bit SGPR queue refilled one dword at a time from a 256-byte window held across
//     the wave (lane l = dword l, next window prefetched).
// Classes 6 and 7 (64 and 129 symbols, rare outside incompressible data) keep their CDFs in one / three more registers.
// ---------------------------------------------------------------------------------------------------------------
// QuasiModel rebuild (model.cpp:160-204) of a register-resident model of A <= 64 * NR symbols: symbol i = lane l of
// register j (i = l + 64 j).  hi/lo/fr become the bounds and width of every symbol, the counts are cleared.
template <int NR>
__device__ __forceinline__ void quasi_rebuild_regs(int A, int l, uint32_t (&hi)[NR], uint32_t (&lo)[NR], uint32_t (&fr)[NR], uint32_t (&f)[NR],
                                                   uint32_t &expn)
{
    uint32_t F[NR];
    uint32_t tot = 0;
#pragma unroll
    for (int j = 0; j < NR; j++) { F[j] = (l + 64 * j < A) ? f[j] : 0u; tot += F[j]; }
    tot = wave_sum(tot);
    int lg = 0;
    while ((tot >> lg) + (uint32_t)A > 65536u) lg++;
    uint32_t t2 = 0;
#pragma unroll
    for (int j = 0; j < NR; j++) { F[j] = (l + 64 * j < A) ? (F[j] >> lg) + 1u : 0u; t2 += F[j]; }
    t2 = wave_sum(t2);
    uint32_t t3 = 0;
#pragma unroll
    for (int j = 0; j < NR; j++) { F[j] = (65536u * F[j]) / t2; t3 += F[j]; }
    t3 = wave_sum(t3);
    if (l == 0) F[0] += 65536u - t3;
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < NR; j++) {
        const uint32_t inc = wave_incl_sum(F[j]);
        hi[j] = carry + inc;                         // symbols past the alphabet end at 65536 with width 0
        lo[j] = carry + inc - F[j];
        fr[j] = F[j];
        f[j] = 0;
        carry += __shfl(inc, 63, 64);
    }
    expn = (expn < 65536u) ? expn << 1 : 65536u;
}

// 256-byte input window held across the wave (lane l = dword l), next window prefetched, drained through a 64-bit
// scalar queue: a renormalisation byte is two scalar instructions away.
struct ByteQueue {
    const uint32_t *pw;       // dword-aligned base (payload start rounded down)
    int64_t gbase;            // byte offset of pw inside the whole input buffer
    int64_t in_len;
    const uint8_t *in;
    uint32_t cur, nxt;        // my dword of the current / next window
    uint32_t di;              // next dword of the stream to enter the queue
    uint64_t buf;             // queued bytes, next one in bits 7:0
    uint32_t nb;              // bytes in the queue
    uint32_t skip;            // bytes in front of the payload in the first dword (alignment)
    int l;
    __device__ __forceinline__ uint32_t load(uint32_t w) const
    {
        const int64_t g = gbase + ((int64_t)w * 64 + l) * 4;     // byte offset in the input buffer
        if (g >= 0 && g + 4 <= in_len) return pw[(size_t)w * 64 + l];
        uint32_t v = 0;
        for (int k = 0; k < 4; k++)
            if (g + k >= 0 && g + k < in_len) v |= (uint32_t)in[g + k] << (8 * k);
        return v;
    }
    __device__ __forceinline__ void refill()
    {
        if ((di & 63u) == 0u && di != 0u) { cur = nxt; nxt = load((di >> 6) + 1u); }      // uniform
        const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(di & 63u));
        buf |= (uint64_t)d << (8u * nb);
        nb += 4u;
        di++;
    }
    __device__ __forceinline__ void init(const uint8_t *input, int64_t input_len, const uint8_t *p, int lane)
    {
        in = input; in_len = input_len; l = lane;
        const uint32_t a = (uint32_t)((uintptr_t)p & 3u);
        pw = reinterpret_cast<const uint32_t *>(p - a);
        gbase = (p - a) - input;
        cur = load(0);
        nxt = load(1);
        di = 0; buf = 0; nb = 0; skip = a;
        refill();
        buf >>= 8u * a;
        nb -= a;
        refill();
    }
    __device__ __forceinline__ void top_up() { if (__builtin_expect(nb < 4u, 0)) refill(); }      // leaves nb >= 4
    // payload bytes consumed so far: what entered the queue minus what is still queued (not counted per byte)
    __device__ __forceinline__ uint32_t taken() const { return 4u * di - skip - nb; }
    __device__ __forceinline__ uint32_t take()
    {
        const uint32_t b = (uint32_t)buf & 0xffu;
        buf >>= 8;
        nb--;
        return b;
    }
};

__device__ __forceinline__ uint32_t dpp_row_shr1_zero(uint32_t v)     // lane j <- lane j-1 inside a row of 16, lane 0 of a row <- 0
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, true);
}

#define JPK_ICMP_EQ 32      // llvm::CmpInst::ICMP_EQ
#define JPK_ICMP_ULT 36     // llvm::CmpInst::ICMP_ULT

// Both states of a symbol are renormalised in the slow block: up to four bytes leave the queue, in stream order (exponent
// state first, ans.cpp:50-86), and one refill restores the >= 4 queued bytes the next symbol relies on.
#define JPK_RENORM2(X, X2)                                        \
    {                                                             \
        if ((X) < RANS_L) {                                       \
            (X) = ((X) << 8) | bq.take();                         \
            if (__builtin_expect((X) < RANS_L, 0)) (X) = ((X) << 8) | bq.take();       \
        }                                                         \
        if ((X2) < RANS_L) {                                      \
            (X2) = ((X2) << 8) | bq.take();                       \
            if (__builtin_expect((X2) < RANS_L, 0)) (X2) = ((X2) << 8) | bq.take();    \
        }                                                         \
        bq.top_up();                                              \
    }

// one RLE0 symbol: exponent from state RA, mantissa from state RB (the states rotate, ans.cpp:50-86); LANEI = its lane in
// the 64-symbol output tile.
// Instruction order matters on a single wave: the exponent compare goes first so that the vector work that does not need
// the exponent (candidates, mantissa compare) covers the wait of the scalar unit for its mask; the model updates sit where
// the scalar unit would otherwise wait for a v_readlane result; sched_barrier keeps the compiler from undoing that.
// A symbol pays one branch plus a quarter of the loop's: the slow block is entered when a model rebuild is due, when the
// class is 6/7 (their lanes of `rem` hold 1 permanently) or when min(x, x2) says that a state needs bytes.
#define JPK_DEC_SYMBOL(RA, RB, LANEI)                                                                     \
    {                                                                                                     \
        /* range = state & 0xffff and state >> 16 are taken straight from the scalar state by SDWA / op_sel operands:  \
           v_cmp(range < HI), range - LO, FR * (state >> 16) + (range - LO) for the exponent and the mantissa model.   \
           One block fixes the order (the SDWA results are consumed two instructions later; FR < 65536 fits u16) */  \
        uint64_t eabove, qabove;                                                                          \
        uint32_t et_, qt_, ecand, qcand;                                                                  \
        asm("v_cmp_lt_u32_sdwa %0, %6, %7 src0_sel:WORD_0 src1_sel:DWORD\n\t"                            \
            "v_sub_u32_sdwa %2, %6, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t" \
            "v_cmp_lt_u32_sdwa %1, %9, %10 src0_sel:WORD_0 src1_sel:DWORD\n\t"                           \
            "v_sub_u32_sdwa %3, %9, %11 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t" \
            "v_mad_u32_u16 %4, %12, %6, %2 op_sel:[0,1,0,0]\n\t"                                          \
            "v_mad_u32_u16 %5, %13, %9, %3 op_sel:[0,1,0,0]"                                              \
            : "=&s"(eabove), "=&s"(qabove), "=&v"(et_), "=&v"(qt_), "=&v"(ecand), "=&v"(qcand)            \
            : "s"(RA), "v"(ehi), "v"(elo), "s"(RB), "v"(qhi), "v"(qlo), "v"(efr), "v"(qfr));              \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        const uint32_t e = (uint32_t)__builtin_ctz((uint32_t)eabove);                                     \
        /* symbol s = lane s; class e owns the lanes whose class is e (none for e >= 6: the event block takes over).           \
           The three lane masks that depend on e are formed first: their users below then sit far enough behind them that no  \
           wait state is needed between a vector compare and the vector instruction that takes its mask */            \
        const bool below = (uint32_t)l < e;                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)ecand, (int)e);                             \
        const bool counts = cls_of_lane == e;                                                             \
        const bool mine = lane_cls == e;                                                                  \
        const uint64_t minemask = __ballot(mine);                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        /* AdaptiveModel update (model.cpp:60-77): entry i = j + 1 lives in lane j */                     \
        const int32_t mix = below ? emix_lo : emix_hi;                                                    \
        ehi = (uint32_t)((int32_t)ehi + ((mix - (int32_t)ehi) >> 5));                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        /* countdowns: lane e - 2 counts the symbols of class e until its rebuild (classes 6, 7: always due) */ \
        rem -= counts ? 1u : 0u;                                                                          \
        const uint64_t due = __builtin_amdgcn_uicmp(rem, 0u, JPK_ICMP_EQ);                                \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        elo = dpp_row_shr1_zero(ehi);                                                                     \
        efr = ehi - elo;                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        /* for e >= 6 the mask is empty: s_ff1 returns -1, v_readlane takes lane 63 and no lane counts; the event block redoes both */ \
        uint32_t sym;                                                                                     \
        asm("s_ff1_i32_b64 %0, %1" : "=s"(sym) : "s"(qabove & minemask));                                 \
        const bool hit = (uint32_t)l == sym;                                                              \
        uint32_t x2 = (uint32_t)__builtin_amdgcn_readlane((int)qcand, (int)sym);                          \
        const int32_t tgt = (sym & 1u) ? 1 : 65535;                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        {                                                                                                 \
            qf += hit ? 1u : 0u;                                                 /* QuasiModel count, in units of 16 */ \
            /* AdaptiveModel update of the alphabet-2 pair (lanes 2e, 2e+1) when e < 2: both lanes carry a = cdf[1] */ \
            const int32_t d = mine ? (tgt - (int32_t)qa) >> 5 : 0;                                        \
            qa += (uint32_t)d;                                                                            \
            qhi = (uint32_t)(__mul24(d, even_lane) + (int32_t)qhi);                                       \
            qlo = (uint32_t)(__mul24(d, odd_lane) + (int32_t)qlo);                                        \
            qfr = (uint32_t)(__mul24(d, sign_lane) + (int32_t)qfr);                                       \
        }                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        /* ONE test sends a symbol to the slow block: an event is due, or one of the two states needs bytes */ \
        uint32_t gate;                                       /* 0 when an event is due, else min(x, x2) */ \
        asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, 0, %2" : "=s"(gate) : "s"(due), "s"(x < x2 ? x : x2) : "scc"); \
        if (__builtin_expect(gate < RANS_L, 0)) {                                                         \
          if (__builtin_expect(due != 0ull, 0)) {        /* most visits are renormalisations */           \
            const uint32_t range_m = (RB) & 0xffffu, xs_m = (RB) >> 16;                                   \
            if (e == 6u) {                                                                                \
                /* classes 6 (64 symbols) and 7 (129): same lane-per-symbol search over one / three registers */ \
                const uint32_t cand = __umul24(fr6[0], xs_m) + (range_m - lo6[0]);                        \
                const uint32_t m = (uint32_t)__builtin_ctzll(__builtin_amdgcn_uicmp(range_m, hi6[0], JPK_ICMP_ULT)); \
                x2 = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)m);                              \
                f6[0] += ((uint32_t)l == m) ? 16u : 0u;                                                   \
                sym = 64u + m;                                                                            \
                if (++seen6 > expn6) { quasi_rebuild_regs<1>(64, l, hi6, lo6, fr6, f6, expn6); seen6 = 0; } \
                rem = (l == 4) ? 1u : rem;                                                                \
            } else if (e == 7u) {                                                                         \
                const uint64_t a0 = __builtin_amdgcn_uicmp(range_m, hi7[0], JPK_ICMP_ULT);                \
                const uint64_t a1 = __builtin_amdgcn_uicmp(range_m, hi7[1], JPK_ICMP_ULT);                \
                uint32_t m;                                                                               \
                if (a0) {                                                                                 \
                    m = (uint32_t)__builtin_ctzll(a0);                                                    \
                    x2 = (uint32_t)__builtin_amdgcn_readlane((int)(__umul24(fr7[0], xs_m) + (range_m - lo7[0])), (int)m); \
                    f7[0] += ((uint32_t)l == m) ? 16u : 0u;                                               \
                } else if (a1) {                                                                          \
                    m = (uint32_t)__builtin_ctzll(a1);                                                    \
                    x2 = (uint32_t)__builtin_amdgcn_readlane((int)(__umul24(fr7[1], xs_m) + (range_m - lo7[1])), (int)m); \
                    f7[1] += ((uint32_t)l == m) ? 16u : 0u;                                               \
                    m += 64u;                                                                             \
                } else {                                             /* the 129th symbol: lane 0 of the third register */ \
                    m = 128u;                                                                             \
                    x2 = (uint32_t)__builtin_amdgcn_readlane((int)(__umul24(fr7[2], xs_m) + (range_m - lo7[2])), 0); \
                    f7[2] += (l == 0) ? 16u : 0u;                                                         \
                }                                                                                         \
                sym = 128u + m;                                                                           \
                if (++seen7 > expn7) { quasi_rebuild_regs<3>(129, l, hi7, lo7, fr7, f7, expn7); seen7 = 0; } \
                rem = (l == 5) ? 1u : rem;                                                                \
            } else {                                                                                      \
                /* QuasiModel rebuild (model.cpp:160-204) of class e (2..5) in its lanes [2^e, 2^(e+1)): the same rule as      \
                   quasi_rebuild_regs, on the layout in which four models share qhi / qlo / qfr / qf, each in its own lanes */ \
                const uint32_t kl = e - 2u;                                                               \
                const uint32_t A = 1u << e;                                                               \
                const bool mine = ((uint32_t)l >> e) == 1u;      /* shadows the symbol's flag: same lanes */ \
                uint32_t F = mine ? qf << 4 : 0u;                                                         \
                const uint32_t tot = wave_sum(F);                                                         \
                int lg = 0;                                                                               \
                while ((tot >> lg) + A > 65536u) lg++;                                                    \
                F = mine ? (F >> lg) + 1u : 0u;                                                           \
                const uint32_t t2 = wave_sum(F);                                                          \
                F = (65536u * F) / t2;                                                                    \
                const uint32_t t3 = wave_sum(F);                                                          \
                if ((uint32_t)l == A) F += 65536u - t3;                 /* first symbol of the class */   \
                const uint32_t inc = wave_incl_sum(F);                                                    \
                qhi = mine ? inc : qhi; qlo = mine ? inc - F : qlo; qfr = mine ? F : qfr; qf = mine ? 0u : qf; \
                const uint32_t ex0 = (uint32_t)__builtin_amdgcn_readlane((int)qexpn, (int)(kl & 3u));     \
                const uint32_t ex1 = (ex0 < 65536u) ? ex0 << 1 : 65536u;                                  \
                qexpn = ((uint32_t)l == kl) ? ex1 : qexpn;                                                \
                rem = ((uint32_t)l == kl) ? ex1 + 1u : rem;                                               \
            }                                                                                             \
          }                                                                                               \
          JPK_RENORM2(x, x2)                                                                              \
        }                                                                                                 \
        (RA) = x;                                                                                         \
        (RB) = x2;                                                                                        \
        mysym = lane_write(mysym, sym, (uint32_t)(LANEI));                                                \
    }

__global__ __launch_bounds__(64) void k_dec_rans(const DecBlock *__restrict__ blocks, const ChunkInfo *__restrict__ info, const uint32_t *__restrict__ order,
                                                uint32_t *__restrict__ status_all)
{
    __builtin_amdgcn_s_setprio(3);         // serial chain: win the issue arbitration on a shared SIMD
    const uint32_t c = order ? order[blockIdx.x] : blockIdx.x;
    const int l = lane_id();
    const ChunkInfo ci = info[c];
    const DecBlock B = blocks[ci.blk];
    const uint8_t *__restrict__ in = B.in;
    const int64_t in_len = B.in_len;
    uint16_t *__restrict__ rle = B.rle;
    uint32_t *status = status_all + ci.blk;
    const uint8_t *p = in + ci.in_off;
    const uint32_t clen = ci.clen, rlen = ci.rlen;
    uint16_t *out = rle + ci.rle_off;

    ByteQueue bq;
    bq.init(in, in_len, p, l);
    // exponent model (alphabet 8): lane j holds LO = cdf[j], HI = cdf[j+1]; lanes >= 7 keep HI = 65536
    uint32_t elo = (l < 8) ? uniform_cdf(8, l) : 65536u;
    uint32_t ehi = (l < 8) ? uniform_cdf(8, l + 1) : 65536u;
    uint32_t efr = ehi - elo;
    // mix targets of entry i = l + 1 (model.cpp:60-77): i when i <= symbol, i + 65536 - 8 otherwise; fixed lanes aim at 65536
    const int32_t emix_lo = (l < 7) ? l + 1 : 65536;
    const int32_t emix_hi = (l < 7) ? l + 1 + 65536 - 8 : 65536;
    // mantissa models of classes 0..5: symbol s = lane s.  Lanes 0..3 hold the two alphabet-2 AdaptiveModels (class 0 =
    // symbols 0,1; class 1 = symbols 2,3; cdf[1] = 32768), lanes 4..63 the QuasiModels of classes 2..5 (uniform start).
    uint32_t qlo, qhi, qfr, qf = 0;
    const uint32_t lane_cls = (l < 2) ? 0u : (uint32_t)(31 - __clz(l));
    int32_t even_lane = (l < 4 && !(l & 1)) ? 1 : 0, odd_lane = (l < 4 && (l & 1)) ? 1 : 0;
    int32_t sign_lane = even_lane - odd_lane;
    // opaque to the optimiser: three v_mad_i32_i24 per symbol instead of select + add pairs
    asm volatile("" : "+v"(even_lane), "+v"(odd_lane), "+v"(sign_lane));
    uint32_t qa = (l < 4) ? 32768u : 0u;                          // lanes 0..3: cdf[1] of the pair's AdaptiveModel
    {
        const int A = (l < 4) ? 2 : 1 << lane_cls, i = (l < 4) ? (l & 1) : l - A;
        qlo = uniform_cdf(A, i);
        qhi = uniform_cdf(A, i + 1);
        qfr = qhi - qlo;
    }
    // classes 6 and 7: symbol i of the class = lane l of register i / 64 (uniform start, model.cpp:85-95)
    uint32_t hi6[1], lo6[1], fr6[1], f6[1] = {0}, seen6 = 0, expn6 = 8;
    uint32_t hi7[3], lo7[3], fr7[3], f7[3] = {0, 0, 0}, seen7 = 0, expn7 = 8;
    lo6[0] = uniform_cdf(64, l); hi6[0] = uniform_cdf(64, l + 1); fr6[0] = hi6[0] - lo6[0];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int i = l + 64 * j;
        lo7[j] = (i < 129) ? uniform_cdf(129, i) : 65536u;
        hi7[j] = (i < 129) ? uniform_cdf(129, i + 1) : 65536u;
        fr7[j] = hi7[j] - lo7[j];
    }
    uint32_t qexpn = 8;                                          // lane k: EXP of class k + 2 (model.cpp:160-204)
    // lane k < 4: symbols until the rebuild of class k + 2; lanes 4, 5: classes 6, 7 (always due: they decode in the event block)
    uint32_t rem = (l < 4) ? 9u : ((l < 6) ? 1u : 0x40000000u);
    const uint32_t cls_of_lane = (l < 6) ? (uint32_t)l + 2u : 99u;   // lane k counts down for class k + 2
    uint32_t R0, R1, R2, R3;
    {
        uint32_t b[16];
        for (int k = 0; k < 16; k++) { b[k] = bq.take(); bq.top_up(); }
        R0 = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        R1 = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        R2 = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        R3 = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
    }
    uint32_t mysym = 0;
    uint32_t t = 0;
    // whole tiles of 64 symbols: the tile is collected with v_writelane and stored once
    for (; t + 64 <= rlen; t += 64) {
        uint32_t j = 0;
        do {
            JPK_DEC_SYMBOL(R0, R1, j)
            JPK_DEC_SYMBOL(R2, R3, j + 1)
            JPK_DEC_SYMBOL(R0, R1, j + 2)
            JPK_DEC_SYMBOL(R2, R3, j + 3)
            j += 4;
        } while (j < 64);
        out[t + l] = (uint16_t)mysym;
    }
    {
        // the last, partial tile one symbol at a time; the state pairs swap instead of a second copy of the symbol code (the
        // final check below looks at all four states, whichever names they ended up under)
        const uint32_t left = rlen - t;
        for (uint32_t j = 0; j < left; j++) {
            JPK_DEC_SYMBOL(R0, R1, j)
            uint32_t sw = R0; R0 = R2; R2 = sw;
            sw = R1; R1 = R3; R3 = sw;
        }
        if ((uint32_t)l < left) out[t + l] = (uint16_t)mysym;
    }
    // ans.cpp:91-92 (all four states back at the lower bound) and no byte taken from beyond the chunk's payload
    const bool bad = (R0 != RANS_L || R1 != RANS_L || R2 != RANS_L || R3 != RANS_L) || bq.taken() > clen;
    if (bad && l == 0) atomicOr(status, ST_RANS_CHECK);
}
#undef JPK_DEC_SYMBOL
#undef JPK_RENORM2

}  // namespace

namespace jpk_dec {

int run_rans(jpk_ctx *ctx, const DecBufs &b, const uint32_t *order, unsigned g, uint64_t units, size_t chain_lds)
{
    JPK_LAUNCH_LDS(ctx, PROF_DEC_RANS, units, chain_lds, k_dec_rans, dim3(g), dim3(64), b.tab, b.info, order, b.status);
    return JPK_OK;
}

}  // namespace jpk_dec
