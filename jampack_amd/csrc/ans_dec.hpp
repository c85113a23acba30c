// ans_dec.hpp -- what the translation units of the rANS decoder share (ans_dec.hip and ans_dec_*.hip only; the overview and the map of
// the units are at the top of ans_dec.hip): the chunk and block tables, the names of the words k_dec_headers posts per block, the status
// bits, the two constants host and device code agree on, and the launch steps of the batch.  Every kernel is defined in one unit, in its
// anonymous namespace, and launched only from that unit; what crosses a unit boundary lives in namespace jpk_dec.
#pragma once
#include "ans_common.hpp"
#include "common.hpp"

namespace jpk_dec {
using namespace jpk;

struct ChunkInfo {          // one per chunk, written by the header walk
    uint64_t in_off;        // payload offset in the block's input
    uint32_t clen, olen, rlen;
    uint32_t blk;           // block of the batch this chunk belongs to
    uint64_t out_off;       // offset in the block's decoded output
    uint64_t rle_off;       // offset in the block's packed rle buffer
};

// one block of a batch (jpk_dev_blocks_*): every serial kernel runs ONE grid over the chunks of all blocks, so the number of
// chains in flight does not depend on how many kernels the hardware queues run side by side
struct DecBlock {
    const uint8_t *in;      // Ans stream
    int64_t in_len;
    uint64_t out_cap;
    uint8_t *ranks;         // RLE0 decode writes the rank array here, the rank decoder reads it
    uint8_t *out;           // decoded bytes (the rank decoder's output)
    uint16_t *rle;          // packed RLE0 symbols
    uint32_t cbase;         // first global chunk index of the block
    uint32_t max_chunks;
};

// ---- the words k_dec_headers posts for block b, at mail[MAIL_STRIDE b + ...] of the batch's own mail array in the arena (dec_head,
// ans_dec.hip); the host reads them in dec_plan and jpk_ans_decoded_sizes.  Plain integers: the kernel indexes mail[...] with them.
constexpr int MAIL_STATUS = 0;           // JPK_OK, or why the walk of the block's chunk headers stopped
constexpr int MAIL_CHUNKS = 1;           // chunks of the block
constexpr int MAIL_OUT_TOTAL = 2;        // decoded bytes of all its chunks, lo / hi
constexpr int MAIL_RLE_TOTAL = 4;        // RLE0 symbols of all its chunks, lo / hi
constexpr int MAIL_STRIDE = 8;           // words per block
static_assert(MAIL_STATUS != MAIL_CHUNKS && MAIL_CHUNKS < MAIL_OUT_TOTAL && MAIL_OUT_TOTAL + 2 == MAIL_RLE_TOTAL, "two words and two lo / hi pairs, back to back");
static_assert(MAIL_RLE_TOTAL + 1 < MAIL_STRIDE, "the highest word lies inside the block's stride");

// ---- bits of a block's word of the status array (zero before the stages run; any bit set: the block is JPK_E_CORRUPT, dec_collect)
constexpr uint32_t ST_RANS_CHECK = 1u;       // k_dec_rans: a chain did not end with all four states at RANS_L, or read past its payload
constexpr uint32_t ST_RLE_MISMATCH = 2u;     // k_dec_rle: the RLE0 symbols do not expand to the declared length

// chains (one wave per chunk) that run at once, one per SIMD: up to here the batch reserves LDS to keep them apart (dec_chain_lds),
// beyond it the longest chains are launched first (k_dec_order)
constexpr uint32_t DEC_CHAINS_AT_ONCE = 1024;
// k_dec_rank's own LDS (rows, stage, meta, span: a static_assert beside the kernel ties the number to them); the host takes it off
// the reservation of a chain
constexpr size_t RANK_LDS_BYTES = 16384 + 256 + 4096 + 2048;

// v with lane `lane` = value (both wave-uniform)
// v_writelane with a scalar value AND a scalar lane select needs the lane select in M0 (one SGPR per VALU instruction on gfx9);
// the asm statements that do so name M0 as clobbered, which is what keeps the compiler's own M0 users (the LDS-DMA top-ups) correct
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ uint32_t lane_write(uint32_t v, uint32_t value, uint32_t lane)
{
    // value and lane select are both scalar: the lane select goes through M0 (one SGPR per VALU instruction on gfx9)
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(value), "s"(lane) : "m0");
    return v;
}
#pragma clang diagnostic pop

// ---- the launch steps, each in the unit that owns its kernel; all enqueue on ctx->stream ----------------------------------------
// The arrays one decode pass works on (device pointers into the arena; dec_layout, ans_dec.hip)
struct DecBufs {
    DecBlock *tab;          // the block table
    uint32_t *mail;         // MAIL_STRIDE words per block
    uint32_t *status;       // one word of ST_* bits per block
    ChunkInfo *info;        // one per chunk of the batch, block after block (DecBlock::cbase)
    int32_t *freq;          // 256 per chunk: the header's Freq[]
    uint32_t *order;        // launch index -> chunk, filled beyond DEC_CHAINS_AT_ONCE only
};
// `g` chains, chain i decoding chunk order[i] (null: chunk i); `units` is what the profiler books for the launch; `chain_lds` is the
// LDS a chain's workgroup should take up in all (0: no reservation), which caps the chains resident on a CU.
// ans_dec_rans.hip -- k_dec_rans: payload -> RLE0 symbols (DecBlock::rle)
int run_rans(jpk_ctx *ctx, const DecBufs &b, const uint32_t *order, unsigned g, uint64_t units, size_t chain_lds);
// ans_dec_rank.hip -- k_dec_rle: RLE0 symbols -> ranks (DecBlock::ranks, zeros on entry); k_dec_rank: ranks, freq -> bytes (DecBlock::out)
int run_rle(jpk_ctx *ctx, const DecBufs &b, unsigned g, uint64_t units);
int run_rank(jpk_ctx *ctx, const DecBufs &b, const uint32_t *order, unsigned g, uint64_t units, size_t chain_lds);

}  // namespace jpk_dec
