// ans_enc.hpp -- what the translation units of the rANS encoder share (ans_enc.hip and ans_enc_*.hip only; the overview and the map of
// the units are at the top of ans_enc.hip): the chunk geometry, the buffers, the constants the arena layout needs, the names of the
// encoder's mailbox words, and the host steps encode_core is made of.  Every kernel is defined in one unit, in its anonymous namespace,
// and launched only from that unit; what crosses a unit boundary lives in namespace jpk_enc.
#pragma once
#include "ans_common.hpp"
#include "common.hpp"

namespace jpk_enc {
using namespace jpk;

constexpr int TB = 256;

struct EncDims {
    uint32_t len;         // total bytes
    uint32_t chunk;       // chunk size (ANS_CHUNK, or len for the stand-alone Postcoder entry)
    uint32_t nch;         // chunks
    uint32_t tpc;         // tiles per chunk
    uint32_t ncl;         // chunks of this launch group (<= nch)
    const uint32_t *cmap; // launch index -> chunk id (null: identity).  The densest chunks are launched first as their own
                          // group so that their rANS chains start while the other chunks are still in the parallel stages.
    // group encode (the images of several blocks, each starting at a chunk boundary of one staging buffer: jpk_ans_encode_group_device)
    const uint32_t *clen; // bytes of every chunk (null: one block, the formula below)
    const uint32_t *cblk; // block of every chunk
    uint8_t *const *bout; // output buffer of every block (device array)
    // compact symbol layout (round 4): the arrays indexed by RLE0 symbol (class bytes, ordinals, model outputs, step records, states)
    // give every chunk as many slots as it HAS symbols (rounded up to 256) instead of one per byte: sbase[c] = first slot of chunk c
    // (sbase[nch] = total), lbase[c] = first record of its four rANS lanes.  null: one slot per byte, chunk c at c * stride (probes).
    const uint32_t *sbase;
    const uint32_t *lbase;
};
__device__ __forceinline__ uint32_t chunk_of(const EncDims &d, uint32_t i) { return d.cmap ? d.cmap[i] : i; }
// slots of chunk c in the symbol-indexed arrays, its first slot, and the first record of its lanes (see EncDims::sbase)
__device__ __forceinline__ size_t sym_stride(const EncDims &d, uint32_t c, size_t rle_stride) { return d.sbase ? (size_t)(d.sbase[c + 1] - d.sbase[c]) : rle_stride; }
__device__ __forceinline__ size_t sym_base(const EncDims &d, uint32_t c, size_t rle_stride) { return d.sbase ? (size_t)d.sbase[c] : (size_t)c * rle_stride; }
__device__ __forceinline__ uint32_t chunk_len(const EncDims &d, uint32_t c)
{
    if (d.clen) return d.clen[c];
    uint64_t beg = (uint64_t)c * d.chunk;
    uint64_t left = d.len - beg;
    return left < d.chunk ? (uint32_t)left : d.chunk;
}

// records per state lane, a multiple of the 128-record staging tile
// (a chain is padded with identity steps to whole rounds of the sixteen-batch ring, RANS_PAD = 256 steps: k_rans_lanes)
__host__ __device__ __forceinline__ size_t rans_lane_stride(size_t rle_stride) { return (rle_stride / 2 + 384) & ~(size_t)127; }
// records per lane of chunk c and the first record of its four lanes (see EncDims::sbase)
__device__ __forceinline__ size_t lane_stride_of(const EncDims &d, uint32_t c, size_t rle_stride) { return rans_lane_stride(sym_stride(d, c, rle_stride)); }
__device__ __forceinline__ size_t lane_base(const EncDims &d, uint32_t c, size_t rle_stride) { return d.lbase ? (size_t)d.lbase[c] : (size_t)c * 4 * rans_lane_stride(rle_stride); }

// ---- what the arena layout (ans_enc.hip enc_layout) needs from the chain unit (ans_enc_chain.hip) ------------------------------
constexpr int RANS_RING = 16;                   // batches of records in flight
constexpr int RANS_SLACK = 16 * RANS_RING;      // records in front of the record array: the prefetches of batches that do not exist read there
constexpr int ETILE = 4096;                     // pairs per tile of the emit kernels (k_emit_count, k_put_payload)
constexpr int HDR_MAX = 259 * 5 + 1;            // 1296: bytes of a chunk's header at most (k_headers: 256 + 3 LEB128 fields, 5 bytes each)
inline uint32_t emit_tiles_per_chunk(size_t stride) { return (uint32_t)((2 * stride + ETILE - 1) / ETILE); }

struct EncBufs {
    uint32_t *tilecnt; int32_t *lastpos; int32_t *freq; uint32_t *bstart; uint8_t *ranks;
    uint32_t *lz, *ext, *tcount, *toff, *rlen;
    uint16_t *rle;
    uint32_t *clscnt, *clstotal, *ord, *qhist, *qcdf, *dens, *cmap;
    uint8_t *cls8; uint32_t *clist;
    uint32_t *seg_flag; int32_t *seg_lo, *seg_end, *seg_start; uint16_t *seg_tab, *seg_miss, *seg_reach;
    uint16_t *exph; uint32_t *mantad, *pairs; uint4 *recs;
    uint16_t *x16; uint32_t *emask, *etsum, *fstate, *csize;
    uint64_t *stamp;
    uint8_t *hdr; uint32_t *hsize; uint64_t *outoff;
};

enum { LAY_RANK = 1, LAY_RLE = 2, LAY_MODEL = 4, LAY_RANS = 8, LAY_PLAIN = 16 };

// ---- the encoder's words of the mailbox (JpkMail::read, common.hpp) -----------------------------------------------------------
// Two kernels post there and the host reads what they posted with jpk_read_mail: k_sym_layout the two totals of the compact symbol
// layout (encode_core's front reads MAIL_LAYOUT_WORDS words), k_out_offsets the stream's totals and the diagnostics of the chain that
// ran longest (jpk_ans_encode_device reads MAIL_OFFSETS_WORDS words).  Both post into the same page within one call, and the second
// read must not find the first one's words overwritten by anything else: the two sets are disjoint.  Plain integers: a kernel indexes
// mail[...] with them.
constexpr int MAIL_TOTAL = 0;            // k_out_offsets: bytes of the output stream(s), lo / hi
constexpr int MAIL_RLE_SYMBOLS = 2;      //   RLE0 symbols of all chunks, lo / hi
constexpr int MAIL_CHAIN_CYCLES = 4;     //   the worst chain's cycle stamp (s_memtime), lo / hi
constexpr int MAIL_CHAIN_TICKS = 6;      //   its time stamp (s_memrealtime), lo / hi
constexpr int MAIL_CHAIN_RLEN = 8;       //   its chunk's RLE0 symbols
constexpr int MAIL_SYM_TOTAL = 12;       // k_sym_layout: slots of the symbol-indexed arrays over all chunks (EncDims::sbase)
constexpr int MAIL_LANE_TOTAL = 13;      //   records of the rANS lanes over all chunks (EncDims::lbase)
constexpr int MAIL_OFFSETS_WORDS = 9, MAIL_LAYOUT_WORDS = 14;      // what the two readers ask jpk_read_mail for
static_assert(MAIL_LANE_TOTAL < JpkMail::READ_WORDS && MAIL_SYM_TOTAL < JpkMail::READ_WORDS, "the highest word lies inside JpkMail::read");
static_assert(MAIL_CHAIN_RLEN < MAIL_OFFSETS_WORDS && MAIL_CHAIN_TICKS + 1 < MAIL_OFFSETS_WORDS, "jpk_ans_encode_device's read covers k_out_offsets' words");
static_assert(MAIL_SYM_TOTAL < MAIL_LAYOUT_WORDS && MAIL_LANE_TOTAL < MAIL_LAYOUT_WORDS && MAIL_LAYOUT_WORDS <= JpkMail::READ_WORDS, "the front's read covers k_sym_layout's words");
static_assert(MAIL_SYM_TOTAL >= MAIL_OFFSETS_WORDS && MAIL_LANE_TOTAL >= MAIL_OFFSETS_WORDS && MAIL_SYM_TOTAL != MAIL_LANE_TOTAL, "k_sym_layout's words are none of k_out_offsets' nine");
static_assert(MAIL_TOTAL + 2 == MAIL_RLE_SYMBOLS && MAIL_RLE_SYMBOLS + 2 == MAIL_CHAIN_CYCLES && MAIL_CHAIN_CYCLES + 2 == MAIL_CHAIN_TICKS &&
              MAIL_CHAIN_TICKS + 2 == MAIL_CHAIN_RLEN, "four lo / hi pairs and one word, back to back");

// ---- the host steps, each in the unit that owns its kernels; all enqueue on ctx->stream ----------------------------------------
// ans_enc_front.hip -- rank coding (k_enc_hist, k_enc_prep, k_enc_mtf) and RLE0 (k_rle_lz, k_rle_ext, k_rle_tiles, k_tile_prefix)
int run_rank(jpk_ctx *ctx, const uint8_t *d_in, const EncDims &d, EncBufs &b);
int run_rle(jpk_ctx *ctx, const uint8_t *d_ranks, const EncDims &d, EncBufs &b);
// ans_enc_model.hip -- class ordinals, QuasiModel tables, AdaptiveModel outputs (k_cls_*, k_quasi_build, k_adapt_*); b.qhist is zero on entry
int run_model(jpk_ctx *ctx, const uint16_t *d_rle, const uint32_t *d_rlen, const EncDims &d, EncBufs &b);
// ans_enc_chain.hip -- the back half: step records (k_pairs), the chains (k_rans_lanes), bytes per emit tile (k_emit_count, k_emit_prefix),
// headers and output offsets with the totals -> mailbox (k_headers, k_out_offsets), placement of headers, states and payload into
// `d_out`, or into the blocks' own buffers (EncDims::bout) for a group of blocks (k_put_headers, k_put_payload)
int run_pairs(jpk_ctx *ctx, const uint16_t *d_rle, const uint32_t *d_rlen, const EncDims &d, EncBufs &b);
int run_chain(jpk_ctx *ctx, const EncDims &d, EncBufs &b);
int run_emit_counts(jpk_ctx *ctx, const EncDims &d, EncBufs &b);
int run_offsets(jpk_ctx *ctx, const EncDims &d, EncBufs &b);
int run_put(jpk_ctx *ctx, const EncDims &d, EncBufs &b, uint8_t *d_out);

}  // namespace jpk_enc
