// common.hpp -- context, HBM arena and launch helpers shared by all translation units of libjampack_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jampack_abi.h"

#define JPK_HIP(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            if (getenv("JPK_VERBOSE"))                                                                  \
                fprintf(stderr, "[jampack_amd] HIP error %s at %s:%d: %s\n", hipGetErrorName(_e),       \
                        __FILE__, __LINE__, #expr);                                                     \
            return (_e == hipErrorOutOfMemory) ? JPK_E_ALLOC : JPK_E_DEVICE;                            \
        }                                                                                               \
    } while (0)

#define JPK_TRY(expr)                 \
    do {                              \
        int _rc = (expr);             \
        if (_rc != JPK_OK) return _rc; \
    } while (0)

// HBM arena: one allocation per context, bump-allocated per call, grown (free + malloc) when a bigger
// block arrives.  Replaces the reference's five cudaMalloc/cudaFree per block (bwt.cpp:195-239).
// per-kernel HIP-event timing (bench.py roofline): ids index jpk_prof_name()
enum JpkProfId {
    PROF_RS_HIST = 0, PROF_RS_SCATTER, PROF_SCAN, PROF_SA_KEYS, PROF_SA_SEG, PROF_SA_RERANK, PROF_BWT_GATHER,
    PROF_INV_HIST, PROF_INV_BUILD, PROF_INV_WALK, PROF_INV_RANK, PROF_INV_COPY,
    PROF_ENC_HIST, PROF_ENC_MTF, PROF_ENC_RLE, PROF_ENC_CLASS, PROF_ENC_ADAPTIVE, PROF_ENC_PAIRS, PROF_ENC_RANS, PROF_ENC_EMIT,
    PROF_DEC_HEADERS, PROF_DEC_RANS, PROF_DEC_RLE, PROF_DEC_RANK, PROF_CHECKSUM, PROF_LG_HIST, PROF_LG_SCATTER, PROF_SA_PACK, PROF_JAM, PROF_JAM_SCAN,
    PROF_ENC_WRAP, PROF_ENC_LPX, PROF_DD_ANCHOR, PROF_DD_CAND, PROF_DD_EXTEND, PROF_DD_SELECT, PROF_DD_EMIT, PROF_ENC_FILTERS,
    PROF_LZX_PLAN, PROF_LZ77_SIZES, PROF_LZX_COPY, PROF_LZD_PLAN, PROF_LZD_COPY, PROF_PRE_LZ77, PROF_PRE_LPX, PROF_PRE_FILTERS, PROF_COUNT
};
struct JpkProfPending { hipEvent_t a, b; int id; uint64_t units; };

// The mailbox for device->host scalars: one 256-word page, pinned on the host (jpk_ctx::h_mail) with a twin in device memory (d_mail),
// both laid out like this.  Regions that different subsystems use at different times overlap where they always have (a context runs one
// call at a time): the suffix sort's count records and the inverse BWT's verdict; the posted scalars, the inverse BWT's index word and
// the entropy decoder's status word.
struct JpkMail {
    static constexpr int WORDS = 256, READ_WORDS = 16, SA_COUNT_WORDS = 5;
    struct Dec { uint32_t posted[8]; uint32_t status; };              // device: k_dec_rank's status behind jpk_dev_rank_decode (ans_dec_rank.hip; the entry is in ans_dec.hip)
    struct SaCounts { uint32_t m[2], npieces, lc, nrun, pad[3]; };    // the head of the suffix sort's SaState as a round leaves it: five words, stride 8
    struct SaStats { uint32_t round_m[JPK_SA_MAX_ROUNDS], round_lc[JPK_SA_MAX_ROUNDS], bits, depth, vmode; };   // SaState from round_m on
    union {                                  // words 0-15
        uint32_t read[READ_WORDS];           // device: the scalars a kernel posts; host: what jpk_read_mail copied of them (callers take up to 14)
        uint32_t inv_index;                  // host: a trailer's index word (bwt_inv.hip, the 120-chain comparator)
        Dec dec;
    };
    union {                                  // words 16-31
        SaCounts sa_counts[2];               // host: what round r of the suffix sort left, in sa_counts[r & 1] (dead once build_sa returns)
        uint32_t inv_verdict[4];             // both: {status, trailer index, overflow slots, bytes the head chain covers} (jpk_inv_bwt_device)
    };
    SaStats sa_stats;                        // words 32-114, host: stays until jpk_sa_stats_sync has read it (jpk_ctx::sa_stats_pending)
    uint32_t spare0[120 - 32 - (int)(sizeof(SaStats) / 4)];
    uint32_t sa_vmode;                       // word 120, host: the code round 0 of the suffix sort chose
    uint32_t spare1[7];
    uint8_t jam_header[4 * (WORDS - 128)];   // words 128-255, host: one frame header on its way to or from the device (abi.hip, jpk_dev_jam_block_write / _read)
};
static_assert(sizeof(JpkMail) == 4 * JpkMail::WORDS, "the page is 256 words");
static_assert(offsetof(JpkMail, dec.status) == 4 * 8 && offsetof(JpkMail, sa_counts) == 4 * 16 && sizeof(JpkMail::SaCounts) == 4 * 8 &&
              offsetof(JpkMail, inv_verdict) == 4 * 16 && offsetof(JpkMail, sa_stats) == 4 * 32 && offsetof(JpkMail, sa_vmode) == 4 * 120 &&
              offsetof(JpkMail, jam_header) == 4 * 128, "every region is where it was when it was a bare word offset");
static_assert(sizeof(JpkMail::read) <= offsetof(JpkMail, sa_counts) && offsetof(JpkMail, sa_counts) + sizeof(JpkMail::sa_counts) <= offsetof(JpkMail, sa_stats) &&
              offsetof(JpkMail, sa_stats) + sizeof(JpkMail::SaStats) <= offsetof(JpkMail, sa_vmode) && offsetof(JpkMail, sa_vmode) + 4 <= offsetof(JpkMail, jam_header),
              "the suffix sort's regions meet neither one another nor what jpk_read_mail fills while sa_stats_pending is set");
static_assert(JPK_JAM_HEADER_BYTES <= sizeof(JpkMail::jam_header), "a frame header fits");

struct jpk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // entropy stage: chunk groups, densest first; group g runs the whole stage on aux[g], the last group on `stream`
    static constexpr int ENC_GROUPS = 4;
    hipStream_t aux[ENC_GROUPS - 1] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_pre[ENC_GROUPS] = {nullptr, nullptr, nullptr, nullptr}, ev_done[ENC_GROUPS] = {nullptr, nullptr, nullptr, nullptr};
    // one group: the chain runs on a stream of the device's chain pool (chain_pool.hpp), ordered through the host with ev_pre[0] / ev_done[0]
    bool chain_on_pool = false;      // a chain of this context is on a pool stream: the arena must stay (jpk_arena_ensure asserts it)
    // jpk_dev_blocks_decompress of many SMALL blocks: more inverse BWTs side by side than the three of a batch of large ones (an inverse
    // BWT of a 1 MiB block is ~30 dependent launches, each a fraction of the chip).  Streams and events made on first use.
    static constexpr int INV_LANES_MAX = 16;
    hipStream_t inv_lane[INV_LANES_MAX] = {};
    hipEvent_t ev_inv[INV_LANES_MAX] = {};
    hipEvent_t ev_batch = nullptr;                 // jpk_dev_blocks_*: "the caller's stream has reached the batch call"
    hipEvent_t ev_sa[2] = {nullptr, nullptr};      // suffix sort: "the count round r left behind has reached the host"
    bool sa_stats_pending = false;   // per-round statistics of the last suffix sort are still in the pinned mailbox
    uint32_t *h_map = nullptr;       // pinned, 4096 words
    uint8_t *arena = nullptr;
    size_t arena_cap = 0;
    size_t arena_off = 0;
    size_t arena_base = 0;           // where the bump allocator starts (non-zero while a batch runs several stage instances side by side)
    // small pinned host mailbox for device->host scalars
    JpkMail *h_mail = nullptr;    // pinned
    JpkMail *d_mail = nullptr;    // device
    // persistent staging buffers for the host-buffer entry points
    uint8_t *stage_in = nullptr, *stage_out = nullptr, *stage_res = nullptr;
    size_t stage_in_cap = 0, stage_out_cap = 0, stage_res_cap = 0;
    // the archive calls (jpk_dev_jam_compress / _decompress): crcs, frame tables and payload slots of one pass
    uint8_t *jam_scratch = nullptr;
    size_t jam_scratch_cap = 0;
    // jpk_dev_jam_update: the new raw frames of one pass, its gather and splice tables -- apart from jam_scratch, which the reader and
    // the compress pass of the same update use
    uint8_t *jam_update = nullptr;
    size_t jam_update_cap = 0;
    jpk_stats stats;
    // jpk_dev_blocks_lz77_expand: the blocks of the last call that took the parallel path and the serial one (jpk_debug_lz77_expand_last)
    int32_t lzx_parallel = 0, lzx_serial = 0;
    // the same for the deep expander (jpk_dev_blocks_lz77_expand_deep and the staged pass that runs it; jpk_debug_lz77_deep_last)
    int32_t lzd_parallel = 0, lzd_serial = 0;
    // profiler
    bool prof_on = false;
    std::vector<JpkProfPending> prof_pending;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[PROF_COUNT] = {0};
    uint64_t prof_launches[PROF_COUNT] = {0};
    uint64_t prof_units[PROF_COUNT] = {0};
};

void jpk_prof_begin(jpk_ctx *ctx, int id, uint64_t units);
void jpk_prof_end(jpk_ctx *ctx);
void jpk_prof_resolve(jpk_ctx *ctx);   // call after a stream synchronisation

// JPK_LAUNCH(ctx, prof id, units processed, kernel, grid, block, args...)
#define JPK_LAUNCH(ctx, id, units, kernel, grid, block, ...)                                   \
    do {                                                                                       \
        if ((ctx)->prof_on) jpk_prof_begin((ctx), (id), (uint64_t)(units));                    \
        hipLaunchKernelGGL(kernel, grid, block, 0, (ctx)->stream, __VA_ARGS__);               \
        if ((ctx)->prof_on) jpk_prof_end((ctx));                                               \
    } while (0)

// the same with a dynamic LDS reservation (bytes): used to cap the number of resident workgroups of a kernel per CU
#define JPK_LAUNCH_LDS(ctx, id, units, lds, kernel, grid, block, ...)                          \
    do {                                                                                       \
        if ((ctx)->prof_on) jpk_prof_begin((ctx), (id), (uint64_t)(units));                    \
        hipLaunchKernelGGL(kernel, grid, block, (lds), (ctx)->stream, __VA_ARGS__);            \
        if ((ctx)->prof_on) jpk_prof_end((ctx));                                               \
    } while (0)

static inline size_t jpk_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// The one way to read a numeric JPK_* environment switch: unset -> dflt, set -> atol, clamped to [lo, hi].  Callers keep the result in
// a `static const` (the environment is read once per process).
static inline long jpk_env_long(const char *name, long dflt, long lo = LONG_MIN, long hi = LONG_MAX)
{
    const char *e = getenv(name);
    if (!e) return dflt;
    const long v = atol(e);
    return v < lo ? lo : (v > hi ? hi : v);
}

struct Arena {
    jpk_ctx *c;
    size_t need = 0;      // planning pass accumulates here
    bool planning;
    Arena(jpk_ctx *ctx, bool plan) : c(ctx), planning(plan) { if (!plan) c->arena_off = c->arena_base; }
    template <typename T> T *get(size_t count)
    {
        size_t bytes = jpk_align(count * sizeof(T) + 64);
        if (planning) { need += bytes; return nullptr; }
        T *p = (T *)(c->arena + c->arena_off);
        c->arena_off += bytes;
        return p;
    }
};

int jpk_arena_ensure(jpk_ctx *ctx, size_t bytes);
bool jpk_arena_fits(const jpk_ctx *ctx, size_t bytes);      // jpk_arena_ensure(bytes) would keep the arena where it is
int jpk_stage_ensure(jpk_ctx *ctx, size_t in_bytes, size_t out_bytes);
// copy the first `words` posted scalars of the device mailbox to the host (synchronises the stream).  Precondition: words <=
// JpkMail::READ_WORDS -- more would run into the suffix sort's regions of the page
int jpk_read_mail(jpk_ctx *ctx, uint32_t *dst, int words);

static inline unsigned jpk_grid(size_t work, unsigned per_block) { return (unsigned)((work + per_block - 1) / per_block); }

static inline int jpk_bits_for(uint32_t maxval)
{
    int b = 0;
    while (b < 32 && (maxval >> b)) b++;
    return b;
}

// 16 bytes from src (any alignment) through two aligned 16-byte loads (jam.hip, prestage_dev.hip): the caller makes sure that both lie
// inside memory it may read -- a scratch slot with at least 16 bytes of padding behind its payload, or a range it has checked
static __device__ __forceinline__ uint4 load16_unaligned(const uint8_t *src)
{
    const uintptr_t a = (uintptr_t)src;
    const uint4 *p = reinterpret_cast<const uint4 *>(a & ~(uintptr_t)15);
    const uint32_t sh = (uint32_t)(a & 15u);
    const uint4 x = p[0];
    if (sh == 0) return x;
    const uint4 y = p[1];
    const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    const uint32_t q = sh >> 2, r = sh & 3u;
    uint32_t v[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {               // v[i] = w[q + i] by selects (q <= 3): no indexed register array
        uint32_t t = w[i];
        t = q == 1u ? w[i + 1] : t;
        t = q == 2u ? w[i + 2] : t;
        t = q == 3u ? w[i + 3] : t;
        v[i] = t;
    }
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(v[1], v[0], r);
    o.y = __builtin_amdgcn_alignbyte(v[2], v[1], r);
    o.z = __builtin_amdgcn_alignbyte(v[3], v[2], r);
    o.w = __builtin_amdgcn_alignbyte(v[4], v[3], r);
    return o;
}

// ---- primitives implemented in scan.hip / radix.hip -------------------------------------------------
// scratch requirements are sized by the *_scratch_words helpers; all buffers come from the arena.
size_t jpk_scan_scratch_words(size_t n);
int jpk_exclusive_sum_u32(jpk_ctx *ctx, const uint32_t *in, uint32_t *out, size_t n, uint32_t *scratch, uint32_t *d_total /*nullable*/);
int jpk_inclusive_max_u32(jpk_ctx *ctx, const uint32_t *in, uint32_t *out, size_t n, uint32_t *scratch);

size_t jpk_radix_scratch_words(size_t n);
// LSD radix sort on bit ranges; result is left in keys/vals (alt buffers used for ping-pong).  A pass sorts on the 8 key bits from its
// shift up, the last pass on `last_bits` of them (1..8)
int jpk_radix_sort_pairs_u64(jpk_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t *keys_alt, uint32_t *vals_alt, size_t n,
                             const int *shifts, int nshifts, uint32_t *scratch, int last_bits = 8);
int jpk_radix_sort_pairs_u64_nocopy(jpk_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t *keys_alt, uint32_t *vals_alt, size_t n,
                                    const int *shifts, int nshifts, uint32_t *scratch, uint64_t **keys_out, uint32_t **vals_out, int last_bits = 8);
bool jpk_radix_onesweep();   // round 0's radix passes in the one-pass form (default; JPK_ONESWEEP=0: histogram + scan + scatter per pass)
int jpk_radix_sort_slot_keys(jpk_ctx *ctx, uint32_t n, uint64_t *keysA, uint32_t *valsA, uint64_t *keysB, uint32_t *valsB,
                             uint32_t *scratch, uint64_t **keys_out, uint32_t **vals_out, bool group, const uint8_t *slot_tag = nullptr, int tag_shift = 26,
                             uint32_t slot_n = 0);
// compress-side calls (forward BWT, rANS encode) of the contexts of ONE DEVICE that are running right now: the encoder cuts its
// chains into fewer launch groups when other blocks are in flight on the same GPU (abi.hip, the in-flight accounting)
int jpk_compress_inflight_enter(int device);        // returns the count on that device including the caller
void jpk_compress_inflight_leave(int device);
int jpk_enc_groups_for(int inflight, uint32_t nch);
struct JpkCompressInflight {
    int n, device;
    explicit JpkCompressInflight(int dev) : n(jpk_compress_inflight_enter(dev)), device(dev) {}
    ~JpkCompressInflight() { jpk_compress_inflight_leave(device); }
    JpkCompressInflight(const JpkCompressInflight &) = delete;
    JpkCompressInflight &operator=(const JpkCompressInflight &) = delete;
};
// moves the per-round statistics of the last suffix sort from the pinned mailbox into ctx->stats (call after a stream sync)
void jpk_sa_stats_sync(jpk_ctx *ctx);

// ---- what the archive layer (jam_archive.hip) shares with the ABI units (abi.hip, abi_pool.hip, abi_multi.hip), each defined once -------
#define JPK_ENTER(ctx)                         \
    if (!(ctx)) return JPK_E_ARG;              \
    JPK_HIP(hipSetDevice((ctx)->device))
// grows the device buffer *p of ctx to at least `bytes` (its contents are lost; synchronises the stream when it grows)
int jpk_buf_ensure(jpk_ctx *ctx, uint8_t **p, size_t *cap, size_t bytes);
// the calling thread's context from the process-wide pool (borrowed on its first call)
int jpk_tls_ctx(jpk_ctx **out);
// the opening of a host-buffer entry: jpk_tls_ctx, its device current, ctx->stage_in of at least stage_in_bytes
int jpk_host_enter(jpk_ctx **ctx, size_t stage_in_bytes);
// the output slot that always holds the compressed form of a block of len bytes
size_t jpk_multi_comp_cap(int32_t len);
bool jpk_jam_block_size_ok(int32_t bs);
// the 15-byte frame header at h, `avail` bytes from h to the end of the input: the fields, and whether they pass DecompReadBlock's checks
bool jpk_jam_header_parse(const uint8_t *h, int64_t avail, uint32_t *crc, int32_t *psize, int32_t *block_size);
// the 15 bytes of a frame header at h (jpk_jam_header_parse reads them back)
void jpk_jam_header_write(uint8_t *h, uint32_t crc, int32_t psize, int32_t block_size_field);

// ---- stage drivers (device buffers) -----------------------------------------------------------------
int jpk_fwd_bwt_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out);
int jpk_suffix_array_device(jpk_ctx *ctx, const uint8_t *d_t, int32_t n, int32_t *d_sa);
// several small blocks as ONE suffix sort (bwt_fwd.hip): images to d_img[b] (len[b] + 480 bytes each); enqueued, no synchronisation
int jpk_fwd_bwt_group_device(jpk_ctx *ctx, int nblk, const uint8_t *const *d_in, const int32_t *len, uint8_t *const *d_img);
size_t jpk_fwd_bwt_group_arena_bytes(uint32_t total_nlen, int nblk);
int jpk_inv_bwt_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len_with_trailer, uint8_t *d_out);
// no host round trip: d_verdict[0..4) (device) receives {status, trailer index, overflow slots, bytes the head chain covers}
int jpk_inv_bwt_enqueue(jpk_ctx *ctx, const uint8_t *d_in, int32_t len_with_trailer, uint8_t *d_out, uint32_t *d_verdict);
int jpk_inv_bwt_chains120_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len_with_trailer, uint8_t *d_out, float *chase_ms);
int jpk_ans_encode_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
int jpk_ans_decode_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
int jpk_ans_decode_batch(jpk_ctx *ctx, int nblk, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap,
                         int32_t *out_len, int32_t *status, size_t arena_skip);
int jpk_ans_encode_group_device(jpk_ctx *ctx, int nblk, const uint8_t *d_stage, const uint32_t *first_chunk, const int32_t *mid_len, uint8_t *const *d_out,
                                const int32_t *out_cap, int32_t *out_len, int32_t *status);
size_t jpk_ans_encode_group_arena_bytes(uint32_t nchunks, int nblk);
size_t jpk_inv_bwt_arena_bytes(uint32_t n);
size_t jpk_inv_bwt_batch_arena_bytes(int njobs, const int32_t *len_with_trailer);
constexpr int JPK_INV_BATCH_MAX_JOBS = 65535;               // one set of launches, blockIdx.y = the job
void jpk_inv_bwt_batch_plan_add(int32_t len_with_trailer, size_t *job_bytes, size_t *tiles);
size_t jpk_inv_bwt_batch_plan_total(int njobs, size_t job_bytes, size_t tiles);
int jpk_inv_bwt_batch_enqueue(jpk_ctx *ctx, int njobs, const uint8_t *const *d_in, const int32_t *len_with_trailer, uint8_t *const *d_out, uint32_t *d_verdict,
                              const int *verdict_slot, std::vector<uint8_t> &host_jobs);
size_t jpk_fwd_bwt_arena_bytes(uint32_t n);
size_t jpk_ans_encode_arena_bytes(uint32_t len);          // text-like data (0.55 RLE0 symbols per byte); the arena grows for denser blocks
size_t jpk_ans_encode_arena_bytes_worst(uint32_t len);    // every byte a symbol
int jpk_rank_encode_device(jpk_ctx *ctx, uint8_t *d_t, int32_t *d_freq, int32_t len);
int jpk_rank_decode_device(jpk_ctx *ctx, uint8_t *d_r, const int32_t *d_freq, int32_t len);
int jpk_rle_encode_device(jpk_ctx *ctx, const uint8_t *d_ranks, int32_t len, uint16_t *d_rle, int32_t *rlen);
int jpk_model_pairs_device(jpk_ctx *ctx, const uint16_t *d_rle, int32_t rlen, uint32_t *d_pairs);
int jpk_checksum_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint32_t *d_result);
// n segments in one pair of launches, crc i -> d_result[i] (device); synchronises the stream when n > 1
int jpk_checksums_device(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *len, uint32_t *d_result);
// pass 1 of jpk_ans_decode_batch alone: the decoded bytes each Ans stream's chunk headers declare (status[b] != JPK_OK: corrupt);
// synchronises the stream
int jpk_ans_decoded_sizes(jpk_ctx *ctx, int nblk, const uint8_t *const *d_in, const int32_t *in_len, int64_t *decoded, int32_t *status);
// .jam archives (jam.hip).  One frame of the walk: where its payload starts, its header fields
struct JamWalkFrame { uint64_t payload_off; int32_t psize; uint32_t crc; int32_t block_size; int32_t pad; };
// one wave walks up to max_frames frame headers of d_in[0..in_len) from `start`: table[0..count); mail[0] = count, mail[1] = 1 when
// the walk stopped at a bad frame (index count), mail[2..3] = offset where it stopped.  Enqueued only.  staged_ok: staged frames pass, and
// their block_size in the table keeps JPK_JAM_STAGED
int jpk_jam_walk_enqueue(jpk_ctx *ctx, const uint8_t *d_in, uint64_t in_len, uint64_t start, uint32_t max_frames, JamWalkFrame *d_table,
                         uint32_t *d_mail, bool staged_ok = false);
// The plausible frame headers that start in [start, end) of d_in[0..in_len) (jam_resync.hpp), 0 <= start < end <= in_len, in two launches
// around a scan of d_counts (jpk_jam_scan_tiles(d_in, start, end) + 1 words): the count leaves the hits per tile; the emit takes their
// exclusive prefix sums and writes the first max_cands candidates to d_out in ascending order (block_size: the field as it is).  Enqueued.
uint32_t jpk_jam_scan_tiles(const uint8_t *d_in, int64_t start, int64_t end);
int jpk_jam_scan_count_enqueue(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int64_t start, int64_t end, bool staged_ok, uint32_t *d_counts);
int jpk_jam_scan_emit_enqueue(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int64_t start, int64_t end, bool staged_ok, uint32_t *d_counts,
                              JamWalkFrame *d_out, uint32_t max_cands);
// one frame of the pack: its payload slot, its offset in the pass's output, its payload size
struct JamPackFrame { const uint8_t *slot; uint64_t off; int32_t psize; int32_t pad; };
constexpr int JPK_JAM_PASS_FRAMES = 128;                     // frames per pass of the archive calls (and per pack launch)
// writes the frames d_frames[0..n) (n <= JPK_JAM_PASS_FRAMES), headers from d_crc[i] / psize / block_size, into d_out[0..total).  Enqueued.
int jpk_jam_pack_enqueue(jpk_ctx *ctx, const JamPackFrame *d_frames, int n, const uint32_t *d_crc, int32_t block_size, uint8_t *d_out, uint64_t total);
// One piece of a range read (jpk_dev_jam_read): len decoded bytes from src to dst, any alignment.  word0 = the aligned 16-byte destination
// words of the pieces in front of it (a piece has (dst % 16 + len + 15) / 16); [src_lo, src_hi) = the bytes that may be read around src.
struct JamGatherPiece { const uint8_t *src; uint8_t *dst; uint64_t len; uint64_t word0; const uint8_t *src_lo; const uint8_t *src_hi; };
// delivers d_pieces[0..n) (len > 0 each, `words` destination words and `bytes` bytes in all) with one launch.  Enqueued.
int jpk_jam_gather_enqueue(jpk_ctx *ctx, const JamGatherPiece *d_pieces, uint32_t n, uint64_t words, uint64_t bytes);
// One frame of a splice (jpk_dev_jam_update): the frame starts `off` bytes into the stretch that one launch writes.  kept != 0: a frame
// copied from the archive, its header and payload the 15 + psize contiguous bytes at src (crc and field are not looked at); otherwise a new
// frame: src is its payload slot (at least 16 readable bytes behind the payload), the header is made of crc, psize and field (the
// BlockSize field as it is written, JPK_JAM_STAGED included)
struct JamSpliceFrame { uint64_t off; const uint8_t *src; int32_t psize; uint32_t crc; int32_t field; int32_t kept; };
// writes the frames d_frames[0..n) (any n >= 1: the table is read through L2), ascending in off from 0 and back to back, into
// d_out[0..total); a kept frame is read only inside [in_lo, in_hi), the archive.  Enqueued.
int jpk_jam_splice_enqueue(jpk_ctx *ctx, const JamSpliceFrame *d_frames, uint32_t n, uint8_t *d_out, uint64_t total, const uint8_t *in_lo, const uint8_t *in_hi);
// the writer's stage chain on the device (prestage_dev.hip): R -> S2 (k_enc_wrap) into d_mid[b] (jpk_cli_stages_bound - 2 bytes; d_mid ==
// nullptr: in ctx's arena) -> S4 = end token | Lpx::Encode(S2) (k_enc_lpx) into d_out[b] (jpk_cli_stages_bound bytes); in_len[b] < 0
// skips block b.  Two launches; synchronises the stream.  flags & JPK_CLI_DEDUPE: the k_dd_* launches first, R -> S1' into d_out[b], one host
// read of the lengths, then k_enc_wrap from d_out[b] and k_enc_lpx back into it.  s4_len[b] (nullable) = |S4| of block b.
// flags & JPK_CLI_FILTERS: k_enc_filters in the place of k_enc_wrap, same sources, same lengths.
int jpk_cli_stages_device(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_mid, uint8_t *const *d_out,
                          uint32_t flags, int32_t *s4_len);
// the same chain stopped at S2, for staged frames: k_enc_lpx is not launched, d_mid[b] (required) receives S2 and s2_len[b] its length;
// d_tmp[b] (jpk_cli_stages_bound bytes) is where the dedupe leaves S1'
int jpk_staged_stages_device(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_mid, uint8_t *const *d_tmp,
                             uint32_t flags, int32_t *s2_len);
// Lz77::Decompress of n blocks through the deep expander (prestage_dev.hip: k_lzd_plan + k_lzd_copy, k_pre_lz77 for the blocks they leave to
// it): jpk_dev_blocks_lz77_expand_deep behind its argument checks.  Synchronises the stream.
int jpk_lz77_expand_deep_device(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap,
                                int32_t *out_len, int32_t *status);
// S2 of the n bytes at in on the host (prestage.cpp): the stage chain of jpk_cli_stages_encode_ex in front of Lpx::Encode
int jpk_staged_s2_host(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags);
