/*
 * jampack_abi.h -- C ABI of libjampack_amd.so: the MI355X (gfx950) implementation of Jampack's block hot path.
 *
 * Every entry point replaces one interface of the reference (loxxous/Jampack, cited file:line).  Plain
 * pointers and sizes only.  Return value: 0 (JPK_OK) or a negative jpk_status; the library never calls
 * exit() (the reference's Error(), format.cpp:6-10, does -- the C++ shim in jampack_amd/csrc/shim maps a
 * non-zero status back to Error() to stay drop-in).
 *
 * Two families:
 *   host-buffer entry points  jpk_*      -- what the reference's call sites would bind (buffers owned by the
 *                                           caller exactly like `Buffer{block,size}`, format.hpp:36-40); data is
 *                                           staged over PCIe on a per-thread context (re-entrant: jampack.cpp:215,
 *                                           313 call these from OpenMP threads, one Jampack instance each).
 *   device-buffer entry points jpk_dev_*  -- same operations on HBM-resident buffers with an explicit context and
 *                                           stream (used by the fused block pipeline, bench.py and the tests).
 *
 * There is no CPU fallback: without a usable gfx950 device every call returns JPK_E_NODEVICE.
 */
#ifndef JAMPACK_ABI_H
#define JAMPACK_ABI_H

#include <stdint.h>

#if defined(__GNUC__)
#define JPK_API __attribute__((visibility("default")))
#else
#define JPK_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define JPK_BWT_UNITS 120                 /* format.hpp:26  BWT_UNITS */
#define JPK_TRAILER_BYTES (JPK_BWT_UNITS * 4)
#define JPK_ANS_CHUNK (1 << 20)           /* ans.hpp:21     StackSize */
#define JPK_MIN_BLOCKSIZE (1 << 20)       /* format.hpp:21  MIN_BLOCKSIZE */
#define JPK_MAX_BLOCKSIZE (1000 << 20)    /* format.hpp:22  MAX_BLOCKSIZE */
/* the forward BWT (jpk_bwt_forward, jpk_block_compress and their jpk_dev_ / batch forms) takes in_len < JPK_FWD_BWT_LIMIT and returns
 * JPK_E_ARG above (the sort keeps the two upper bits of a 32-bit rank for flags): the format's largest block is below it */
#define JPK_FWD_BWT_LIMIT (1u << 30)
#define JPK_SA_MAX_ROUNDS 40               /* rounds reported in jpk_stats (h doubles: 7 * 2^31 > any block) */
#define JPK_JAM_HEADER_BYTES 15           /* jampack.cpp:128-131: "JAM" + crc + payload size + BlockSize */

typedef enum jpk_status {
    JPK_OK = 0,
    JPK_E_ARG = -1,        /* null pointer / negative size */
    JPK_E_CAPACITY = -2,   /* output buffer too small (the reference would overflow) */
    JPK_E_CORRUPT = -3,    /* malformed stream (reference: Error("...") at ans.cpp:92, 298; rle.cpp:72; rank.cpp:107) */
    JPK_E_DEVICE = -4,     /* HIP runtime error */
    JPK_E_ALLOC = -5,      /* device/host allocation failed */
    JPK_E_NODEVICE = -6    /* no gfx950 device visible */
} jpk_status;

typedef struct jpk_ctx jpk_ctx;

/* per-call statistics of the last operation on a context (for bench.py / DESIGN.md accounting) */
typedef struct jpk_stats {
    int32_t sa_rounds;            /* prefix-doubling rounds of the last forward BWT */
    int32_t sa_key_depth;         /* symbols of a suffix that round 0's key holds: the average over the block with the variable-length codes
                                   * (order 0: about 56 / H0 -- 12 for English-like text, 10 over enwik8's byte alphabet; with the order-1 /
                                   * order-2 context codes 13-15), exactly floor(56 / ceil(log2 sigma)) with the fixed-width code (flat
                                   * histograms, blocks above 2^28 bytes, JPK_VARKEYS=0): 7 above 128 byte values */
    int64_t sa_sorted_elems;      /* sum over rounds of active suffixes that went through a sort */
    int64_t inv_splitters;        /* walkers used by the last inverse BWT */
    int64_t inv_overflow_slots;   /* overflow slots chained by the last inverse BWT: a sub-list of L bytes adds (L - 1) / 256 */
    int64_t workspace_bytes;      /* HBM arena currently held by the context */
    int64_t ans_chunks;           /* 1 MiB chunks in the last entropy call */
    int64_t ans_rle_symbols;      /* RLE0 symbols in the last entropy call */
    /* per round r (r = 0: the radix round on the key; r >= 1: every group of tied suffixes compared at its own depth -- sa_key_depth * 2^(r-1)
     * with the fixed-width code -- or a pair round, see sa_pair_rounds) of the last forward BWT:
     * suffixes still unresolved when the round starts / of those, members of groups too large for the LDS path */
    int32_t sa_round_active[JPK_SA_MAX_ROUNDS];
    int32_t sa_round_large[JPK_SA_MAX_ROUNDS];
    /* the rANS chunk whose four state chains ran longest in the last entropy encode (the serial floor of the stage):
     * shader cycles, nanoseconds (from the 100 MHz real-time counter), encoder steps per chain */
    int64_t enc_chain_cycles;
    int64_t enc_chain_ns;
    int64_t enc_chain_steps;
    /* bit r set: round r of the last forward BWT was a pair round (the induction step over long repeats, bwt_fwd.hip k_pair_*: it
     * resolves whole groups from the order of their successors and leaves the doubling distance alone) instead of a doubling round;
     * r >= 1 then stands for the r-th round after round 0, h = sa_key_depth * 2^(doubling rounds before it) */
    int64_t sa_pair_rounds;
    /* the code of round 0's keys in the last forward BWT: -1 = fixed width, 0 = the variable-length code of the bytes alone, 1 / 2 = every
     * symbol behind the one / the two bytes in front of it (chosen per block from a sample) */
    int32_t sa_key_order;
    int32_t reserved0;
} jpk_stats;

/* ---- contexts ------------------------------------------------------------------------------------------ */
/* stream: a hipStream_t to launch on (NULL = the context creates its own non-blocking stream).
 * Replaces the reference's per-call cudaMalloc/cudaMemcpy/cudaFree staging (bwt.cpp:189-239). */
JPK_API int jpk_ctx_create(jpk_ctx **out, int device, void *hip_stream);
JPK_API void jpk_ctx_destroy(jpk_ctx *ctx);
JPK_API int jpk_ctx_stats(jpk_ctx *ctx, jpk_stats *out);
/* pre-size the HBM arena for blocks up to max_block_bytes (otherwise it grows on demand): the maximum of the four stages' own
 * layouts (jpk_debug_arena_bytes).  JPK_E_ARG for max_block_bytes < 0 or > JPK_MAX_BLOCKSIZE, JPK_E_ALLOC when HBM is short. */
JPK_API int jpk_ctx_reserve(jpk_ctx *ctx, int64_t max_block_bytes);
/* per-kernel timing with HIP events recorded on the context's stream: enable = 1 on, 2 on + reset, 0 off + reset.
 * id < jpk_ctx_profile_count(); units = elements the timed launches processed (see DESIGN.md for bytes per unit). */
JPK_API int jpk_ctx_profile(jpk_ctx *ctx, int enable);
JPK_API int jpk_ctx_profile_count(void);
JPK_API const char *jpk_ctx_profile_name(int id);
JPK_API int jpk_ctx_profile_get(jpk_ctx *ctx, int id, double *ms, int64_t *launches, int64_t *units);
JPK_API int jpk_device_count(void);
JPK_API const char *jpk_strerror(int status);
JPK_API const char *jpk_version(void);

/* ---- process-wide set-up of the host-buffer entry points -------------------------------------- */
/* Selects the devices the host-buffer entry points may use: bit d of device_mask = HIP device d, 0 = every visible
 * gfx950 device.  Calling threads are dealt round robin over the selected devices and keep a persistent context
 * (stream + HBM arena + staging) from a process-wide pool, so the OpenMP block loop of jampack.cpp:215/313 spreads
 * its blocks over the node.  Returns the number of devices selected (> 0) or a negative jpk_status.  Optional: without
 * it the first host-buffer call selects all devices (or the one named by the JPK_DEVICE environment variable).
 * Replaces the reference's per-block cudaMalloc/cudaFree and its single-device choice (bwt.cpp:98-114, 189-239). */
JPK_API int jpk_init(uint64_t device_mask);
/* the devices selected by jpk_init (or by the implicit selection), in round-robin order; returns their count */
JPK_API int jpk_init_devices(int32_t *devices, int32_t cap);
/* device the calling thread has been dealt (creates its context if needed), or a negative jpk_status */
JPK_API int jpk_thread_device(void);
/* destroys every pooled context (arenas, streams, staging).  No host-buffer call may be in flight.  Threads that call
 * again afterwards get fresh contexts. */
JPK_API void jpk_shutdown(void);
/* gives back what the batch entries keep between calls and nobody is using right now: the idle worker contexts of
 * jpk_dev_blocks_compress / jpk_dev_blocks_decompress (one arena each: ~54 bytes per block byte of the largest block they have seen) and
 * the multi-device entries' slabs.  May run beside other calls; they create what they need again.  Returns the contexts destroyed.
 * (The reference frees its device buffers after every block: bwt.cpp:98-114.) */
JPK_API int jpk_release_idle(void);

/* ---- host-buffer entry points (drop-in boundary) ------------------------------------------------------- */
/* BlockSort::Bwt::ForwardBwt(Buffer,Buffer)            bwt.hpp:15, bwt.cpp:22-65.   *out_len = in_len + 480.  in_len < JPK_FWD_BWT_LIMIT. */
JPK_API int jpk_bwt_forward(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* BlockSort::Bwt::InverseBwt(Buffer,Buffer,Options)    bwt.hpp:16, bwt.cpp:72-282.  threads/use_gpu mirror
 * Options.Threads / Options.Gpu (format.hpp:46-54); they do not change the bytes and are accepted for ABI fidelity. */
JPK_API int jpk_bwt_inverse(const uint8_t *in, int32_t in_len_with_trailer, uint8_t *out, int32_t out_cap, int32_t *out_len,
                    int32_t threads, int32_t use_gpu);
/* Ans::Encode(Buffer,Buffer,Options)                   ans.hpp:32, ans.cpp:113-234. The reference clobbers its
 * input (rank.cpp:88); this implementation leaves it intact but the contract still allows clobbering. */
JPK_API int jpk_ans_encode(uint8_t *in_clobbered, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* Ans::Decode(Buffer,Buffer,Options)                   ans.hpp:33, ans.cpp:236-270 */
JPK_API int jpk_ans_decode(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t threads);
/* Header-only walk of an Ans stream (ReadHeader per chunk, ans.cpp:254-261, 287-302) on the host: the decoded length
 * (sum of the chunks' original lengths) and the chunk count, with the reference's header sanity checks.  The reference's
 * Ans::Decode has no capacity argument -- it trusts that the caller's buffer holds the frame (jampack.cpp:156-159) -- so the
 * C++ shim uses this to bound jpk_ans_decode by what the stream itself declares instead of by Options.BlockSize, which on
 * the decompress path is the CLI default, not the frame's block size (main.cpp:60, jampack.cpp:146-159). */
JPK_API int jpk_ans_decoded_size(const uint8_t *in, int32_t in_len, int64_t *decoded_len, int32_t *chunks);
/* Postcoder::Encode / Decode                           rank.hpp:12-13, rank.cpp:45-151 (in place) */
JPK_API int jpk_rank_encode(uint8_t *t, int32_t *freq256, int32_t len);
JPK_API int jpk_rank_decode(uint8_t *ranks, const int32_t *freq256, int32_t len);
/* fused Jampack::Comp()/Decomp() tail: ForwardBwt -> Ans::Encode / Ans::Decode -> InverseBwt with the BWT
 * image kept in HBM between the two stages (jampack.cpp:40-41, 49-50). */
JPK_API int jpk_block_compress(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_block_decompress(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* Checksum::IntegrityCheck(Buffer)                     checksum.hpp:15, checksum.cpp:12-36 */
JPK_API int jpk_checksum(const uint8_t *in, int32_t in_len, uint32_t *crc);
/* One framed block of a .jam stream: Jampack::Comp() (crc of the input, jampack.cpp:31) + CompWriteBlock
 * (jampack.cpp:122-135):  "JAM" | u32 crc | i32 payload size | i32 BlockSize | payload   (15-byte header, LE).
 * The payload is jpk_block_compress(in): the reference CLI additionally runs its LZ77 / filter / LPX pre-stages in
 * front of the BWT (jampack.cpp:33-38), so these frames interchange with a reference build whose Comp()/Decomp() call
 * this path; an unmodified `jampack d` rejects them.  jpk_jam_cli_block_write below writes the frame
 * the stock CLI decodes.  block_size is Options.BlockSize and must lie in
 * [JPK_MIN_BLOCKSIZE, JPK_MAX_BLOCKSIZE] with in_len <= block_size. */
JPK_API int jpk_jam_block_write(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* DecompReadBlock + Decomp() (jampack.cpp:140-164, 47-60): validates the header exactly as the reference does
 * (magic, BlockSize range, 0 <= payload size <= MAX_BLOCKSIZE), decodes the payload and checks the crc.
 * *consumed = 15 + payload size (where the next frame starts).  JPK_E_CORRUPT on a bad header, a payload that
 * runs past in_len, or a crc mismatch ("Detected corrupt block!", jampack.cpp:59). */
JPK_API int jpk_jam_block_read(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t *consumed);

/* ---- pre-stage decoders, stored-form encoders + frames of the stock CLI (host code) ------- */
/* Lz77::Decompress(Buffer,Buffer)                      lz77.hpp:22, lz77.cpp:678-714 */
JPK_API int jpk_lz77_decompress(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* Lpx::Decode(Buffer,Buffer,Options)                   lpx.hpp:32, lpx.cpp:101-169 (output length = input length) */
JPK_API int jpk_lpx_decode(const uint8_t *in, int32_t len, uint8_t *out);
/* Lpx::Encode(Buffer,Buffer,Options)                   lpx.hpp:31, lpx.cpp:56-99, 148-158 (output length = input length),
 * bit-identical to the reference; jpk_lpx_decode(jpk_lpx_encode(x)) == x */
JPK_API int jpk_lpx_encode(const uint8_t *in, int32_t len, uint8_t *out);
/* Filters::Decode(Buffer,Buffer)                       filters.hpp:44, filters.cpp:442-490 */
JPK_API int jpk_filters_decode(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* Checksum::IntegrityCheck on the host                 checksum.cpp:12-36 */
JPK_API uint32_t jpk_checksum_host(const uint8_t *p, int32_t size);
/* One frame written by an unmodified `jampack c` (any -m / -f setting): DecompReadBlock + the whole Jampack::Decomp()
 * (jampack.cpp:47-60, 140-164) -- Ans::Decode and InverseBwt on the GPU, Lz77::Decompress, Lpx::Decode,
 * Filters::Decode, Lz77::Decompress on the host, then the crc check.  *consumed = 15 + payload size. */
JPK_API int jpk_jam_cli_block_read(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t *consumed);

/* The stages the stock CLI's decoder undoes behind its inverse BWT, written WITHOUT match finding or filter selection (the format
 * lets LZ77 and Filters be written as "stored"; Lpx::Encode runs exactly; the _ex forms below add a dedupe and a filter choice as
 * options).  For a raw block R of n bytes:
 *   S1 = 04 80 | R                  the LZ77 end token (offset 0: the rest are literals, lz77.cpp:620, 705-711)
 *   S2 = every 64 KiB piece of S1 behind a 00 00 header (raw, filters.cpp:421-426); split as filters.cpp:245
 *   S3 = Lpx::Encode(S2),  S4 = 04 80 | S3
 * jpk_cli_stages_bound: |S4| = n + 4 + 2 * ceil((n + 2) / 65536), exact (JPK_E_ARG, < 0, for n < 0).  jpk_cli_stages_encode writes S4:
 * *out_len = the bound, JPK_E_CAPACITY when out_cap is below it.  The stock encoder's output for the same block differs (it finds
 * matches and picks filters); both decode to R. */
JPK_API int64_t jpk_cli_stages_bound(int64_t n);
JPK_API int jpk_cli_stages_encode(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* The counterpart of jpk_jam_cli_block_read: one frame an unmodified `jampack d` decodes -- the 15-byte header of jpk_jam_block_write
 * (crc of `in`, payload size, BlockSize) + jpk_block_compress(S4).  The stages run on the host, ForwardBwt + Ans::Encode on the GPU.
 * Arguments as jpk_jam_block_write: block_size in [JPK_MIN_BLOCKSIZE, JPK_MAX_BLOCKSIZE], in_len <= block_size (JPK_E_ARG), out_cap
 * below the header or the frame JPK_E_CAPACITY.  With the BWT trailer S4 fits the decoder's (int)(BlockSize * 1.05) stage buffers
 * (jampack.cpp:157) for every such in_len (the arithmetic is in prestage.cpp). */
JPK_API int jpk_jam_cli_block_write(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len);

/* The dedupe of the stock encoder's first LZ77 stage (Jampack::Comp(), jampack.cpp:34-36: Lz->Compress with MatchFinder = 0, lz77.cpp:544-625
 * "Deduplicate big chunks"): repeats of at least 256 bytes inside the block leave as tokens of Lz77::WriteToken (lz77.cpp:53-70), the rest as
 * literals, the end token 04 80 in front of the last literals.  The token STREAM is not the reference's -- the matches come from a rule
 * that runs in parallel (anchors at every 64th byte, a slot table that keeps the smallest position, runs of matching windows, greedy
 * selection in position order; DESIGN 4.7 "Dedupe") -- but every decoder of the format reads it: jpk_lz77_decompress(S1') == R.
 * |S1'| <= n + 2, a block without a qualifying repeat gives exactly 04 80 | R, the bytes depend on R alone, and the work is O(n) for every
 * R.  *out_len = |S1'|; JPK_E_CAPACITY (nothing written, *out_len = 0) when out_cap is below it. */
JPK_API int jpk_lz77_dedupe(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* flags of the _ex forms of the stock-CLI writer.  JPK_CLI_DEDUPE: S1 = jpk_lz77_dedupe(R) instead of 04 80 | R; the rest of the chain is
 * unchanged (stored filter pieces over S1, Lpx::Encode, stored second LZ77), so out_len depends on the data and jpk_cli_stages_bound /
 * jpk_jam_cli_compress_bound stay bounds.  flags = 0 is the entry without _ex, byte for byte; any other bit is JPK_E_ARG. */
/* The writer of staged frames (jpk_jam_staged_block_write, jpk_*_jam_staged_compress) takes the same two flags with the same meaning
 * for S1 and S2, and stops the chain there. */
#define JPK_CLI_DEDUPE 1
/* JPK_CLI_FILTERS: every 64 KiB piece of S1 (of the dedupe's S1' with both flags) goes through the filter choice of DESIGN 4.7 "Filters" and
 * leaves as `type, width | transformed piece` (type 0 = reorder + delta, type 2 = in-place delta, widths 1..32) when a candidate's integer
 * order-0 cost beats the raw piece's by more than a sixteenth, as `00 00 | piece` otherwise.  Lengths do not change.  It is bit 2, not bit
 * 1: the values 2 and 3 were refused before this flag existed and stay refused (tests/test_dedupe_host.py pins them).  The accepted values
 * of flags are exactly 0, 1, 4 and 5. */
#define JPK_CLI_FILTERS 4
#define JPK_CLI_FLAGS_OK(f) (((f) & ~(uint32_t)(JPK_CLI_DEDUPE | JPK_CLI_FILTERS)) == 0u)
/* Filters::Encode (filters.hpp:43) with that choice: S2 of in_len bytes of S1, *out_len = in_len + 2 * ceil(in_len / 65536); JPK_E_CAPACITY
 * (nothing written) when out_cap is below it.  jpk_filters_decode gives `in` back, and so does the reference's Filters::Decode. */
JPK_API int jpk_filters_encode(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len);
/* the rule's cost (1/4096 bit) of one candidate for one piece of len bytes in [1, 65536]: type 0 or 2 at width 1..32, width 0 = raw (type
 * ignored); computed from the candidate's actual output bytes.  JPK_E_ARG otherwise. */
JPK_API int jpk_filters_cost(const uint8_t *piece, int32_t len, int32_t type, int32_t width, int64_t *cost);
JPK_API int jpk_cli_stages_encode_ex(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags);
JPK_API int jpk_jam_cli_block_write_ex(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags);

/* ---- device-buffer entry points (all pointers except ctx/out_len are HBM addresses on ctx's device) ---- */
/* ADDRESSES AND BOUNDS of every jpk_dev_* stage entry and probe (tests/test_gpu_stage_contracts.py, tests/test_gpu_primitives.py):
 *   - a byte buffer (const uint8_t *d_in, uint8_t *d_out, the in-place d_t / d_ranks) may start at ANY address and have any length: the
 *     kernels peel to their vector width themselves;
 *   - a typed array (int32_t *d_freq256 / d_sa, uint16_t *d_rle, uint32_t *d_pairs / d_vals / d_data, uint64_t *d_keys) needs the
 *     alignment of its element type and no more;
 *   - a call writes NOTHING outside [d_out, d_out + out_cap), whatever it returns (JPK_E_CAPACITY included), and leaves a const input as
 *     it found it -- jpk_dev_ans_encode too, like jpk_ans_encode;
 *   - on JPK_OK it writes nothing at or beyond d_out + *out_len: capacity the call did not need keeps the caller's bytes;
 *   - out_cap is exact: *out_len bytes fit out_cap == *out_len, and one byte less is JPK_E_CAPACITY.
 * The in-place entries and the probes that name no capacity write exactly their result: len bytes, int32[256] frequencies, int32[n]
 * suffixes, *rlen uint16 symbols (jpk_dev_rle_encode; at most len), 2 * rlen uint32 words (jpk_dev_model_pairs), n keys / values / words. */
JPK_API int jpk_dev_bwt_forward(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_dev_bwt_inverse(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len_with_trailer, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_dev_ans_encode(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_dev_ans_decode(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_dev_rank_encode(jpk_ctx *ctx, uint8_t *d_t, int32_t *d_freq256, int32_t len);
JPK_API int jpk_dev_rank_decode(jpk_ctx *ctx, uint8_t *d_ranks, const int32_t *d_freq256, int32_t len);
JPK_API int jpk_dev_block_compress(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_dev_block_decompress(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_dev_checksum(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, uint32_t *crc);
JPK_API int jpk_dev_jam_block_write(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, int32_t block_size, uint8_t *d_out, int32_t out_cap, int32_t *out_len);
JPK_API int jpk_dev_jam_block_read(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len, uint8_t *d_out, int32_t out_cap, int32_t *out_len, int32_t *consumed);

/* ---- batches of independent blocks (device buffers) ------------------------------------------------------------ */
/* Jampack::Decompress's multi-block mode (jampack.cpp:286-317: Threads blocks read, Decomp() in an OpenMP loop, written in
 * order) for blocks that already sit in HBM: Ans::Decode (+ InverseBwt) of nblocks independent blocks in ONE pass -- every
 * serial entropy kernel runs a single grid over the 1 MiB chunks of all blocks, which is what fills the GPU (one block is 65
 * chains on 1024 SIMDs).  Arrays of nblocks device pointers / sizes (the arrays themselves are host memory).  status may be
 * NULL; otherwise status[b] receives block b's jpk_status and a corrupt block does not stop the others.
 * jpk_dev_blocks_decompress: the inverse BWTs follow on up to three streams of the context; a batch of many small blocks (>= 32 blocks
 * of <= 4 MiB, a stream of the reference's smallest block size, format.hpp:22) runs them through one set of launches over all blocks
 * and needs scratch for all of them at once (about 10 bytes per block byte of the context's arena). */
JPK_API int jpk_dev_blocks_ans_decode(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                              const int32_t *out_cap, int32_t *out_len, int32_t *status);
JPK_API int jpk_dev_blocks_decompress(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                              const int32_t *out_cap, int32_t *out_len, int32_t *status);

/* The compress direction of the same loop (jampack.cpp:205-224: Threads blocks read, Comp() in an OpenMP loop, written in order)
 * for blocks that sit in HBM: ForwardBwt + Ans::Encode of nblocks independent blocks in ONE call.  Compression wants several
 * blocks IN FLIGHT rather than one wide grid (the suffix sort fills the GPU by itself; the entropy stage of the other blocks
 * hides in its latency), so the library runs `in_flight` worker threads (<= 0: 10; at most 16), each with a context of its own on
 * ctx's device (kept by the library between calls, released by jpk_shutdown), that take the work in array order.  Blocks of up to
 * 16 MiB -- the reference's default block is 8 MiB, its smallest 1 MiB (format.hpp:20-22) -- are compressed in GROUPS of
 * consecutive blocks (a quarter of their total bytes, 8 .. 64 MiB, at most 256 blocks; JPK_GROUP_MIB fixes the size, JPK_GROUP=0
 * turns grouping off): one suffix sort over the blocks of a group, one set of entropy grids over all their chunks, and a handful of
 * host synchronisations per group instead of one per block -- the suffix sort's per-round counts from its third round on, the symbol
 * layout, the chunk sizes and the end of the emit kernels (one more when a block does not fit its buffer); every block's bytes are those
 * of jpk_dev_block_compress for that block.  A group that fails as a whole (its arena, a device error) is retried block by block through
 * the single-block path on the same context; a block whose out_cap is too small reports JPK_E_CAPACITY alone.
 * The calling thread works too (with ctx) and returns when every block is done.  status may be NULL; otherwise
 * status[b] receives block b's jpk_status (JPK_E_CAPACITY when out_cap[b] is too small, ...) and the other blocks still complete.
 * Stream order: as for every jpk_dev_* call, work already queued on ctx's stream (the producers of d_in[], readers of an earlier
 * d_out[]) is ordered in front of the batch -- the workers' streams wait for an event recorded on ctx's stream at entry -- and
 * every block is complete when the call returns. */
JPK_API int jpk_dev_blocks_compress(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                            const int32_t *out_cap, int32_t *out_len, int32_t *status, int32_t in_flight);

/* ---- whole .jam archives (Jampack::Compress / Jampack::Decompress, jampack.cpp:186-336) ---------------------------------------- */
/* Checksum::IntegrityCheck of n device segments (any length 0 .. 2^31 - 1, any start address) in one launch pair; crc[i] (host
 * array) receives segment i's checksum.  jpk_dev_checksum is the batch of one. */
JPK_API int jpk_dev_checksums(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint32_t *crc);
/* the largest archive in_len bytes can produce with this block size (0 for in_len 0); JPK_E_ARG (< 0) for a bad argument */
JPK_API int64_t jpk_jam_compress_bound(int64_t in_len, int32_t block_size);
/* The archive of `jampack c` (frames of the block path, no LZ77 / LPX / filter pre-stages): bytes identical to the concatenation of
 * jpk_dev_jam_block_write over consecutive block_size slices of d_in, the last one short; in_len == 0 gives an empty archive.
 * block_size in [JPK_MIN_BLOCKSIZE, JPK_MAX_BLOCKSIZE].  Runs through jpk_dev_blocks_compress (in_flight as there: worker contexts,
 * blocks in flight, groups of small blocks): per pass one batched checksum of the slices, the batch compress into payload slots, one
 * pack launch that writes the frames.  JPK_E_CAPACITY when the archive does not fit out_cap (jpk_jam_compress_bound always does).
 * Per-pass HBM: passes of at most 128 frames and 4 GiB of input; the slots take jpk_jam_compress_bound of the pass (about 1.25 bytes
 * per input byte, <= 5.2 GB) in a scratch buffer of ctx, on top of the workers' arenas of jpk_dev_blocks_compress. */
JPK_API int jpk_dev_jam_compress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                 int32_t in_flight);
/* The inverse (Jampack::Decompress, jampack.cpp:262-336, without pre-stages): a frame walk over the whole archive with the checks of
 * DecompReadBlock (jampack.cpp:140-163: magic, BlockSize range, 0 <= payload size <= MAX_BLOCKSIZE, the payload inside the archive;
 * 1..14 trailing bytes are a bad frame), every payload's decoded size from its chunk headers (at least the BWT trailer, at most
 * BlockSize raw bytes), then per pass jpk_dev_blocks_decompress with every frame decoded in place in d_out and one batched checksum
 * compared with the header crcs.
 *   out_cap too small: JPK_E_CAPACITY, *out_len = the bytes needed, nothing written (out_cap = 0 is the size query).
 *   bad frame k (header, payload or crc): its status (JPK_E_CORRUPT), *bad_frame = k, *frames = k, *out_len = the raw bytes of frames
 *   0..k-1, which are verified and in place; bytes past them are unspecified (the reference stops at the first corrupt block).
 *   success: *frames = the frame count, *bad_frame = -1.  frames and bad_frame may be NULL.
 * Per-pass HBM: passes of at most 128 frames and 4 GiB of raw bytes; the batch decoder's arena on ctx takes about 4 bytes per raw byte
 * of the pass (the BWT images, the rank arrays, the RLE0 symbols) plus the inverse BWT's scratch (jpk_dev_blocks_decompress). */
JPK_API int jpk_dev_jam_decompress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len, int32_t *frames,
                                   int32_t *bad_frame);
/* host-buffer forms of the two: staged one pass at a time through the calling thread's pooled context, same contracts */
JPK_API int jpk_jam_compress(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight);
JPK_API int jpk_jam_decompress(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frames, int32_t *bad_frame);
/* host walk of an archive in host memory with the checks of jpk_dev_jam_decompress's walk (the decoded sizes by jpk_ans_decoded_size):
 * *frames / *raw_len = count and exact raw bytes of the frames in front of the first bad one, *bad_frame = its index (JPK_E_CORRUPT)
 * or -1 (JPK_OK).  No device call.  Pointers other than in may be NULL. */
JPK_API int jpk_jam_frames(const uint8_t *in, int64_t in_len, int32_t *frames, int64_t *raw_len, int32_t *bad_frame);

/* ---- archives of the stock CLI: the pre-stage decoders on the device, whole archives in one batched call ---------------------------- */
/* The three decoders the stock `jampack c` needs behind Ans::Decode + InverseBwt (Jampack::Decomp(), jampack.cpp:47-60), for n independent
 * blocks that sit in HBM, one launch per call.  Arrays of n device pointers / sizes (the arrays themselves are host memory) as for
 * jpk_dev_blocks_ans_decode; status may be NULL (the call then returns the first failing block's status), otherwise status[b] receives
 * block b's jpk_status and a bad block does not stop the others.  Output and status are those of the host decoders (jpk_lz77_decompress,
 * jpk_lpx_decode, jpk_filters_decode) on the same bytes; the buffer of a failed block is unspecified inside [d_out, d_out + out_cap).
 * ADDRESSES AND BOUNDS above holds; input and output of a block must not overlap.
 *   Lz77::Decompress(Buffer,Buffer)            lz77.hpp:22, lz77.cpp:678-714    one workgroup per block */
JPK_API int jpk_dev_blocks_lz77_decompress(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                           const int32_t *out_cap, int32_t *out_len, int32_t *status);
/*   Lpx::Decode(Buffer,Buffer,Options)         lpx.hpp:32, lpx.cpp:101-169      one workgroup per part (len / 4 bytes), one lane runs its model;
 *   writes exactly len[b] bytes; every byte string is a valid stream */
JPK_API int jpk_dev_blocks_lpx_decode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *len, uint8_t *const *d_out, int32_t *status);
/*   Filters::Decode(Buffer,Buffer)             filters.hpp:44, filters.cpp:442-490   one workgroup per 64 KiB filter block */
JPK_API int jpk_dev_blocks_filters_decode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                          const int32_t *out_cap, int32_t *out_len, int32_t *status);
/*   Lpx::Encode(Buffer,Buffer,Options)         lpx.hpp:31, lpx.cpp:56-99, 148-158   the mirror image: one workgroup per part, one lane runs
 *   its model over the input; the bytes of jpk_lpx_encode; writes exactly len[b] bytes */
JPK_API int jpk_dev_blocks_lpx_encode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *len, uint8_t *const *d_out, int32_t *status);
/*   the whole stage chain of jpk_cli_stages_encode, two launches for all blocks (the stored forms, then Lpx::Encode; S2 lives in ctx's
 *   arena): out_len[b] = jpk_cli_stages_bound(in_len[b]), the bytes of the host form.  A block whose out_cap is below that reports
 *   JPK_E_CAPACITY alone, out_len[b] = 0, and nothing of it is written. */
JPK_API int jpk_dev_blocks_cli_stages_encode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                             const int32_t *out_cap, int32_t *out_len, int32_t *status);
/*   jpk_lz77_dedupe of n blocks, the bytes and statuses of the host form (kernels k_dd_*): the anchor table, the heads per tile, their
 *   runs, one selection chain per block, then -- behind ONE host read of the blocks' lengths -- the emit by destination.  A block whose
 *   out_cap is below its |S1'| reports JPK_E_CAPACITY alone, out_len[b] = 0, and nothing of it is written.  Scratch in ctx's arena: about
 *   1.2 bytes per input byte (the slot table <= 0.5, the heads 0.5, the tokens 0.125). */
JPK_API int jpk_dev_blocks_lz77_dedupe(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                       const int32_t *out_cap, int32_t *out_len, int32_t *status);
/*   jpk_cli_stages_encode_ex of n blocks: with JPK_CLI_DEDUPE the dedupe launches run in front of k_enc_wrap, and k_enc_wrap / k_enc_lpx take
 *   every block's length from its result (one host read for all blocks); out_len[b] = the host form's */
JPK_API int jpk_dev_blocks_cli_stages_encode_ex(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                                const int32_t *out_cap, int32_t *out_len, int32_t *status, uint32_t flags);
/*   jpk_filters_encode of n blocks of S1, the bytes and statuses of the host form, one launch (k_enc_filters: one workgroup per 64 KiB
 *   piece -- the piece and the 65 histograms in LDS, the costs, the choice, the transformed piece by destination).  A block whose out_cap
 *   is below in_len + 2 * ceil(in_len / 65536) reports JPK_E_CAPACITY alone, out_len[b] = 0, and nothing of it is written.  With
 *   JPK_CLI_FILTERS the _ex writer entries run the same kernel in the place of k_enc_wrap; no host read is added. */
JPK_API int jpk_dev_blocks_filters_encode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                          const int32_t *out_cap, int32_t *out_len, int32_t *status);
/* Jampack::Decompress (jampack.cpp:262-336) of an archive written by an unmodified `jampack c` (any -m / -f setting; the frames of
 * jpk_jam_cli_block_read, back to back): the frame walk of jpk_dev_jam_decompress, with an entropy-decoded size of at most
 * 1.05 x BlockSize + 4096 per frame (the reference's stage buffers, jampack.cpp:156), then per pass jpk_dev_blocks_decompress into
 * per-frame slots of a scratch buffer of ctx, the four batched pre-stage launches in the order of Jampack::Decomp() (Lz77, Lpx, Filters,
 * Lz77), one batched checksum compared with the header crcs, and one gather launch that packs the verified frames back to back into d_out.
 *   bad frame k (header, payload, a pre-stage stream, a raw size above BlockSize, crc): its status (JPK_E_CORRUPT), *bad_frame = k,
 *   *frames = k, *out_len = the raw bytes of frames 0..k-1, which are verified and in place.
 *   capacity: a frame's raw size is known only when it has been decoded.  The sum of the frames' BlockSize (*raw_bound of
 *   jpk_jam_cli_frames) always suffices.  When the frames of a pass do not fit the rest of out_cap: JPK_E_CAPACITY, *out_len = that sum,
 *   *frames = the frames of the earlier passes, which may be in place; nothing at or beyond d_out + out_cap is written.
 *   success: *frames = the frame count, *bad_frame = -1.  frames and bad_frame may be NULL.  1..14 trailing bytes are a bad frame.
 * Per-pass HBM: passes of at most 128 frames and 4 GiB of BlockSize; two slots of 1.05 x BlockSize + 4096 per frame (<= 9 GB) in the
 * scratch buffer, plus the batch decoder's arena (about 4 bytes per entropy-decoded byte of the pass). */
JPK_API int jpk_dev_jam_cli_decompress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len, int32_t *frames,
                                       int32_t *bad_frame);
/* host-buffer form through the calling thread's pooled context, staged one pass at a time; same contract (the arguments are checked
 * before a device is looked for) */
JPK_API int jpk_jam_cli_decompress(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frames, int32_t *bad_frame);
/* host walk of a stock-CLI archive in host memory with the checks of jpk_dev_jam_cli_decompress's walk: *frames = the frames in front of
 * the first bad one, *raw_bound = the sum of their BlockSize (an out_cap that always suffices), *bad_frame = its index (JPK_E_CORRUPT)
 * or -1 (JPK_OK).  No device call.  Pointers other than in may be NULL. */
JPK_API int jpk_jam_cli_frames(const uint8_t *in, int64_t in_len, int32_t *frames, int64_t *raw_bound, int32_t *bad_frame);

/* The archive an unmodified `jampack d` decodes (with any -t / -T): the frames of jpk_jam_cli_block_write over consecutive block_size
 * slices of the input, back to back.  The contract is that of jpk_jam_compress_bound / jpk_dev_jam_compress / jpk_jam_compress: the last
 * slice short, in_len == 0 gives an empty archive, block_size in [JPK_MIN_BLOCKSIZE, JPK_MAX_BLOCKSIZE], JPK_E_CAPACITY when the archive
 * does not fit out_cap (the bound always suffices), in_flight as jpk_dev_blocks_compress, arguments checked before a device is looked
 * for.  Per pass: one batched checksum of the raw slices, k_enc_wrap into slot A of every frame, k_enc_lpx from A into slot B (the BWT
 * inputs), jpk_dev_blocks_compress from the B slots into payload slots, one pack launch.
 * Per-pass HBM: passes of at most 128 frames and 4 GiB of input; per input byte about 1 byte of slot A, 1 of slot B and 1.25 of
 * payload slot (<= 14 GB) in the scratch buffer of ctx, on top of the workers' arenas of jpk_dev_blocks_compress. */
JPK_API int64_t jpk_jam_cli_compress_bound(int64_t in_len, int32_t block_size);
JPK_API int jpk_dev_jam_cli_compress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                     int32_t in_flight);
JPK_API int jpk_jam_cli_compress(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight);
/* The same with flags (JPK_CLI_DEDUPE): the frames of jpk_jam_cli_block_write_ex over the slices.  With the dedupe a pass runs the k_dd_*
 * launches from the raw slices into slot B, reads the pass's S1' lengths on the host -- jpk_dev_blocks_compress wants host lengths: ONE
 * synchronisation per pass, never one per frame -- and goes on with k_enc_wrap from B into A and k_enc_lpx from A into B at those lengths.
 * The dedupe's scratch (about 1.2 bytes per input byte of the pass) comes from ctx's arena.  With JPK_CLI_FILTERS k_enc_filters runs in the
 * place of k_enc_wrap, on the raw slices or on the dedupe's S1'; the lengths do not depend on its choices, so a pass gains no host read. */
JPK_API int jpk_dev_jam_cli_compress_ex(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap,
                                        int64_t *out_len, int32_t in_flight, uint32_t flags);
JPK_API int jpk_jam_cli_compress_ex(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight,
                                    uint32_t flags);

/* ---- staged frames: the dedupe and the filter choice in front of the BWT, without LPX and without the second LZ77 ------------------- */
/* A staged frame is the 15-byte header + jpk_block_compress(S2), with S1 and S2 the streams of those names in DESIGN 4.7 ("Writing",
 * "Dedupe", "Filters"): S1 = 04 80 | R, or jpk_lz77_dedupe(R) with JPK_CLI_DEDUPE; S2 = the 64 KiB pieces of S1 behind 00 00, or behind the
 * filter choice with JPK_CLI_FILTERS.  It is what Jampack::Comp() (jampack.cpp:29-44) writes when it runs Lz->Compress (-m0), Filter->Encode,
 * ForwardBwt and Entropy->Encode, i.e. jampack.cpp:36-41 without LocalModel->Encode and the second Lz->Compress (lines 38-39); the decoder is
 * Jampack::Decomp() (jampack.cpp:47-60) without lines 51-52.  Every stage stream is in the reference's format.  The crc is that of R.  The
 * header's BlockSize field carries JPK_JAM_STAGED (bit 30; JPK_MAX_BLOCKSIZE is below 2^30): the stock DecompReadBlock (jampack.cpp:150),
 * jpk_jam_frames, jpk_jam_cli_frames and the plain and stock-CLI decoders refuse such a header, so no decoder takes a staged frame for
 * another kind.  The flags (JPK_CLI_DEDUPE, JPK_CLI_FILTERS; accepted values 0, 1, 4, 5, anything else JPK_E_ARG) decide only whether the
 * writer's stages are stored or real: the decoder always runs Filters::Decode, then Lz77::Decompress.  A staged frame's raw size is in no
 * header, but it is a function of the tokens of its S1 alone: jpk_(dev_)jam_staged_index_create (below, with the range reads) index an
 * archive of plain and staged frames without expanding a frame, and jpk_dev_jam_read / jpk_jam_read read byte ranges through that index. */
#define JPK_JAM_STAGED (1 << 30)
/* one frame, host buffers (the stages on the host, the BWT and the entropy coder on the GPU): arguments and statuses as
 * jpk_jam_cli_block_write_ex / jpk_jam_cli_block_read; the reader takes staged frames only (any other header is JPK_E_CORRUPT) */
JPK_API int jpk_jam_staged_block_write(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags);
JPK_API int jpk_jam_staged_block_read(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t *consumed);
/* Jampack::Compress (jampack.cpp:186-260) with that Comp(): the frames of jpk_jam_staged_block_write over consecutive block_size slices,
 * back to back; the contract of jpk_dev_jam_cli_compress_ex.  Per pass: one batched checksum of the raw slices, the stage chain of the
 * stock-CLI writer stopped at S2 (k_enc_wrap or k_enc_filters into slot A, behind the k_dd_* launches and their one host read with the
 * dedupe), jpk_dev_blocks_compress from the A slots, one pack launch.  The bound counts jpk_cli_stages_bound bytes of BWT input per slice. */
JPK_API int64_t jpk_jam_staged_compress_bound(int64_t in_len, int32_t block_size);
JPK_API int jpk_dev_jam_staged_compress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap,
                                        int64_t *out_len, int32_t in_flight, uint32_t flags);
JPK_API int jpk_jam_staged_compress(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight,
                                    uint32_t flags);
/* host walk (DecompReadBlock's checks, jampack.cpp:140-163, with bit 30 allowed) of an archive that may hold plain and staged frames in
 * any order -- archives are concatenable by format: *frames = the frames in front of the first bad one, *raw_bound = the raw bytes of its
 * plain frames + the BlockSize of its staged ones (an out_cap that always suffices), *bad_frame as jpk_jam_cli_frames.  Bit 31, or bit 30
 * with a BlockSize out of range, is a bad frame.  No device call. */
JPK_API int jpk_jam_staged_frames(const uint8_t *in, int64_t in_len, int32_t *frames, int64_t *raw_bound, int32_t *bad_frame);
/* Jampack::Decompress (jampack.cpp:262-336) of such an archive, in passes of at most 128 frames and 4 GiB.  A plain frame decodes in its
 * place in d_out as in jpk_dev_jam_decompress.  A staged frame goes jpk_dev_blocks_decompress -> slot A, k_pre_filters -> slot B,
 * jpk_dev_blocks_lz77_expand_deep -> slot A (at most BlockSize bytes), one batched checksum against the header crcs, and one gather launch
 * into its place. Bad frames, capacity and success are reported as by jpk_dev_jam_cli_decompress: a stage that runs out of its slot (1.05 x
 * BlockSize + 4096) is JPK_E_CORRUPT; when the frames of a pass do not fit the rest of out_cap the call is JPK_E_CAPACITY with *out_len =
 * *raw_bound of jpk_jam_staged_frames and nothing of that pass written.  Arguments are checked before a device is looked for. */
JPK_API int jpk_dev_jam_staged_decompress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                          int32_t *frames, int32_t *bad_frame);
JPK_API int jpk_jam_staged_decompress(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frames, int32_t *bad_frame);
/* Lz77::Decompress(Buffer,Buffer) (lz77.hpp:46, lz77.cpp:678-714) of n blocks in two launches: bytes, lengths and statuses are those of
 * jpk_dev_blocks_lz77_decompress for every input, valid or not.  k_lzx_plan (one wave per block) writes a record per literal run and per
 * match, at most in_len / 64 + 4 per block in ctx's arena; k_lzx_copy fills aligned 16-byte words of the output from the records, a byte
 * of a match finding its literal in at most 8 hops.  A block that fails a check, needs more records or a longer chase goes through
 * k_pre_lz77 in one more launch.  The arguments are checked before a device is looked for.  No entry of the library calls it: it is far
 * faster than the serial kernel on stored and shallow streams and slower on the deep streams the dedupe writes of large blocks of real
 * sources ("Tried"); the staged reader runs jpk_dev_blocks_lz77_expand_deep, below, whose caps are made for those streams. */
JPK_API int jpk_dev_blocks_lz77_expand(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                       const int32_t *out_cap, int32_t *out_len, int32_t *status);
/* how many blocks of ctx's last jpk_dev_blocks_lz77_expand call took the two parallel launches and how many the serial kernel */
JPK_API int jpk_debug_lz77_expand_last(jpk_ctx *ctx, int32_t *parallel, int32_t *serial);
/* The same stage and the same contract -- bytes, lengths and statuses of jpk_dev_blocks_lz77_decompress for every input, valid or not,
 * d_out[b] at any alignment, the arguments checked before a device is looked for -- with the deep rule (lz_expand.hpp; DESIGN 4.6, "The
 * deep expander"): k_lzd_plan gives a block up behind the first token that leaves it with more than op / 128 + 4 records for op bytes
 * of output (a stream of the dedupe has at most op / 128 + 2; the record array is out_cap / 128 + 8 per block in ctx's arena), and
 * k_lzd_copy follows a byte through up to H hops and leaves a block as soon as one of its two serial words is set.  Two launches for the
 * batch, one host read of lengths and flags, one k_pre_lz77 launch for the blocks left to it and only then.  The last stage of the staged
 * reader (jpk_dev_jam_staged_decompress and what runs its pass: the _ix and host forms, the verify = 1 index, reads and salvage). */
JPK_API int jpk_dev_blocks_lz77_expand_deep(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                            const int32_t *out_cap, int32_t *out_len, int32_t *status);
/* how many blocks of the last deep call on ctx -- jpk_dev_blocks_lz77_expand_deep, or the last staged pass -- took the two parallel
 * launches and how many the serial kernel */
JPK_API int jpk_debug_lz77_deep_last(jpk_ctx *ctx, int32_t *parallel, int32_t *serial);
/* the constants of the deep rule: the hop cap H, the output bytes that pay for one record (128) and the records of slack (4) */
JPK_API int jpk_debug_lz77_deep_limits(int32_t *hops, int32_t *bytes_per_record, int32_t *slack);
/* The raw size of an Lz77 stream without its bytes: the token walk of Lz77::Decompress (lz77.cpp:678-714) with the checks of
 * jpk_lz77_decompress in their order and no copy.  Returns the status jpk_lz77_decompress gives the same stream at the same out_cap, for
 * every stream, valid or not (a token that does not parse, a negative offset, literals beyond the input or an offset beyond the output
 * so far JPK_E_CORRUPT; more than out_cap bytes JPK_E_CAPACITY), and *out_len = its *out_len on JPK_OK, 0 otherwise.  No device call,
 * no output buffer; in may be NULL when in_len == 0. */
JPK_API int jpk_lz77_size(const uint8_t *in, int32_t in_len, int32_t out_cap, int32_t *out_len);
/* the same for n blocks in HBM, one launch (k_lz77_sizes: one wave per block, one load per token, two result words per block and no
 * other store) and one read-back: out_len[b] and status[b] are those of jpk_dev_blocks_lz77_decompress on the same inputs and capacities,
 * the inputs stay as they are.  status may be NULL as there; the arguments are checked before a device is looked for. */
JPK_API int jpk_dev_blocks_lz77_sizes(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, const int32_t *out_cap, int32_t *out_len,
                                      int32_t *status);

/* ---- byte ranges of a .jam archive without decoding all of it ------------------------------------------------------------------- */
/* The frame table of one archive: per frame the payload offset and size, the header crc, BlockSize, the raw (decoded) size and the
 * 64-bit raw offset (the prefix sum of the raw sizes).  jpk_dev_jam_index_create walks an archive in HBM, jpk_jam_index_create one
 * in host memory (no device call); both apply the checks of jpk_dev_jam_decompress's walk / jpk_jam_frames.  An archive with a bad
 * frame gives JPK_OK and an index over the frames in front of the first bad one -- a damaged archive stays readable up to the damage --
 * with *bad_frame = its position (-1: none; may be NULL).  The index keeps no pointer to the archive, is immutable after creation and
 * may be used from several contexts and threads; jpk_jam_index_destroy releases it (NULL is allowed). */
typedef struct jpk_jam_index jpk_jam_index;
JPK_API int jpk_dev_jam_index_create(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame);
JPK_API int jpk_jam_index_create(const uint8_t *in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame);
/* *frames = the indexed frames, *raw_len = their raw bytes, *archive_len = the in_len the index was made from.  Pointers may be NULL. */
JPK_API int jpk_jam_index_info(const jpk_jam_index *index, int32_t *frames, int64_t *raw_len, int64_t *archive_len);
/* frame k: its raw offset and raw size, where its payload starts in the archive and the payload's size; JPK_E_ARG for k out of range */
JPK_API int jpk_jam_index_frame(const jpk_jam_index *index, int32_t k, int64_t *raw_off, int64_t *raw, int64_t *payload_off, int32_t *psize);
JPK_API void jpk_jam_index_destroy(jpk_jam_index *index);
/* The index of a stock-CLI archive (the frames jpk_dev_jam_cli_decompress reads).  Such a frame's raw size is in neither its header nor
 * its chunk headers: it is known only behind the frame's last stage, the second Lz77::Decompress.  So this index is made by DECODING the
 * archive once: the frame walk of jpk_dev_jam_cli_decompress, then its passes (at most 128 frames and 4 GiB of BlockSize, two slots of
 * 1.05 x BlockSize + 4096 per frame in the scratch buffer of ctx) -- the whole stage chain and the batched checksum against the header
 * crcs, but no output buffer and no gather.  Every frame in the index has been verified.  (Sizing the frames as "BlockSize each, the
 * last one the rest" from a known total is NOT sound: `cat a.jam b.jam` with frames of 500 KB, 1 MiB and 700 KB has a plausible frame
 * count and a middle frame that passes a per-frame check, and would be delivered at the wrong raw offset, silently.)
 * A bad frame is handled as by the plain index: JPK_OK, an index over the frames in front of the first bad one (bad header, payload,
 * pre-stage stream or crc, or a raw size above BlockSize), *bad_frame = its position (-1: none; may be NULL).  The arguments are
 * checked before a device is looked for, and in_len == 0 gives an empty index without a device.  jpk_jam_index_info / _frame / _destroy
 * work on it unchanged, and jpk_dev_jam_read / jpk_jam_read take it in the place of a plain index.  The host-buffer form stages the
 * archive one pass at a time through the calling thread's pooled context. */
#define JPK_JAM_INDEX_PLAIN 0
#define JPK_JAM_INDEX_CLI 1
JPK_API int jpk_dev_jam_cli_index_create(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame);
JPK_API int jpk_jam_cli_index_create(const uint8_t *in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame);
/* JPK_JAM_INDEX_PLAIN for an index of jpk_(dev_)jam_index_create, JPK_JAM_INDEX_CLI for one of the stock-CLI creators,
 * JPK_JAM_INDEX_STAGED (below) for one of the staged creators; JPK_E_ARG for NULL */
JPK_API int jpk_jam_index_kind(const jpk_jam_index *index);
/* jpk_dev_jam_cli_decompress that also hands back the index of the frames it delivered (the whole archive on JPK_OK, the frames in
 * front of the bad one on JPK_E_CORRUPT): a caller who decodes an archive once has its index for free.  index == NULL is allowed and
 * makes this the plain call; *index is NULL after JPK_E_CAPACITY and every other failure. */
JPK_API int jpk_dev_jam_cli_decompress_ix(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len, int32_t *frames,
                                          int32_t *bad_frame, jpk_jam_index **index);
/* The index of an archive of plain and staged frames in any order (the archives jpk_dev_jam_staged_decompress reads), kind
 * JPK_JAM_INDEX_STAGED.  The frame walk is that call's.  A plain frame keeps the raw size of the walk and is not decoded.  A staged
 * frame's raw size comes per pass (at most 128 frames and 4 GiB, a staged frame counted at its BlockSize; two slots of 1.05 x BlockSize
 * + 4096 per staged frame in the scratch buffer of ctx):
 *   verify == 0  jpk_dev_blocks_decompress -> slot A, k_pre_filters -> slot B, jpk_dev_blocks_lz77_sizes on B with out_cap = BlockSize:
 *                no expansion, no checksum, no gather.  A frame is bad when its header or payload is bad, a stage refuses its stream, or
 *                it declares more than BlockSize raw bytes.  THE FRAMES OF SUCH AN INDEX ARE NOT VERIFIED against their crcs -- as those
 *                of a plain index are not, whose sizes come from unverified headers too.  A read verifies every frame it touches.
 *   verify == 1  the whole stage list of jpk_dev_jam_staged_decompress into slot A and the batched checksum against the header crcs, as
 *                jpk_dev_jam_cli_index_create does for its kind: every STAGED frame in the index has been verified.
 *   any other value is JPK_E_ARG.
 * A bad frame is handled as by the other creators: JPK_OK, an index over the frames in front of the first bad one, *bad_frame = its
 * position (-1: none; may be NULL); a stage's JPK_E_CAPACITY counts as JPK_E_CORRUPT.  The arguments are checked before a device is
 * looked for, and in_len == 0 gives an empty index of this kind without a device.  The host-buffer form walks the archive on the host
 * and makes NO device call for an archive without a staged frame (such an index can be made on a machine without a GPU); otherwise it
 * stages the archive one pass at a time through the calling thread's pooled context.  jpk_jam_index_create and the stock-CLI creators
 * go on refusing staged frames.  jpk_jam_index_info / _frame / _kind / _destroy work on this kind unchanged. */
#define JPK_JAM_INDEX_STAGED 2
JPK_API int jpk_dev_jam_staged_index_create(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t verify, jpk_jam_index **index, int32_t *bad_frame);
JPK_API int jpk_jam_staged_index_create(const uint8_t *in, int64_t in_len, int32_t verify, jpk_jam_index **index, int32_t *bad_frame);
/* frame k of an index: JPK_JAM_INDEX_PLAIN or JPK_JAM_INDEX_STAGED for a frame of a JPK_JAM_INDEX_STAGED index, the index's own kind
 * for the other two kinds; JPK_E_ARG for NULL or k out of range */
JPK_API int jpk_jam_index_frame_kind(const jpk_jam_index *index, int32_t k);
/* jpk_dev_jam_staged_decompress that also hands back the index (kind JPK_JAM_INDEX_STAGED) of the frames it delivered (the whole
 * archive on JPK_OK, the frames in front of the bad one on JPK_E_CORRUPT): a caller who decodes an archive once has its index for free.
 * index == NULL is allowed and makes this the plain call; *index is NULL after JPK_E_CAPACITY and every other failure. */
JPK_API int jpk_dev_jam_staged_decompress_ix(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                             int32_t *frames, int32_t *bad_frame, jpk_jam_index **index);
/* n ranges in raw coordinates, [off[r], off[r] + len[r]) delivered at d_out[r] (a device pointer of any alignment; the buffers must
 * not overlap).  in_len must be the index's archive length and every range must satisfy 0 <= off, 0 <= len, off + len <= raw_len:
 * JPK_E_ARG otherwise, before any device work, nothing written.  len == 0 is legal anywhere in [0, raw_len] and touches no frame.
 * Ranges may be unsorted, overlapping or identical.
 * Cost: the crc of a frame covers the whole frame, so every frame a range touches is decoded whole -- ONCE per call, however many
 * ranges want it -- through jpk_dev_blocks_decompress, in passes of at most 128 touched frames and 4 GiB of raw bytes.  A frame that
 * lies wholly inside a range is decoded straight into that range's buffer (as jpk_dev_jam_decompress decodes in place; further ranges
 * copy from there), every other one into a padded slot of a scratch buffer of ctx (the raw bytes of the pass's partial frames).  Per
 * pass: the batch decode, one batched checksum of the touched frames against their header crcs, one gather launch for all pieces of
 * verified frames.  Nothing outside [d_out[r], d_out[r] + len[r]) is written; a frame no range touches is neither decoded nor checked.
 * status[r] = JPK_OK, or the status of the lowest-numbered frame of range r that failed to decode or failed its crc (JPK_E_CORRUPT);
 * ranges whose frames are all good are delivered whatever happens to the others, the buffer of a failed range is unspecified.
 * *bad_frame = the lowest failing frame any range touches, or -1 (may be NULL).  Returns as jpk_dev_blocks_decompress: with a
 * status array JPK_OK once the arguments were accepted, with status == NULL the first failing range's status.
 * With an index of kind JPK_JAM_INDEX_CLI the contract is the same, word for word, and the decoder of a pass is the stage chain of
 * jpk_dev_jam_cli_decompress on the touched frames alone: passes of at most 128 touched frames and 4 GiB of BlockSize (the slots are
 * sized by BlockSize, not by raw size), two slots of 1.05 x BlockSize + 4096 per touched frame in the scratch buffer of ctx.  A frame
 * wholly inside a range has its LAST stage, the second Lz77::Decompress, write straight into that range's buffer; every other frame ends
 * in its slot A.  Unlike the whole-archive call the read does not stop at the first bad frame: after every stage the jobs are compacted
 * to the frames that passed it, a stage that runs out of its slot is JPK_E_CORRUPT (never JPK_E_CAPACITY), and the last stage's
 * capacity is the indexed raw size exactly -- a frame that decodes to another size belongs to an archive that is not the indexed one and
 * is JPK_E_CORRUPT.  The crc a frame must meet is the one in its header in the archive being read (four bytes per touched frame are
 * read for it), so a header damaged after indexing fails its frame too.
 * With an index of kind JPK_JAM_INDEX_STAGED the contract is the same again, and a pass of touched frames (a staged one counted at its
 * BlockSize, a plain one at its raw size) holds two groups.  Its plain frames go through jpk_dev_blocks_decompress exactly as under a
 * plain index: in place or in a slot of their raw size, against the indexed crc.  Its staged frames go through the stage list of
 * jpk_dev_jam_staged_decompress as the frames of a stock-CLI index go through theirs: two slots of 1.05 x BlockSize + 4096 per frame,
 * compacted after every stage, the last stage into the range that holds the frame whole or into slot A at exactly the indexed raw size
 * (any other size is JPK_E_CORRUPT), against the crc in the header of the archive being read.  One gather launch per pass delivers the
 * pieces of both groups.  Whether the index was made with verify 0 or 1, every touched frame is verified by the read. */
JPK_API int jpk_dev_jam_read(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len,
                             uint8_t *const *d_out, int32_t *status, int32_t *bad_frame);
/* host-buffer form through the calling thread's pooled context: only the payloads of the touched frames are staged to the device,
 * pass by pass, and only the ranges travel back; same contract (the arguments are checked before a device is looked for) */
JPK_API int jpk_jam_read(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len, uint8_t *const *out,
                         int32_t *status, int32_t *bad_frame);

/* ---- damaged archives: an index past the damage, and everything recoverable ("Damaged archives") ----
 * The creators above stop at the first bad frame, and so do the whole-archive decoders; their contracts stay as they are.  These
 * entries go on behind the damage.  The rule (jampack_amd/csrc/jam_resync.hpp, one source for both forms): a frame is STRUCTURALLY VALID
 * at offset o when its header is plausible -- "JAM", BlockSize in [JPK_MIN_BLOCKSIZE, JPK_MAX_BLOCKSIZE] (kind JPK_JAM_INDEX_STAGED:
 * JPK_JAM_STAGED allowed), 0 <= payload size <= JPK_MAX_BLOCKSIZE, header and payload inside the archive --, jpk_ans_decoded_size
 * accepts its payload and the size that declares fits its BlockSize: the checks of the frame walks, no more and no fewer.  From g = 0:
 * o = the smallest offset >= g at which a structurally valid frame starts (none: in_len); the bytes [g, o) in front of it, if any, are
 * a gap; the frame at o is taken and g moves behind its payload.  Frames and gaps tile [0, in_len) in order and without overlap; on an
 * undamaged archive the result is the frame table of the creators above, no gap, and for an archive in HBM no launch beyond theirs.
 * The index is a pure function of the archive bytes, kind and verify.  A header-shaped decoy inside a lost payload is taken only if
 * its chunk headers walk too; one that does is a frame of the index, and a read of it fails its crc (or, rarely, its decode) -- kinds
 * 0 and 2; with kind 1 such a decoy is decoded like every candidate, fails, and is a JPK_JAM_GAP_STAGE gap, never a frame.
 * A gap is {archive_off, archive_len, frame = the number of recovered frames in front of it, why}:
 *   JPK_JAM_GAP_NOFRAME  no structurally valid frame starts in these archive bytes
 *   JPK_JAM_GAP_STAGE    (kind JPK_JAM_INDEX_STAGED) a structurally valid staged frame whose stages -- or, verify = 1, crc -- refuse it;
 *                        (kind JPK_JAM_INDEX_CLI) a structurally valid frame that a stage refuses, that decodes to more than its
 *                        BlockSize or that fails its crc: its raw size is unknown, so it cannot be a frame of the index; the gap is
 *                        its span, header + payload
 * kind JPK_JAM_INDEX_PLAIN: verify must be 0; frames are unverified as in a plain index; the host form makes no device call.
 * kind JPK_JAM_INDEX_STAGED: staged frames are sized pass by pass as by jpk_dev_jam_staged_index_create (verify as there); a pass holds
 * frames that lie back to back; the host form looks for a device only when the walk found a staged frame.
 * kind JPK_JAM_INDEX_CLI: verify must be 1 (verify = 0: JPK_E_ARG) -- every frame of a stock-CLI index has been decoded and has met its
 * crc, as with jpk_dev_jam_cli_index_create.  Structurally valid means what the stock-CLI frame walk means: no staged bit, and a
 * declared entropy-decoded size of at most 1.05 x BlockSize + 4096.  Every structurally valid frame then goes through the whole
 * stock-CLI stage chain and the crc, pass by pass, each with a status of its own; a pass holds frames that lie back to back, at most
 * JPK_JAM_PASS_FRAMES of them and 4 GiB of BlockSize; there is no output buffer.  f.raw comes from that decode.  The walk goes on behind
 * a frame that fails.  The host form walks on the host, looks for a device only when the walk found a frame, and stages pass by pass.
 * The price is one full stage chain per structurally valid candidate, decoys included.
 * The index has the requested kind, no bad frame (jpk_jam_index_info and the readers see a plain table), raw offsets that count the
 * recovered frames only -- a gap holds no raw bytes --, and jpk_jam_index_info / _frame / _kind / _frame_kind / _destroy,
 * jpk_dev_jam_read and jpk_jam_read take it unchanged.  *gaps (may be NULL) = the number of gaps.  Arguments are checked before a
 * device is looked for; in_len == 0 gives an empty index.  Cost on hostile input: every archive byte is scanned once per search that
 * reaches it, every plausible header costs one chunk-header walk of its payload (DESIGN 4.6 has the bound). */
#define JPK_JAM_GAP_NOFRAME 0   /* no structurally valid frame starts in these archive bytes */
#define JPK_JAM_GAP_STAGE   1   /* a structurally valid staged frame (kind 2) whose stages (or, verify = 1, crc) refuse it, or frame of the
                                 * stock CLI (kind 1) that fails its stage chain or its crc: its raw size is unknown */
JPK_API int jpk_dev_jam_index_recover(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t kind, int32_t verify, jpk_jam_index **index, int32_t *gaps);
JPK_API int jpk_jam_index_recover(const uint8_t *in, int64_t in_len, int32_t kind, int32_t verify, jpk_jam_index **index, int32_t *gaps);
JPK_API int jpk_jam_index_gaps(const jpk_jam_index *index);   /* count; 0 for an index of the existing creators; JPK_E_ARG for NULL */
/* gap g of an index (JPK_E_ARG outside [0, jpk_jam_index_gaps)); every output pointer may be NULL */
JPK_API int jpk_jam_index_gap(const jpk_jam_index *index, int32_t g, int64_t *archive_off, int64_t *archive_len, int32_t *frame, int32_t *why);
/* Everything an index can deliver of its archive, in one call: frame k at d_out + its raw offset, *out_len = the index's raw_len.  Takes
 * any index -- recovered or not, any kind.  A frame that fails its decode or its crc gets frame_status[k] = JPK_E_CORRUPT and its place
 * filled with zeros; *failed = the number of such frames; the call returns JPK_OK whenever it ran, however many frames failed.  A frame of
 * 0 raw bytes is reported JPK_OK and is not verified.  frame_status (one entry per frame of the index) and failed may be NULL.
 * out_cap < raw_len: JPK_E_CAPACITY, *out_len = raw_len, nothing written.  in_len must be the index's archive length (JPK_E_ARG).
 * It is one range per frame handed to the reader of jpk_dev_jam_read -- its passes, its decoders, every frame in place --, then a memset
 * per failed frame.  Nothing outside [d_out, d_out + raw_len) is written. */
JPK_API int jpk_dev_jam_salvage(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                int32_t *frame_status, int32_t *failed);
/* host-buffer form through the calling thread's pooled context (the arguments and the capacity are checked before a device is looked for) */
JPK_API int jpk_jam_salvage(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frame_status,
                            int32_t *failed);
/* The archive that holds exactly the kept frames of an index, back to back: for every frame k of the index with frame_status == NULL or
 * frame_status[k] == JPK_OK, in order, its 15 header bytes (at payload_off - 15 of the archive) and its payload, copied unchanged.  *out_len
 * = the bytes written, *frames (may be NULL) = the frames kept.  in_len must be the index's archive length (JPK_E_ARG).  out_cap too
 * small: JPK_E_CAPACITY, *out_len = the size needed, nothing written.  Nothing outside [d_in, d_in + in_len) is read and nothing outside
 * [d_out, d_out + *out_len) is written; d_in and d_out at any alignment; the buffers must not overlap.  No frame is decoded: pass the
 * frame_status of a salvage to drop frames that fail their decode or crc.  Takes any index, recovered or not, of any kind; the result
 * of a recovered one is an archive that the stock decoder and every whole-archive decoder here read to its end.  One k_jam_gather
 * launch, a piece per kept frame; an index without a kept frame gives *out_len = 0 and no launch.  Arguments and capacity are checked
 * before a device is looked for. */
JPK_API int jpk_dev_jam_repair(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, const int32_t *frame_status,
                               uint8_t *d_out, int64_t out_cap, int64_t *out_len, int32_t *frames);
JPK_API int jpk_jam_repair(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, const int32_t *frame_status, uint8_t *out,
                           int64_t out_cap, int64_t *out_len, int32_t *frames);   /* host memory: memcpy, no device call */
/* ---- updating an archive: byte ranges replaced, only the touched frames encoded again ("Updating an archive") ----
 * The input is an index of any kind, recovered or not, and its archive (in_len must be the index's archive length).  The n writes
 * (off[r], len[r], src[r]) are in raw coordinates; a tail of tail_len bytes (may be 0) is appended.  The result is the archive whose decode
 * is the old raw bytes with every [off[r], off[r] + len[r]) replaced by the len[r] bytes at src[r], followed by the tail.
 *   writes      every one inside [0, raw_len]; those with len > 0 pairwise disjoint (end to end is allowed), in any order; len == 0 is
 *               legal anywhere and touches nothing.  An overlap, a write outside the range, a wrong in_len, a NULL pointer that is
 *               needed, flags other than 0, 1, 4, 5 (checked always), tail_len < 0 or a tail_block_size outside [JPK_MIN_BLOCKSIZE,
 *               JPK_MAX_BLOCKSIZE] with a tail: JPK_E_ARG before any device is looked for, and nothing is written, the results included
 *   untouched   a frame no write touches is copied unchanged, header and payload, neither decoded nor verified (as jpk_dev_jam_repair);
 *               the gaps of a recovered index are dropped as repair drops them; a frame of 0 raw bytes is always kept
 *   rewritten   a touched frame keeps its raw size, its BlockSize field and its kind: a plain frame stays plain (also under an index of
 *               kind 2) and is what jpk_jam_block_write gives for its new raw bytes and its BlockSize; a staged frame what
 *               jpk_jam_staged_block_write gives with `flags`; a frame of an index of kind 1 what jpk_jam_cli_block_write_ex gives with
 *               `flags` -- byte for byte.  A frame whose every byte the union of the writes covers is not decoded: its old content does
 *               not matter, so a frame that fails its crc can be replaced this way.  A partly covered frame is decoded and verified
 *               through the passes of jpk_dev_jam_read; if one fails its decode or its crc the call returns JPK_E_CORRUPT, *bad_frame
 *               (may be NULL) = the lowest such frame of the index, *new_index = NULL, and what the output buffer holds is unspecified
 *   tail        new frames behind the last one: tail_block_size slices, the last one short, of the index's kind (kind 2: staged frames
 *               with `flags`) -- the bytes of the matching jpk_dev_jam_*compress call over the tail.  tail_len == 0 ignores
 *               tail_block_size.  An empty index with a tail makes the call a writer that returns its index
 *   new index   *new_index (the caller destroys it) has the index's kind, no gap and no bad frame, and equals field by field what the
 *               matching creator makes of the output.  It is built from what the call knows -- offsets, payload sizes, crcs, BlockSize
 *               fields, raw sizes, staged bits --: the output is not walked, and a rewritten frame is WRITTEN by this call, not decoded
 *               back, so its entry vouches for the writer, not for a read-back.  *rewritten (may be NULL) = the rewritten frames
 *   capacity    jpk_jam_update_bound = the spans of the kept frames + the frame bound of every rewritten frame (15 + the payload slot of
 *               its raw size, of its pre-stage bound for a chained frame) + the kind's compress bound of the tail; it always suffices,
 *               and is JPK_E_ARG for arguments the entries refuse.  A smaller out_cap that turns out too small: JPK_E_CAPACITY, *out_len
 *               = the bound (earlier stretches of the output may have been written; one that cannot even hold the kept frames and
 *               the new headers is refused before anything is written)
 * The archive, the sources, the tail and the output must not overlap; each at any alignment.  Nothing outside [d_in, d_in + in_len) and
 * [d_src[r], d_src[r] + len[r]) is read of them and nothing outside [d_out, d_out + *out_len) is written.  Per pass of at most 128
 * rewritten frames (and 4 GiB of their weight, a chained frame its BlockSize): the reader for the partly covered ones, one k_jam_gather
 * launch for the sources, the compress pass, one k_jam_splice launch for the stretch of the output the pass ends. */
JPK_API int64_t jpk_jam_update_bound(const jpk_jam_index *index, int32_t n, const int64_t *off, const int64_t *len, int64_t tail_len, int32_t tail_block_size);
JPK_API int jpk_dev_jam_update(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len,
                               const uint8_t *const *d_src, const uint8_t *d_tail, int64_t tail_len, int32_t tail_block_size, uint32_t flags, int32_t in_flight,
                               uint8_t *d_out, int64_t out_cap, int64_t *out_len, jpk_jam_index **new_index, int32_t *rewritten, int32_t *bad_frame);
/* host-buffer form through the calling thread's pooled context: only the payloads of the partly covered frames, the pieces of the sources
 * and the tail travel to the device, only the new payloads travel back, and the kept frames are copied with memcpy.  Arguments are
 * checked before a device is looked for; a call with no rewritten frame and no tail makes no device call, and its output is
 * jpk_jam_repair's */
JPK_API int jpk_jam_update(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len,
                           const uint8_t *const *src, const uint8_t *tail, int64_t tail_len, int32_t tail_block_size, uint32_t flags, int32_t in_flight, uint8_t *out,
                           int64_t out_cap, int64_t *out_len, jpk_jam_index **new_index, int32_t *rewritten, int32_t *bad_frame);
/* probe: the offsets of the first max_cands (1..65536) plausible frame headers that start in [start, start + window) of d_in[0..in_len),
 * ascending, from one run of k_jam_scan_count / the prefix scan / k_jam_scan_emit; window <= 2^30; stateless, reads only.  offsets holds
 * max_cands entries */
JPK_API int jpk_debug_jam_scan(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int64_t start, int64_t window, int32_t staged_ok, int32_t max_cands,
                               int64_t *offsets, int32_t *count);
/* test hook (JPK_DEBUG_HOOKS=1 only, JPK_E_ARG otherwise): the window (bytes) and the candidates per round of the search of both recover
 * entries in this process; 0, 0 restores the defaults (256 MiB, 4096).  The index does not depend on either. */
JPK_API int jpk_debug_jam_recover_limits(int64_t window, int32_t max_cands);

/* ---- kernel-level probes used by tests/ and bench.py (device buffers) ------------------------------------ */
/* Comparator for BASELINE config 3 ("120-way parallel LF-map"): the reference's own GPU kernel shape -- 120 threads, one per
 * stored index, p = Map[p-1] (CUDAInverse<<<40,3>>>, bwt.cpp:8-19, 176-183, 226-229) -- on the same Map.  Same bytes as
 * jpk_dev_bwt_inverse; *chase_ms = device time of the chase kernel alone.  A measured baseline, never a product path. */
JPK_API int jpk_dev_bwt_inverse_chains120(jpk_ctx *ctx, const uint8_t *d_in, int32_t in_len_with_trailer, uint8_t *d_out, int32_t out_cap,
                                  int32_t *out_len, float *chase_ms);
/* suffix array of d_t[0..n) into d_sa (int32[n]) -- the divsufsort() replacement, divsufsort.cpp:1721 */
JPK_API int jpk_dev_suffix_array(jpk_ctx *ctx, const uint8_t *d_t, int32_t n, int32_t *d_sa);
/* stable LSD radix sort of (u64 key, u32 value) pairs on bits [bit_lo, bit_hi): 0 <= bit_lo <= bit_hi <= 64, any width -- the key bits outside the
 * range decide nothing (pairs that agree inside it keep their order) and travel with their pair; bit_lo == bit_hi leaves the arrays as they are */
JPK_API int jpk_dev_sort_pairs_u64(jpk_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, int32_t n, int32_t bit_lo, int32_t bit_hi);
/* exclusive prefix sum of uint32[n] in place; returns the total in *total */
JPK_API int jpk_dev_exclusive_scan_u32(jpk_ctx *ctx, uint32_t *d_data, int32_t n, uint32_t *total);
/* entropy sub-stages of one chunk: rank array -> RLE0 symbols; symbols -> packed (low | freq<<16) pairs.
 * jpk_dev_model_pairs takes the symbols of ONE chunk: rlen > JPK_ANS_CHUNK is JPK_E_ARG, refused with the other arguments before anything is allocated or launched (beyond a chunk a
 * class can outrun the QuasiModel's rebuild schedule as the encoder tabulates it).  PRECONDITION: every symbol is <= 256, as RLE0
 * produces them; the probe does not check it, and the kernels index their tables by the symbol. */
JPK_API int jpk_dev_rle_encode(jpk_ctx *ctx, const uint8_t *d_ranks, int32_t len, uint16_t *d_rle, int32_t *rlen);
JPK_API int jpk_dev_model_pairs(jpk_ctx *ctx, const uint16_t *d_rle, int32_t rlen, uint32_t *d_pairs);

/* ---- host-logic probes (no device call; tests/test_abi_and_host.py) ----------------------------------------------- */
/* The encoder cuts one block's chunks into 1..4 graded launch groups by the number of blocks that are in their forward BWT or
 * entropy encode ON THE SAME DEVICE at that moment (jampack.cpp:215 runs one block per OpenMP thread; with jpk_init over eight
 * GPUs every block is alone on its device).  jpk_debug_compress_inflight: delta > 0 registers a block on `device` and returns the
 * count including it, delta < 0 removes one and returns what is left, delta == 0 reads.  jpk_debug_enc_groups: the launch groups
 * a block of `nch` chunks arriving on `device` now would get. */
JPK_API int jpk_debug_compress_inflight(int device, int delta);
/* HBM arena bytes stage 0 (forward BWT) / 1 (rANS encode, text-like data: 0.55 RLE0 symbols per byte) / 2 (inverse BWT) /
 * 3 (rANS decode, bound) plans for one block of block_bytes; jpk_ctx_reserve takes their maximum.  Stage 4: rANS encode of the
 * densest data (every byte a symbol) -- what a context's arena grows to the first time such a block arrives. */
JPK_API int64_t jpk_debug_arena_bytes(int64_t block_bytes, int stage);
/* jpk_ans_decode calls that arrive from different threads at about the same time are merged into one batched pass on their
 * device (ans.cpp:254-264 decodes Threads chunks at a time; jampack.cpp:313 calls Decomp() from Threads OpenMP threads): the
 * number of requests the most recent pass on `device` carried (1: a lone caller, single-block path).  JPK_COMBINE_US=<grace
 * in microseconds, default 300; negative: never merge> in the environment. */
JPK_API int jpk_debug_combiner_last_batch(int device);
JPK_API int jpk_debug_enc_groups(int device, int32_t nch);
/* The block loops of Jampack::Compress / Jampack::Decompress (jampack.cpp:205-224, 286-317) over the GPUs of one node, natively:
 * block b runs on the (b mod G)-th device of `device_mask` (bit d = device d, 0 = every visible gfx950 device; one worker thread per
 * device; `in[b]` are HOST buffers, copied into a per-device slab the library keeps between calls), THROUGH THE LIBRARY'S BATCH ENTRY
 * on that device -- jpk_dev_blocks_compress with `in_flight` blocks in flight (<= 0: its default, 10) and small blocks in groups, or
 * jpk_dev_blocks_decompress (one pass over the chunks of all the device's blocks) -- and the results are gathered in block order into
 * `d_out`, a buffer of out_cap bytes on the FIRST device of the mask: block b occupies [out_off[b], out_off[b + 1]) (out_off has
 * nblocks + 1 entries).  Decompress: in_len[b] = compressed bytes, raw_len[b] = the block's decompressed size (the frame header's
 * BlockSize or what jpk_ans_decoded_size reports minus the trailer); the gather moves raw_len[b] bytes per block.
 * The gather is one ncclSend / ncclRecv pair of exactly the block's bytes per block of a non-root device, grouped, over a
 * single-process RCCL communicator (ncclCommInitAll) that the library loads at first use and keeps until jpk_shutdown; the root's
 * own blocks are device-to-device copies (JPK_MULTI_FORCE_RCCL=1: through RCCL as well).  Compress: a device's inputs travel on a
 * stream of their own, block by block, while the blocks before them are being compressed (jampack.cpp:205-224 overlaps its reads the
 * same way).
 * STATUS AND RESULTS: status[b] (nullable) receives every block's own status; a block that was never reached (its device failed
 * early) reports an error, never JPK_OK.  Every block whose status is JPK_OK IS GATHERED, also when other blocks failed (a corrupt
 * frame among healthy ones): its bytes are at [out_off[b], out_off[b + 1]), a failed block's range is empty, and the call returns the
 * first failed block's status.  When the gather itself cannot run (JPK_E_CAPACITY: d_out too small for the blocks that are done;
 * RCCL missing) nothing is in d_out, EVERY status is an error and every range is empty.
 * ONE CALL AT A TIME PER DEVICE: a call holds the mutexes of the devices of its mask; calls on disjoint device sets run side by side,
 * calls that share a device (and jpk_shutdown) queue.  The caller's current HIP device is restored on return.
 * jpk_debug_multi_plan: the ownership rule alone, for `ndev_visible` devices (no device call).  jpk_debug_multi_lock_probe: takes the
 * device mutexes of `device_mask` for hold_ms milliseconds (no device call; returns the number of mutexes). */
JPK_API int jpk_blocks_compress_multi(uint64_t device_mask, int32_t nblocks, const uint8_t *const *in, const int32_t *in_len, uint8_t *d_out, int64_t out_cap,
                                      int64_t *out_off, int32_t *status);
JPK_API int jpk_blocks_compress_multi_ex(uint64_t device_mask, int32_t nblocks, const uint8_t *const *in, const int32_t *in_len, uint8_t *d_out, int64_t out_cap,
                                         int64_t *out_off, int32_t *status, int32_t in_flight);
JPK_API int jpk_blocks_decompress_multi(uint64_t device_mask, int32_t nblocks, const uint8_t *const *in, const int32_t *in_len, const int32_t *raw_len, uint8_t *d_out,
                                        int64_t out_cap, int64_t *out_off, int32_t *status);
JPK_API int jpk_debug_multi_plan(uint64_t device_mask, int32_t ndev_visible, int32_t nblocks, int32_t *owner);
JPK_API int jpk_debug_multi_lock_probe(uint64_t device_mask, int32_t hold_ms);
/* host-logic probe: the work list jpk_dev_blocks_compress forms for these block lengths (groups of small blocks, large blocks alone):
 * task t covers blocks [first[t], first[t] + count[t]); returns the number of tasks.  No device call. */
JPK_API int jpk_debug_group_plan(int32_t nblocks, const int32_t *in_len, int32_t *first, int32_t *count);
/* host-logic probe: the groups the batched inverse BWT of jpk_dev_blocks_decompress cuts nblocks consecutive blocks of these output
 * capacities into: as many blocks per group as fit budget_bytes of scratch (0 = the production 8 GiB) and 65 535 jobs, a block beyond the
 * budget alone; group g ends in front of block group_end[g] (nblocks entries of room).  Returns the number of groups.  No device call. */
JPK_API int jpk_debug_inv_batch_plan(int32_t nblocks, const int32_t *out_cap, int64_t budget_bytes, int32_t *group_end);
/* host-logic probe: which rounds of a suffix sort the host makes PAIR rounds (bwt_fwd.hip PairSchedule: behind a doubling round that left >= 90 % of
 * its list, two doubling rounds apart, twice as far behind a pair round that left most of its list; JPK_PAIR_* override), given what the host
 * knows -- list[r] = the unresolved suffixes round r started with (list[0] = n; 0 = the sort had ended).  is_pair[r] = 1 for pair rounds; returns
 * their number.  No device call. */
JPK_API int jpk_debug_pair_schedule(int64_t n, int32_t nrounds, const uint32_t *list, int32_t runs_heavy, int32_t *is_pair);
/* Hooks that CHANGE live state work only in a process with JPK_DEBUG_HOOKS=1 in its environment (JPK_E_ARG otherwise):
 * jpk_debug_compress_inflight with delta != 0, and jpk_debug_combiner_fail_next(n): the next n merged decode passes fail as a
 * whole before they run -- every merged request must then come back through its own thread's single-block path. */
JPK_API int jpk_debug_combiner_fail_next(int n);
/* (JPK_DEBUG_HOOKS=1 only) the next n groups of jpk_dev_blocks_compress fail as a whole before they run: their blocks must come back
 * through the single-block path with the same bytes */
JPK_API int jpk_debug_group_fail_next(int n);

#ifdef __cplusplus
}
#endif
#endif /* JAMPACK_ABI_H */
