// abi_host.hip -- the host-buffer (drop-in) entry points of the C ABI: PCIe staging around the device entries, the decode
// combiner, and the single .jam frames (plain, stock-CLI and staged) on host buffers.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "abi.hpp"
#include "jam_resync.hpp"

namespace {
// the arguments of a host-buffer stage entry
bool staged_args_ok(const uint8_t *in, int32_t in_len, const uint8_t *out, int32_t out_cap, const int32_t *out_len)
{
    return out && out_len && in_len >= 0 && out_cap >= 0 && (in_len == 0 || in);
}
// ... and its tail: the n result bytes at d_res to the caller's buffer, behind everything on the context's stream
int staged_finish(jpk_ctx *ctx, const uint8_t *d_res, int32_t n, uint8_t *out, int32_t *out_len)
{
    if (n > 0) JPK_HIP(hipMemcpyAsync(out, d_res, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    *out_len = n;
    return JPK_OK;
}

// H2D -> device entry fn(ctx, d_in, in_len, d_out, out_cap, &out_len) -> D2H.  prefill_out: copy the caller's out bytes to the device
// first (used where the reference leaves part of the output untouched).
template <class Fn> int staged(Fn fn, const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, bool prefill_out)
{
    if (!staged_args_ok(in, in_len, out, out_cap, out_len)) return JPK_E_ARG;
    jpk_ctx *ctx;
    JPK_TRY(jpk_host_enter(&ctx, (size_t)in_len + 64));
    // the fused entry points use stage_out as their intermediate, so the host-visible result gets its own buffer
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_res, &ctx->stage_res_cap, (size_t)out_cap + 64));
    uint8_t *d_res = ctx->stage_res;
    if (in_len) JPK_HIP(hipMemcpyAsync(ctx->stage_in, in, (size_t)in_len, hipMemcpyHostToDevice, ctx->stream));
    if (prefill_out && out_cap) JPK_HIP(hipMemcpyAsync(d_res, out, (size_t)out_cap, hipMemcpyHostToDevice, ctx->stream));
    int32_t n = 0;
    JPK_TRY(fn(ctx, ctx->stage_in, in_len, d_res, out_cap, &n));
    return staged_finish(ctx, d_res, n, out, out_len);
}
}  // namespace

extern "C" int jpk_bwt_forward(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    if (in_len >= 0 && (int64_t)in_len + JPK_TRAILER_BYTES > (int64_t)out_cap) return JPK_E_CAPACITY;
    // a block shorter than 120 bytes leaves the trailer untouched (bwt.cpp:35): round-trip the caller's bytes
    const bool keep = in_len >= 0 && in_len < JPK_BWT_UNITS;
    return staged(jpk_dev_bwt_forward, in, in_len, out, keep ? in_len + JPK_TRAILER_BYTES : out_cap, out_len, keep);
}

extern "C" int jpk_bwt_inverse(const uint8_t *in, int32_t in_len_with_trailer, uint8_t *out, int32_t out_cap, int32_t *out_len,
                               int32_t threads, int32_t use_gpu)
{
    (void)threads; (void)use_gpu;      // Options.Threads / Options.Gpu do not change the bytes (bwt.cpp:92-132)
    return staged(jpk_dev_bwt_inverse, in, in_len_with_trailer, out, out_cap, out_len, false);
}

extern "C" int jpk_ans_encode(uint8_t *in_clobbered, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    return staged(jpk_dev_ans_encode, in_clobbered, in_len, out, out_cap, out_len, false);
}

// ---- decode combiner: concurrent host-buffer Ans::Decode calls share one batched grid ---------------------------------------
// The reference decodes `Threads` chunks at a time inside one Ans::Decode call (ans.cpp:254-264) and its multi-block loop calls
// Decomp() from `Threads` OpenMP threads at once (jampack.cpp:313).  On the GPU one block is 65 single-wave chains on 1024
// SIMDs, so the rate lives in the batch (jpk_ans_decode_batch: ONE grid per serial kernel over the chunks of all blocks).  A
// plain drop-in caller never sees the batch ABI; instead, calls that arrive from different threads within a short window are
// merged here: every thread stages its own input (its context, its stream), the first one to arrive leads -- it waits until
// nobody is on the way in any more (threads between entry and submission are counted) plus a grace period that applies only
// when the process has shown concurrency before, decodes all requests in one pass on a combiner context of the device, and
// wakes the others, which copy their own results back.  A lone caller runs exactly the single-block path at once; a thread
// that arrives while a batch is already on the GPU leads a new batch immediately (nobody ever waits for a running batch).
namespace {
struct DecReq {
    const uint8_t *d_in; int32_t in_len; uint8_t *d_out; int32_t out_cap;
    hipEvent_t staged;              // the request's input has reached the device
    int32_t out_len = 0, status = JPK_OK;
    bool done = false;
    bool alone = false;             // the merged pass did not take place for this request: its own thread decodes it on its own context
};
struct Combiner {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<DecReq *> pending;
    bool collecting = false;        // a leader is gathering `pending`
    std::atomic<int> arriving{0};   // threads between entry and submission
    int last_batch = 1;             // requests of the most recent batch (> 1: the process decodes concurrently)
};
Combiner &combiner(int device) { static Combiner c[64]; return c[device & 63]; }
// grace in microseconds the leader grants late arrivals once the process has shown concurrent decode calls; < 0 = combiner off
int combine_grace_us()
{
    static const int v = (int)jpk_env_long("JPK_COMBINE_US", 300, INT_MIN, INT_MAX);
    return v;
}
}  // namespace

// test hook (JPK_DEBUG_HOOKS=1 only): the next `n` merged decode passes are treated as failed as a whole before they run, as if the
// combiner context could not be had -- every merged request must then come back through its own thread's single-block path
namespace { std::atomic<int> g_combiner_fail_next{0}; }
extern "C" int jpk_debug_combiner_fail_next(int n)
{
    if (!jpk_debug_hooks_on() || n < 0) return JPK_E_ARG;
    g_combiner_fail_next.store(n);
    return JPK_OK;
}

// test hook: requests the most recent combined decode on `device` carried (1 = a lone caller took the single-block path)
extern "C" int jpk_debug_combiner_last_batch(int device)
{
    if (device < 0 || device >= 64) return JPK_E_ARG;
    Combiner &cb = combiner(device);
    std::lock_guard<std::mutex> lk(cb.mu);
    return cb.last_batch;
}

namespace {
// Stage and submit: the input to the thread's stage_in, behind it the event the merged pass waits for; the request joins `pending`.
// *leader: nobody was collecting -- the caller leads this batch.  Otherwise returns once a leader has marked the request done.
int combiner_submit(Combiner &cb, jpk_ctx *ctx, const uint8_t *in, int32_t in_len, int32_t out_cap, DecReq &req, bool *leader)
{
    cb.arriving.fetch_add(1);
    struct Arrived { Combiner &c; bool in = true; ~Arrived() { if (in) c.arriving.fetch_sub(1); } void submitted() { if (in) { c.arriving.fetch_sub(1); in = false; } } } arrived{cb};
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_in, &ctx->stage_in_cap, (size_t)in_len + 64));
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_res, &ctx->stage_res_cap, (size_t)out_cap + 64));
    JPK_HIP(hipMemcpyAsync(ctx->stage_in, in, (size_t)in_len, hipMemcpyHostToDevice, ctx->stream));
    JPK_HIP(hipEventRecord(ctx->ev_batch, ctx->stream));
    req.d_in = ctx->stage_in; req.in_len = in_len; req.d_out = ctx->stage_res; req.out_cap = out_cap; req.staged = ctx->ev_batch;
    std::unique_lock<std::mutex> lk(cb.mu);
    cb.pending.push_back(&req);
    arrived.submitted();
    *leader = !cb.collecting;
    if (*leader) cb.collecting = true;
    else cb.cv.wait(lk, [&] { return req.done; });
    return JPK_OK;
}

// The leader's gather: until nobody is on the way in; once the process has decoded concurrently before, a grace period on top.
// Returns the requests of this batch; the next arrival leads a batch of its own.
std::vector<DecReq *> combiner_gather(Combiner &cb)
{
    const auto t0 = std::chrono::steady_clock::now();
    int grace;
    { std::lock_guard<std::mutex> lk(cb.mu); grace = cb.last_batch > 1 ? combine_grace_us() : 0; }
    for (;;) {
        const auto waited = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (cb.arriving.load() == 0 && waited >= grace) break;
        if (waited > 20000) break;                              // a thread stuck in its staging must not hold the others
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    std::vector<DecReq *> batch;
    std::lock_guard<std::mutex> lk(cb.mu);
    batch.swap(cb.pending);
    cb.collecting = false;                                   // the next arrival leads a batch of its own, beside this one
    return batch;
}

// the merged pass is bounded: requests beyond JPK_COMBINE_MAX_MIB (default 2048) of output capacity stay with their own
// threads, so that the hidden combiner context's arena (~3 bytes per output byte) cannot grow without limit
void combiner_cap(std::vector<DecReq *> &batch, std::vector<DecReq *> &turned_away)
{
    static const size_t max_bytes = (size_t)jpk_env_long("JPK_COMBINE_MAX_MIB", 2048, 1) << 20;
    size_t bytes = 0;
    std::vector<DecReq *> kept;
    for (DecReq *r : batch) {
        if (!kept.empty() && bytes + (size_t)r->out_cap > max_bytes) { r->alone = true; turned_away.push_back(r); continue; }
        bytes += (size_t)r->out_cap;
        kept.push_back(r);
    }
    batch.swap(kept);
}

// The merged pass: the batch's requests in one jpk_ans_decode_batch on a combiner context of the device, behind their staging
// events.  A pass that fails as a whole hands every request back to its own thread.
void combiner_merged_pass(int device, std::vector<DecReq *> &batch)
{
    const int nb = (int)batch.size();
    int rc = JPK_OK;
    jpk_ctx *cc = nullptr;
    if (g_combiner_fail_next.load() > 0 && g_combiner_fail_next.fetch_sub(1) > 0) rc = JPK_E_ALLOC;     // (test hook)
    else rc = jpk_batch_ctx_acquire(device, &cc);
    const uint64_t generation = jpk_pool_generation();
    if (rc == JPK_OK) {
        std::vector<const uint8_t *> ins((size_t)nb);
        std::vector<uint8_t *> outs((size_t)nb);
        std::vector<int32_t> il((size_t)nb), oc((size_t)nb), ol((size_t)nb), st((size_t)nb);
        for (int b = 0; b < nb && rc == JPK_OK; b++) {
            ins[b] = batch[b]->d_in; il[b] = batch[b]->in_len; outs[b] = batch[b]->d_out; oc[b] = batch[b]->out_cap;
            if (hipStreamWaitEvent(cc->stream, batch[b]->staged, 0) != hipSuccess) rc = JPK_E_DEVICE;
        }
        if (rc == JPK_OK) rc = jpk_ans_decode_batch(cc, nb, ins.data(), il.data(), outs.data(), oc.data(), ol.data(), st.data(), 0);   // synchronises cc->stream
        if (rc != JPK_OK) (void)hipStreamSynchronize(cc->stream);      // nothing of the failed pass may still touch the requests' buffers
        for (int b = 0; b < nb && rc == JPK_OK; b++) { batch[b]->out_len = ol[b]; batch[b]->status = st[b]; }
        jpk_batch_ctx_release(device, cc, generation);
    }
    // The pass as a WHOLE failed (no combiner context, its arena for N blocks did not fit beside the callers' own arenas, a
    // stream error): that says nothing about any single request -- each would have gone through on the single-block path
    // with its own context.  Every thread retries its own request alone (per-block statuses of a pass that ran stand).
    if (rc != JPK_OK)
        for (int b = 0; b < nb; b++) { batch[b]->alone = true; batch[b]->status = JPK_OK; batch[b]->out_len = 0; }
}

// Wake: the batch's size is on record, every request of it is done -- decoded, or handed back to its own thread.
void combiner_wake(Combiner &cb, int nb, const std::vector<DecReq *> &batch, const std::vector<DecReq *> &turned_away)
{
    {
        std::lock_guard<std::mutex> lk(cb.mu);
        cb.last_batch = nb;
        for (DecReq *r : batch) r->done = true;
        for (DecReq *r : turned_away) r->done = true;
    }
    cb.cv.notify_all();
}
}  // namespace

extern "C" int jpk_ans_decode(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t threads)
{
    (void)threads;
    if (combine_grace_us() < 0) return staged(jpk_dev_ans_decode, in, in_len, out, out_cap, out_len, false);
    if (!staged_args_ok(in, in_len, out, out_cap, out_len)) return JPK_E_ARG;
    jpk_ctx *ctx;
    JPK_TRY(jpk_tls_ctx(&ctx));
    JPK_HIP(hipSetDevice(ctx->device));
    if (ctx->device < 0 || ctx->device >= 64 || in_len == 0) return staged(jpk_dev_ans_decode, in, in_len, out, out_cap, out_len, false);
    Combiner &cb = combiner(ctx->device);
    DecReq req;
    bool leader;
    JPK_TRY(combiner_submit(cb, ctx, in, in_len, out_cap, req, &leader));
    if (leader) {
        std::vector<DecReq *> batch = combiner_gather(cb), turned_away;
        combiner_cap(batch, turned_away);
        const int nb = (int)batch.size();
        if (nb == 1 && batch[0] != &req) { batch[0]->alone = true; turned_away.push_back(batch[0]); batch.clear(); }
        else if (nb == 1) req.status = jpk_dev_ans_decode(ctx, req.d_in, req.in_len, req.d_out, req.out_cap, &req.out_len);       // the single-block path, as ever
        else combiner_merged_pass(ctx->device, batch);
        combiner_wake(cb, nb, batch, turned_away);
    }
    if (req.alone) {
        req.status = jpk_dev_ans_decode(ctx, req.d_in, req.in_len, req.d_out, req.out_cap, &req.out_len);
    }
    if (req.status != JPK_OK) return req.status;
    return staged_finish(ctx, ctx->stage_res, req.out_len, out, out_len);
}

extern "C" int jpk_ans_decoded_size(const uint8_t *in, int32_t in_len, int64_t *decoded_len, int32_t *chunks)
{
    if (!decoded_len || in_len < 0 || (in_len > 0 && !in)) return JPK_E_ARG;
    return jrs::ans_decoded_size(in, in_len, decoded_len, chunks);          // the chunk-header walk is part of the resync rule (jam_resync.hpp)
}

extern "C" int jpk_block_compress(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    return staged(jpk_dev_block_compress, in, in_len, out, out_cap, out_len, false);
}

extern "C" int jpk_block_decompress(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    return staged(jpk_dev_block_decompress, in, in_len, out, out_cap, out_len, false);
}

// the rank coder on host buffers, either way: t travels in and comes back transformed in place; the table comes back (encode) or
// travels in (decode)
static int rank_staged(bool encode, uint8_t *t, int32_t *freq256, int32_t len)
{
    if (!freq256 || len < 0 || (len > 0 && !t)) return JPK_E_ARG;
    jpk_ctx *ctx;
    JPK_TRY(jpk_host_enter(&ctx, (size_t)len + 2048));
    uint8_t *d_t = ctx->stage_in + 1024;
    int32_t *d_f = (int32_t *)ctx->stage_in;
    if (len) JPK_HIP(hipMemcpyAsync(d_t, t, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
    if (!encode) JPK_HIP(hipMemcpyAsync(d_f, freq256, 1024, hipMemcpyHostToDevice, ctx->stream));
    JPK_TRY(encode ? jpk_rank_encode_device(ctx, d_t, d_f, len) : jpk_rank_decode_device(ctx, d_t, d_f, len));
    if (len) JPK_HIP(hipMemcpyAsync(t, d_t, (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
    if (encode) JPK_HIP(hipMemcpyAsync(freq256, d_f, 1024, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    return JPK_OK;
}
extern "C" int jpk_rank_encode(uint8_t *t, int32_t *freq256, int32_t len) { return rank_staged(true, t, freq256, len); }
extern "C" int jpk_rank_decode(uint8_t *ranks, const int32_t *freq256, int32_t len) { return rank_staged(false, ranks, const_cast<int32_t *>(freq256), len); }

extern "C" int jpk_checksum(const uint8_t *in, int32_t in_len, uint32_t *crc)
{
    if (!crc || in_len < 0 || (in_len > 0 && !in)) return JPK_E_ARG;
    jpk_ctx *ctx;
    JPK_TRY(jpk_host_enter(&ctx, (size_t)in_len + 64));
    if (in_len) JPK_HIP(hipMemcpyAsync(ctx->stage_in, in, (size_t)in_len, hipMemcpyHostToDevice, ctx->stream));
    return jpk_dev_checksum(ctx, ctx->stage_in, in_len, crc);
}

extern "C" int jpk_jam_block_write(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    auto write = [block_size](jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out, int32_t cap, int32_t *n) {
        return jpk_dev_jam_block_write(ctx, d_in, len, block_size, d_out, cap, n);
    };
    return staged(write, in, in_len, out, out_cap, out_len, false);
}

extern "C" int jpk_jam_block_read(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t *consumed)
{
    if (in_len >= JPK_JAM_HEADER_BYTES && in) {      // stage only this frame, not the rest of the stream
        int32_t csize;
        memcpy(&csize, in + 7, 4);
        if (csize < 0 || csize > JPK_MAX_BLOCKSIZE || (int64_t)csize + JPK_JAM_HEADER_BYTES > in_len) return JPK_E_CORRUPT;
        in_len = csize + JPK_JAM_HEADER_BYTES;
    }
    int32_t used = 0;
    auto read = [&used](jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out, int32_t cap, int32_t *n) {
        return jpk_dev_jam_block_read(ctx, d_in, len, d_out, cap, n, &used);
    };
    const int rc = staged(read, in, in_len, out, out_cap, out_len, false);
    if (rc == JPK_OK && consumed) *consumed = used;
    return rc;
}

namespace {
// a frame's stage chain on the host, encoder side: jpk_cli_stages_encode_ex (S4) or jpk_staged_s2_host (S2)
typedef int (*FrameStagesEncode)(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags);
// ... and decoder side: the n bytes InverseBwt left in a -> out; a and b are the two stage buffers of cap bytes
typedef int (*FrameStagesDecode)(uint8_t *a, int32_t n, uint8_t *b, int32_t cap, uint8_t *out, int32_t out_cap, int32_t *out_len);

// One frame on host buffers: crc (jampack.cpp:31), the stage chain `stages` on the host in place of Jampack::Comp()'s pre-stage
// encoders (jampack.cpp:36-39), ForwardBwt + Ans::Encode on the GPU, the header of CompWriteBlock (jampack.cpp:122-135) with
// `field_bits` set in the BlockSize field.
int frame_write(FrameStagesEncode stages, int32_t field_bits, const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len,
                uint32_t flags)
{
    if (!out || !out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !in) || !JPK_CLI_FLAGS_OK(flags)) return JPK_E_ARG;
    if (!jpk_jam_block_size_ok(block_size) || in_len > block_size) return JPK_E_ARG;     // InitComp, jampack.cpp:70
    if (out_cap < JPK_JAM_HEADER_BYTES) return JPK_E_CAPACITY;
    const int32_t cap = (int32_t)jpk_cli_stages_bound(in_len);                       // < 2^31 for in_len <= JPK_MAX_BLOCKSIZE (prestage.cpp); |S2| <= n + 2 + 2 P, two below it
    static thread_local std::vector<uint8_t> s;
    try { if (s.size() < (size_t)cap) s.resize((size_t)cap); } catch (...) { return JPK_E_ALLOC; }
    int32_t m = 0, n = 0;
    JPK_TRY(stages(in, in_len, s.data(), cap, &m, flags));
    JPK_TRY(jpk_block_compress(s.data(), m, out + JPK_JAM_HEADER_BYTES, out_cap - JPK_JAM_HEADER_BYTES, &n));
    jpk_jam_header_write(out, jpk_checksum_host(in, in_len), n, block_size | field_bits);
    *out_len = n + JPK_JAM_HEADER_BYTES;
    return JPK_OK;
}

// One frame read back: the header h (jampack.cpp:140-164; the frame's own bytes, or a copy with its flag bits cleared), Ans::Decode +
// InverseBwt on the GPU, the host stages `stages`, the crc check (jampack.cpp:58-59).
int frame_read(FrameStagesDecode stages, const uint8_t *h, const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t *consumed)
{
    uint32_t crc;
    int32_t csize, block_size;
    if (!jpk_jam_header_parse(h, in_len, &crc, &csize, &block_size)) return JPK_E_CORRUPT;
    const int64_t cap64 = (int64_t)((double)block_size * 1.05) + 4096;             // the reference's stage buffers, jampack.cpp:156
    if (cap64 > 0x7fffffff) return JPK_E_ARG;
    const int32_t cap = (int32_t)cap64;
    // the two 1.05 x BlockSize stage buffers of the reference (jampack.cpp:156-159), kept per thread across frames
    static thread_local std::vector<uint8_t> a, b;
    try { if (a.size() < (size_t)cap) a.resize((size_t)cap); if (b.size() < (size_t)cap) b.resize((size_t)cap); } catch (...) { return JPK_E_ALLOC; }
    int32_t n = 0, m = 0;
    JPK_TRY(jpk_block_decompress(in + JPK_JAM_HEADER_BYTES, csize, a.data(), cap, &n));     // Ans::Decode + InverseBwt
    JPK_TRY(stages(a.data(), n, b.data(), cap, out, out_cap, &m));
    if (jpk_checksum_host(out, m) != crc) return JPK_E_CORRUPT;                              // "Detected corrupt block!"
    *out_len = m;
    if (consumed) *consumed = csize + JPK_JAM_HEADER_BYTES;
    return JPK_OK;
}

// the host pre-stage decoders in the order of Jampack::Decomp() (jampack.cpp:47-57)
int cli_stages_decode(uint8_t *a, int32_t n, uint8_t *b, int32_t cap, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    int32_t m = 0;
    JPK_TRY(jpk_lz77_decompress(a, n, b, cap, &m));                                          // Lz->Decompress
    JPK_TRY(jpk_lpx_decode(b, m, a));                                                        // LocalModel->Decode
    JPK_TRY(jpk_filters_decode(a, m, b, cap, &n));                                           // Filter->Decode
    return jpk_lz77_decompress(b, n, out, out_cap, out_len);                                 // Lz->Decompress
}
// ... and without its lines 51-52, for staged frames
int staged_stages_decode(uint8_t *a, int32_t n, uint8_t *b, int32_t cap, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    int32_t m = 0;
    JPK_TRY(jpk_filters_decode(a, n, b, cap, &m));                                           // Filter->Decode
    return jpk_lz77_decompress(b, m, out, out_cap, out_len);                                 // Lz->Decompress
}
}  // namespace

// One frame of the stock CLI: header (jampack.cpp:140-164), GPU stages, host pre-stage decoders in the order of
// Jampack::Decomp() (jampack.cpp:47-57), crc check (jampack.cpp:58-59).
extern "C" int jpk_jam_cli_block_read(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t *consumed)
{
    if (!in || !out || !out_len || in_len < 0 || out_cap < 0) return JPK_E_ARG;
    return frame_read(cli_stages_decode, in, in, in_len, out, out_cap, out_len, consumed);
}

// The counterpart: the stage chain of jpk_cli_stages_encode on the host.
extern "C" int jpk_jam_cli_block_write_ex(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags)
{
    return frame_write(jpk_cli_stages_encode_ex, 0, in, in_len, block_size, out, out_cap, out_len, flags);
}

extern "C" int jpk_jam_cli_block_write(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    return jpk_jam_cli_block_write_ex(in, in_len, block_size, out, out_cap, out_len, 0u);
}

// One staged frame ("Staged frames"): Jampack::Comp() (jampack.cpp:29-44) with the stage chain stopped at S2 -- no
// LocalModel->Encode, no second Lz->Compress (jampack.cpp:38-39) --, the header of CompWriteBlock with JPK_JAM_STAGED in the BlockSize field.
extern "C" int jpk_jam_staged_block_write(const uint8_t *in, int32_t in_len, int32_t block_size, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags)
{
    return frame_write(jpk_staged_s2_host, JPK_JAM_STAGED, in, in_len, block_size, out, out_cap, out_len, flags);
}

// The reader: Jampack::Decomp() (jampack.cpp:47-60) without its lines 51-52 -- Ans::Decode + InverseBwt on the GPU, Filter->Decode and
// Lz->Decompress on the host, the crc check.  A header without JPK_JAM_STAGED is not a staged frame: JPK_E_CORRUPT.
extern "C" int jpk_jam_staged_block_read(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len, int32_t *consumed)
{
    if (!in || !out || !out_len || in_len < 0 || out_cap < 0) return JPK_E_ARG;
    if (in_len < JPK_JAM_HEADER_BYTES || (in[14] & 0xC0u) != 0x40u) return JPK_E_CORRUPT;   // bit 30 of the little-endian BlockSize field, bit 31 clear
    uint8_t h[JPK_JAM_HEADER_BYTES];
    memcpy(h, in, sizeof h);
    h[14] &= 0xBFu;
    return frame_read(staged_stages_decode, h, in, in_len, out, out_cap, out_len, consumed);
}

