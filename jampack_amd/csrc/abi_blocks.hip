// abi_blocks.hip -- the batch engines of the C ABI: jpk_dev_blocks_ans_decode, jpk_dev_blocks_decompress and
// jpk_dev_blocks_compress with its group planner, and their host-logic probes.
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "abi.hpp"

namespace {
// the block-list arguments of the batch entries: every array when there are blocks, every block's lengths and buffers
int blocks_args_check(int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap, const int32_t *out_len)
{
    if (nblocks < 0 || (nblocks > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len))) return JPK_E_ARG;
    for (int b = 0; b < nblocks; b++)
        if (in_len[b] < 0 || out_cap[b] < 0 || !d_out[b] || (in_len[b] > 0 && !d_in[b])) return JPK_E_ARG;
    return JPK_OK;
}
}  // namespace

// ---- batches of independent blocks -------------------------------------------------------------------------------------------
// The serial entropy-decode kernels run one wave per 1 MiB chunk; a 64 MiB block keeps 65 of the chip's 1024 SIMDs busy.  A
// batch runs ONE grid per stage over the chunks of all its blocks, so sixteen blocks fill the chip whatever the hardware
// queues do with concurrent kernels (tools/conctest.hip).
extern "C" int jpk_dev_blocks_ans_decode(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                         const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    JPK_ENTER(ctx);
    JPK_TRY(blocks_args_check(nblocks, d_in, in_len, d_out, out_cap, out_len));
    if (nblocks == 0) return JPK_OK;
    std::vector<int32_t> st_local;
    int32_t *stp = jpk_status_or_local(status, st_local, nblocks);
    JPK_TRY(jpk_ans_decode_batch(ctx, nblocks, d_in, in_len, d_out, out_cap, out_len, stp, 0));
    return status ? JPK_OK : jpk_first_error(stp, nblocks);
}

namespace {
// one jpk_dev_blocks_decompress call: its arguments, and what each step leaves for the next
struct InvCall {
    jpk_ctx *ctx; int32_t nblocks; uint8_t *const *d_out; const int32_t *out_cap; int32_t *out_len, *stp;
    std::vector<int32_t> mid_cap, mid_len;                     // the BWT images: capacity (out_cap + trailer), decoded length
    size_t mid_total = 0, bound = 0;                           // the images' bytes in the arena; the batch decoder's buffers at most
    uint32_t nmax = 1;                                         // the largest out_cap
    bool batched = false;
    int lanes = 1;
    hipStream_t lane_stream[jpk_ctx::INV_LANES_MAX] = {};
    hipEvent_t lane_event[jpk_ctx::INV_LANES_MAX] = {};
    std::vector<int> group_end;                                // batched: group g ends in front of block group_end[g]
    size_t batch_bytes_max = 0;                                // ... and the largest group's scratch
    size_t inv_one = 0, inv_bytes = 0;                         // scratch of one lane; everything in front of the images
    uint32_t *d_verdict = nullptr;
    std::vector<uint8_t *> mid;
    std::vector<int> ran;                                      // blocks whose inverse BWT was enqueued
    std::vector<std::vector<uint8_t>> host_jobs;               // the batched inverse BWTs' job tables: copied from here asynchronously
};

// The per-block bounds: every image's capacity (JPK_E_ARG when it passes 2^31 - 1), their sum, the largest block, the decoder's bound.
int inv_block_bounds(InvCall &C, const int32_t *in_len)
{
    for (int b = 0; b < C.nblocks; b++) {
        const int64_t mc = (int64_t)C.out_cap[b] + JPK_TRAILER_BYTES;
        if (mc > 0x7fffffffLL) return JPK_E_ARG;
        C.mid_cap[b] = (int32_t)mc;
        C.mid_total += jpk_align((size_t)mc + 64);
        if ((uint32_t)C.out_cap[b] > C.nmax) C.nmax = (uint32_t)C.out_cap[b];
        // what the batch decoder can need for this block at most: rank array + 2-byte RLE0 symbols + chunk tables
        C.bound += (size_t)mc * 3 + ((size_t)in_len[b] / 275 + 2) * 1100 + 4096;
    }
    return JPK_OK;
}

// Lanes or batch -- a function of nblocks, nmax and the three switches alone: C.batched, and the lanes the call asks for.
void inv_choose_mode(InvCall &C)
{
    const int32_t nblocks = C.nblocks;
    // Lanes: an inverse BWT is ~30 dependent launches of which only the walk fills the chip (1.6 of 2.5 ms for 64 MiB, the rest
    // is 20-microsecond rank-jump rounds and launch gaps), so up to three run side by side, each on its own stream with its own
    // scratch, behind one event on the decode stream.
    static const int max_lanes = (int)jpk_env_long("JPK_INV_LANES", 3, 1, jpk_ctx::ENC_GROUPS);
    // ... and up to JPK_INV_LANES_SMALL (default 12) when the batch is many SMALL blocks (<= 4 MiB): an inverse BWT of a 1 MiB block is
    // the same ~30 dependent launches, each a sliver of the chip, and 256 of them on three lanes took 100 ms of a 245 ms call whose
    // chains had finished after 145 (round 4: 1 070 -> 1 400 MB/s with 8 to 16 lanes; what is left is the host's launch rate, 7 700
    // launches per call).  Blocks of 8 MiB gain nothing (nine chains per block: the chains are the call) and would pay 12 scratch areas.
    static const int small_lanes = (int)jpk_env_long("JPK_INV_LANES_SMALL", 12, 1, jpk_ctx::INV_LANES_MAX);
    // Only a batch with many blocks gets lanes: they save the latency part of each inverse BWT (~1 ms of 2.5), nothing next to
    // the 270 ms of a small batch's chains, and every extra stream of a context lands on a hardware queue that another
    // context's chain kernels may be using (eight contexts decoding 2-block passes lost 18 % with a second stream each).
    const bool many_small = nblocks >= 32 && C.nmax <= (4u << 20);
    // ... or, by default, through ONE set of launches over all of them (bwt_inv.hip jpk_inv_bwt_batch_enqueue; JPK_INV_BATCH=0 keeps the lanes)
    static const bool batch_on = jpk_env_long("JPK_INV_BATCH", 1) != 0;
    // (in groups of consecutive blocks whose scratch fits 8 GiB.  Batches of LARGE blocks gain nothing from it --
    // 16 / 32 / 64 blocks of 64 MiB: 310 / 350 / 438 ms against 309 / 348 / 435 on the three lanes: their walks fill the chip -- and stay
    // on the lanes.)
    C.batched = batch_on && many_small;
    C.lanes = (nblocks < 8 || C.batched) ? 1 : (many_small ? (small_lanes > max_lanes ? small_lanes : max_lanes) : max_lanes);
}

// The lane streams and their events, made on first use; C.lanes shrinks to what could be had.  Lane 0 is the context's stream.
void inv_lane_streams(InvCall &C)
{
    jpk_ctx *ctx = C.ctx;
    C.lane_stream[0] = ctx->stream;
    for (int k = 1; k < C.lanes; k++) {
        hipStream_t *slot = k < jpk_ctx::ENC_GROUPS ? &ctx->aux[k - 1] : &ctx->inv_lane[k];
        hipEvent_t *ev = k < jpk_ctx::ENC_GROUPS ? &ctx->ev_done[k] : &ctx->ev_inv[k];
        if ((!*slot && hipStreamCreateWithFlags(slot, hipStreamNonBlocking) != hipSuccess) ||
            (!*ev && hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess)) { C.lanes = k; break; }
        C.lane_stream[k] = *slot;
        C.lane_event[k] = *ev;
    }
}

constexpr size_t INV_BATCH_BUDGET = (size_t)8 << 30;

// groups of consecutive blocks whose batch scratch fits the budget (many small blocks: one group): group g ends in front of block
// group_end[g]; a block that passes the budget alone is a group of its own.  Returns the largest group's scratch.  No device call.
size_t inv_batch_plan(int32_t nblocks, const int32_t *mid_cap, size_t batch_budget, std::vector<int> &group_end)
{
    size_t batch_bytes_max = 0;
    int b0 = 0;
    while (b0 < nblocks) {
        // (extended block by block: a job adds its own bytes and tiles, the tables follow from the totals; at most 65 535 jobs --
        // the batch launches use blockIdx.y = the job)
        int e = b0 + 1;
        size_t job_bytes = 0, tiles = 0;
        jpk_inv_bwt_batch_plan_add(mid_cap[(size_t)b0], &job_bytes, &tiles);
        size_t need = jpk_inv_bwt_batch_plan_total(1, job_bytes, tiles);
        while (e < nblocks && e - b0 < JPK_INV_BATCH_MAX_JOBS) {
            size_t jb2 = job_bytes, t2 = tiles;
            jpk_inv_bwt_batch_plan_add(mid_cap[(size_t)e], &jb2, &t2);
            const size_t more = jpk_inv_bwt_batch_plan_total(e + 1 - b0, jb2, t2);
            if (more > batch_budget) break;
            need = more; job_bytes = jb2; tiles = t2;
            e++;
        }
        if (need > batch_bytes_max) batch_bytes_max = need;
        group_end.push_back(e);
        b0 = e;
    }
    return batch_bytes_max;
}

// arena: [inverse-BWT scratch of the largest block x lanes][one verdict per block][BWT images of all blocks][the batch
// decoder's buffers]; sized once so that it cannot move while the images sit in it.
int inv_arena_layout(InvCall &C)
{
    jpk_ctx *ctx = C.ctx;
    C.inv_one = jpk_align(jpk_inv_bwt_arena_bytes(C.nmax), 4096);
    const size_t verdict_bytes = jpk_align((size_t)C.nblocks * 16 + 64, 4096);
    C.inv_bytes = (C.batched ? jpk_align(C.batch_bytes_max, 4096) : C.inv_one * (size_t)C.lanes) + verdict_bytes;
    JPK_TRY(jpk_arena_ensure(ctx, C.inv_bytes + C.mid_total + C.bound + (1u << 20)));
    C.d_verdict = reinterpret_cast<uint32_t *>(ctx->arena + C.inv_bytes - verdict_bytes);
    C.mid.resize((size_t)C.nblocks);
    size_t off = C.inv_bytes;
    for (int b = 0; b < C.nblocks; b++) { C.mid[b] = ctx->arena + off; off += jpk_align((size_t)C.mid_cap[b] + 64); }
    return JPK_OK;
}

// the inverse BWTs are enqueued without a host round trip between them (trailer index, slot count and the head check stay
// on the device); their verdicts come back in one copy.  A block that cannot run gets its status here; C.ran lists the others.
int inv_enqueue(InvCall &C)
{
    jpk_ctx *ctx = C.ctx;
    const int32_t nblocks = C.nblocks;
    const int lanes = C.lanes;
    const bool batched = C.batched;
    hipStream_t *lane_stream = C.lane_stream;
    int32_t *stp = C.stp, *out_len = C.out_len;
    const int32_t *out_cap = C.out_cap;
    const std::vector<int32_t> &mid_len = C.mid_len;
    const std::vector<uint8_t *> &mid = C.mid;
    uint8_t *const *d_out = C.d_out;
    uint32_t *d_verdict = C.d_verdict;
    std::vector<int> &ran = C.ran;
    struct Restore {                                       // whatever happens below, the context gets its stream and base back
        jpk_ctx *c; hipStream_t s; hipStream_t *lane; int lanes; bool failed = true;
        ~Restore()
        {
            c->stream = s; c->arena_base = 0;
            // an early return leaves inverse BWTs queued on the lane streams that read the images and write the arena and the
            // callers' buffers: nothing may reuse the arena before they have drained (the main stream never waited for them)
            if (failed) for (int k = 1; k < lanes; k++) if (lane[k]) (void)hipStreamSynchronize(lane[k]);
        }
    } restore{ctx, ctx->stream, lane_stream, lanes};
    hipStream_t main_stream = ctx->stream;
    if (lanes > 1) {
        JPK_HIP(hipEventRecord(ctx->ev_batch, main_stream));       // the decoded images are complete
        for (int k = 1; k < lanes; k++) JPK_HIP(hipStreamWaitEvent(lane_stream[k], ctx->ev_batch, 0));
    }
    int next = 0;
    std::vector<int> jb;                                   // blocks that go through the batched inverse BWT
    for (int b = 0; b < nblocks; b++) {
        out_len[b] = 0;
        if (stp[b] != JPK_OK) continue;
        if (mid_len[b] < JPK_TRAILER_BYTES) { stp[b] = JPK_E_CORRUPT; continue; }
        if (mid_len[b] - JPK_TRAILER_BYTES > out_cap[b]) { stp[b] = JPK_E_CAPACITY; continue; }
        if (batched && mid_len[b] - JPK_TRAILER_BYTES >= JPK_BWT_UNITS) { jb.push_back(b); continue; }   // (a shorter image has no sorted part: two copies, below)
        const int k = next % lanes;
        ctx->stream = lane_stream[k];
        ctx->arena_base = C.inv_one * (size_t)k;
        const int rc = jpk_inv_bwt_enqueue(ctx, mid[b], mid_len[b], d_out[b], d_verdict + 4 * (size_t)b);
        if (rc != JPK_OK) { stp[b] = rc; continue; }
        ran.push_back(b);
        next++;
    }
    ctx->stream = main_stream;
    // one batch per group, one after the other on the main stream (they share the scratch at the start of the arena)
    size_t jq = 0;
    for (size_t g = 0; g < C.group_end.size() && jq < jb.size(); g++) {
        std::vector<int> part;
        while (jq < jb.size() && jb[jq] < C.group_end[g]) part.push_back(jb[jq++]);
        if (part.empty()) continue;
        std::vector<const uint8_t *> jin(part.size());
        std::vector<uint8_t *> jout(part.size());
        std::vector<int32_t> jlen(part.size());
        for (size_t q = 0; q < part.size(); q++) { jin[q] = mid[part[q]]; jout[q] = d_out[part[q]]; jlen[q] = mid_len[part[q]]; }
        // (job q reports into the verdict slot of its block, part[q])
        ctx->arena_base = 0;
        C.host_jobs.emplace_back();
        const int rc = jpk_inv_bwt_batch_enqueue(ctx, (int)part.size(), jin.data(), jlen.data(), jout.data(), d_verdict, part.data(), C.host_jobs.back());
        if (rc != JPK_OK) { for (int b : part) stp[b] = rc; }
        else for (int b : part) ran.push_back(b);
    }
    for (int k = 1; k < lanes; k++) {                      // the main stream continues behind every lane
        JPK_HIP(hipEventRecord(C.lane_event[k], lane_stream[k]));
        JPK_HIP(hipStreamWaitEvent(main_stream, C.lane_event[k], 0));
    }
    restore.failed = false;
    return JPK_OK;
}

// The verdicts of the blocks that ran, in one copy behind everything on the stream: a block passes (its out_len) or is corrupt.
int inv_read_verdicts(InvCall &C)
{
    jpk_ctx *ctx = C.ctx;
    std::vector<uint32_t> verdict((size_t)C.nblocks * 4);
    if (!C.ran.empty()) JPK_HIP(hipMemcpyAsync(verdict.data(), C.d_verdict, (size_t)C.nblocks * 16, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof_on) jpk_prof_resolve(ctx);
    for (int b : C.ran) {
        if (verdict[4 * (size_t)b]) { C.stp[b] = JPK_E_CORRUPT; continue; }
        C.out_len[b] = C.mid_len[b] - JPK_TRAILER_BYTES;
    }
    return JPK_OK;
}
}  // namespace

extern "C" int jpk_dev_blocks_decompress(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                         const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    JPK_ENTER(ctx);
    JPK_TRY(blocks_args_check(nblocks, d_in, in_len, d_out, out_cap, out_len));
    if (nblocks == 0) return JPK_OK;
    std::vector<int32_t> st_local;
    InvCall C{ctx, nblocks, d_out, out_cap, out_len, jpk_status_or_local(status, st_local, nblocks)};
    C.mid_cap.resize((size_t)nblocks);
    C.mid_len.resize((size_t)nblocks);
    JPK_TRY(inv_block_bounds(C, in_len));
    inv_choose_mode(C);
    inv_lane_streams(C);
    if (C.batched) C.batch_bytes_max = inv_batch_plan(nblocks, C.mid_cap.data(), INV_BATCH_BUDGET, C.group_end);
    JPK_TRY(inv_arena_layout(C));
    JPK_TRY(jpk_ans_decode_batch(ctx, nblocks, d_in, in_len, C.mid.data(), C.mid_cap.data(), C.mid_len.data(), C.stp, C.inv_bytes + C.mid_total));
    JPK_TRY(inv_enqueue(C));
    JPK_TRY(inv_read_verdicts(C));
    return status ? JPK_OK : jpk_first_error(C.stp, nblocks);
}

// host-logic probe (no device call): the groups the batched inverse BWT of jpk_dev_blocks_decompress would cut nblocks blocks of
// these output capacities into under budget_bytes of scratch (0 = the production 8 GiB): group g ends in front of block group_end[g];
// returns the number of groups (at most nblocks)
extern "C" int jpk_debug_inv_batch_plan(int32_t nblocks, const int32_t *out_cap, int64_t budget_bytes, int32_t *group_end)
{
    if (nblocks < 0 || budget_bytes < 0 || (nblocks > 0 && (!out_cap || !group_end))) return JPK_E_ARG;
    std::vector<int32_t> mid_cap((size_t)nblocks);
    for (int b = 0; b < nblocks; b++) {
        if (out_cap[b] < 0 || out_cap[b] > 0x7fffffff - JPK_TRAILER_BYTES) return JPK_E_ARG;
        mid_cap[b] = out_cap[b] + JPK_TRAILER_BYTES;
    }
    std::vector<int> ends;
    inv_batch_plan(nblocks, mid_cap.data(), budget_bytes ? (size_t)budget_bytes : INV_BATCH_BUDGET, ends);
    for (size_t g = 0; g < ends.size(); g++) group_end[g] = ends[g];
    return (int)ends.size();
}


// ---- jpk_dev_blocks_compress: blocks in flight inside the library ---------------------------------------------------------
namespace {
// Small blocks -- the reference's default block is 8 MiB, its smallest 1 MiB (format.hpp:20-22), and Jampack::Compress feeds
// `Threads` of them at a time (jampack.cpp:205-224) -- are compressed in GROUPS: one suffix sort over the blocks of a group
// (jpk_fwd_bwt_group_device), one set of entropy grids over all their chunks (jpk_ans_encode_group_device), one host
// synchronisation per stage boundary of a group (four in all, below) instead of ~200 launches and a synchronisation per block.  Bytes per block are those of
// jpk_dev_block_compress.
constexpr int32_t GROUP_BLOCK_MAX = 16 << 20;       // blocks up to this size are grouped
// Bytes per group: large groups amortise best (a 256 MiB stream of 1 MiB blocks: 4.6 GB/s in groups of 64 MiB, 4.2 in groups of
// 16, 2.9 in groups of 8; of 8 MiB blocks: 3.6 / 3.5 / 3.1 -- profiles/r04_group_size.txt), but a short stream still wants several
// groups in flight: a quarter of the small blocks' bytes, between 8 and 64 MiB.  JPK_GROUP_MIB fixes it.
size_t group_target_bytes(size_t small_bytes_total)
{
    static const long fixed = jpk_env_long("JPK_GROUP_MIB", 0, 0, 512);
    if (fixed > 0) return (size_t)fixed << 20;
    size_t t = small_bytes_total / 4;
    if (t < ((size_t)8 << 20)) t = (size_t)8 << 20;
    if (t > ((size_t)64 << 20)) t = (size_t)64 << 20;
    return t;
}

struct Task { int first, count; };
// the work list of jpk_dev_blocks_compress: every block exactly once, in order; consecutive blocks of <= GROUP_BLOCK_MAX bytes form
// groups of at most 256 blocks and (beyond the first block) at most the target size; a larger block is a task of its own
void plan_tasks(int nblocks, const int32_t *in_len, std::vector<Task> &tasks)
{
    static const bool grouping = jpk_env_long("JPK_GROUP", 1) != 0;
    size_t small_total = 0;
    for (int k = 0; k < nblocks; k++) if (in_len[k] <= GROUP_BLOCK_MAX) small_total += (size_t)in_len[k];
    const size_t target = group_target_bytes(small_total);
    int b = 0;
    while (b < nblocks) {
        if (!grouping || in_len[b] > GROUP_BLOCK_MAX) { tasks.push_back(Task{b, 1}); b++; continue; }
        int e = b;
        size_t bytes = 0;
        while (e < nblocks && in_len[e] <= GROUP_BLOCK_MAX && e - b < 256 && (e == b || bytes + (size_t)in_len[e] <= target)) { bytes += (size_t)in_len[e]; e++; }
        tasks.push_back(Task{b, e - b});
        b = e;
    }
}

// what a group of these blocks needs: the staging buffer for the images and the arena (the larger of the two stages' layouts + the
// encoder's capacity sink); first[b] / mid[b] (nullable together): block b's first chunk in the staging buffer, its image's bytes
void group_needs(int nb, const int32_t *in_len, size_t *stage_bytes, size_t *arena_bytes, uint32_t *first = nullptr, int32_t *mid = nullptr)
{
    uint64_t nlen_total = 0;
    uint32_t nch = 0;
    for (int b = 0; b < nb; b++) {
        if (first) { first[b] = nch; mid[b] = in_len[b] + JPK_TRAILER_BYTES; }
        nch += ((uint32_t)in_len[b] + JPK_TRAILER_BYTES + JPK_ANS_CHUNK - 1) / JPK_ANS_CHUNK;
        nlen_total += (uint32_t)in_len[b] - (uint32_t)in_len[b] % JPK_BWT_UNITS;
    }
    *stage_bytes = (size_t)nch * JPK_ANS_CHUNK;
    const size_t a_sort = jpk_fwd_bwt_group_arena_bytes((uint32_t)nlen_total, nb), a_enc = jpk_ans_encode_group_arena_bytes(nch, nb);
    *arena_bytes = (a_sort > a_enc ? a_sort : a_enc) + (size_t)GROUP_BLOCK_MAX + (1u << 20);
}

// test hook (JPK_DEBUG_HOOKS=1 only): the next `n` groups fail as a whole before they run, as if their arena could not be had --
// every block of such a group must then come back through the single-block path with the same bytes
std::atomic<int> g_group_fail_next{0};

int group_compress(jpk_ctx *c, int nb, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap, int32_t *out_len,
                   int32_t *status)
{
    if (g_group_fail_next.load() > 0 && g_group_fail_next.fetch_sub(1) > 0) return JPK_E_ALLOC;
    std::vector<uint32_t> first((size_t)nb);
    std::vector<int32_t> mid((size_t)nb);
    size_t stage_bytes, arena_bytes;
    group_needs(nb, in_len, &stage_bytes, &arena_bytes, first.data(), mid.data());
    JPK_TRY(jpk_buf_ensure(c, &c->stage_out, &c->stage_out_cap, stage_bytes));
    JPK_TRY(jpk_arena_ensure(c, arena_bytes));
    std::vector<uint8_t *> img((size_t)nb);
    for (int b = 0; b < nb; b++) {
        img[b] = c->stage_out + (size_t)first[b] * JPK_ANS_CHUNK;
        // bwt.cpp:35: a block shorter than 120 bytes leaves its 480 trailer bytes alone -- defined bytes here, as in jpk_dev_block_compress
        if (in_len[b] < JPK_BWT_UNITS) JPK_HIP(hipMemsetAsync(img[b], 0, (size_t)mid[b], c->stream));
    }
    int rc = jpk_fwd_bwt_group_device(c, nb, d_in, in_len, img.data());
    if (rc == JPK_OK) rc = jpk_ans_encode_group_device(c, nb, c->stage_out, first.data(), mid.data(), d_out, out_cap, out_len, status);   // synchronises
    if (rc == JPK_OK) jpk_sa_stats_sync(c);
    else (void)hipStreamSynchronize(c->stream);            // the pinned tables and the staged images stay valid until the queue is empty
    return rc;
}
}  // namespace

extern "C" int jpk_dev_blocks_compress(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                       const int32_t *out_cap, int32_t *out_len, int32_t *status, int32_t in_flight)
{
    return jpk_blocks_compress_body(ctx, nblocks, d_in, in_len, d_out, out_cap, out_len, status, in_flight, nullptr);
}

int jpk_blocks_compress_body(jpk_ctx *ctx, int32_t nblocks, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                             const int32_t *out_cap, int32_t *out_len, int32_t *status, int32_t in_flight, JpkBlocksReady *ready)
{
    JPK_ENTER(ctx);
    JPK_TRY(blocks_args_check(nblocks, d_in, in_len, d_out, out_cap, out_len));
    if (nblocks == 0) return JPK_OK;
    if (ctx->device < 0 || ctx->device >= 64) return JPK_E_ARG;
    std::vector<int32_t> st_local;
    int32_t *stp = jpk_status_or_local(status, st_local, nblocks);
    // tasks: a large block, or a group of consecutive small ones (up to the target size / 256 blocks)
    std::vector<Task> tasks;
    plan_tasks(nblocks, in_len, tasks);
    const int ntasks = (int)tasks.size();
    // every worker sizes its staging buffer and arena for the largest group once, before it takes its first task: which worker gets
    // which group changes from call to call, and an arena that grows in the middle of a call costs a free + malloc + synchronise
    size_t max_stage = 0, max_arena = 0;
    for (const Task &t : tasks)
        if (t.count > 1) {
            size_t sb, ab;
            group_needs(t.count, in_len + t.first, &sb, &ab);
            if (sb > max_stage) max_stage = sb;
            if (ab > max_arena) max_arena = ab;
        } else if (in_len[t.first] <= (128 << 20)) {        // (larger blocks grow a worker's arena when it meets one: ten arenas of a 1000 MiB block would not fit)
            // ... and for the largest single block (end of round 6): a worker whose first call brought it the stream's short last blocks only grew
            // its arena in the middle of the NEXT call -- one call in six of a fresh process took 4.1-4.3 GB/s instead of 6.1-6.5
            const uint32_t n1 = (uint32_t)in_len[t.first];
            const size_t mid = (size_t)n1 + JPK_TRAILER_BYTES;
            const size_t fb = jpk_fwd_bwt_arena_bytes(n1), eb = jpk_ans_encode_arena_bytes((uint32_t)mid);
            if (mid > max_stage) max_stage = mid;
            if (fb > max_arena) max_arena = fb;
            if (eb > max_arena) max_arena = eb;
        }
    int nw = in_flight > 0 ? in_flight : 10;       // (10 since round 6, like the bench line: profiles/r06_blocks_in_flight.txt; 8 in rounds 4-5; an arena is 3.7 GB)
    if (nw > ntasks) nw = ntasks;
    if (nw > 16) nw = 16;
    const uint64_t generation = jpk_pool_generation();
    // Stream order: the workers' streams are the library's own.  Whatever the caller has queued on ctx->stream before this call
    // (the kernels that produce d_in[], the consumers of a previous d_out[]) must be ordered in front of them, as it is for
    // jpk_dev_block_compress on the caller's context: an event on ctx->stream that every worker stream waits for.  The call
    // returns when every block is complete (each worker synchronises its stream), so nothing needs ordering at the exit.
    JPK_HIP(hipEventRecord(ctx->ev_batch, ctx->stream));
    std::atomic<int> next{0};
    auto work = [&](jpk_ctx *c) {
        if (hipSetDevice(c->device) != hipSuccess) return;                  // a fresh thread starts on device 0
        if (c != ctx && hipStreamWaitEvent(c->stream, ctx->ev_batch, 0) != hipSuccess) return;   // leaves its share to the others
        if (max_arena && (jpk_buf_ensure(c, &c->stage_out, &c->stage_out_cap, max_stage) != JPK_OK || jpk_arena_ensure(c, max_arena) != JPK_OK)) {
            // no room for the largest group on this context: the groups say so themselves when they get here (single blocks may still fit)
        }
        for (;;) {
            const int k = next.fetch_add(1, std::memory_order_relaxed);
            if (k >= ntasks) return;
            const int b = tasks[(size_t)k].first, nb = tasks[(size_t)k].count;
            if (ready && !ready->wait(b, nb)) {                 // the copy of an input failed: the blocks nobody has taken yet say so
                for (int j = b; j < b + nb; j++) { out_len[j] = 0; stp[j] = JPK_E_DEVICE; }
                continue;
            }
            if (nb == 1) {
                out_len[b] = 0;
                stp[b] = jpk_dev_block_compress(c, d_in[b], in_len[b], d_out[b], out_cap[b], &out_len[b]);
                continue;
            }
            const int rc = group_compress(c, nb, d_in + b, in_len + b, d_out + b, out_cap + b, out_len + b, stp + b);
            if (rc != JPK_OK)                                   // the group as a whole failed (its ~46 B/byte arena or staging buffer, a device error):
                for (int j = b; j < b + nb; j++) {              // every block goes through the single-block path on this context (~50 B/byte of ITS size), as before grouping
                    out_len[j] = 0;
                    stp[j] = jpk_dev_block_compress(c, d_in[j], in_len[j], d_out[j], out_cap[j], &out_len[j]);
                }
        }
    };
    // workers 1 .. nw-1 on contexts of their own; a worker that cannot get one (or a thread that cannot be started) leaves its
    // share to the others
    std::vector<std::thread> threads;
    std::vector<jpk_ctx *> held;
    for (int k = 1; k < nw; k++) {
        jpk_ctx *c = nullptr;
        if (jpk_batch_ctx_acquire(ctx->device, &c) != JPK_OK) break;
        held.push_back(c);
        try { threads.emplace_back(work, c); } catch (...) { break; }      // std::system_error: the caller's thread does that share
    }
    work(ctx);
    for (auto &t : threads) t.join();
    for (jpk_ctx *c : held) jpk_batch_ctx_release(ctx->device, c, generation);
    return status ? JPK_OK : jpk_first_error(stp, nblocks);
}

extern "C" int jpk_debug_group_fail_next(int n)
{
    if (!jpk_debug_hooks_on() || n < 0) return JPK_E_ARG;
    g_group_fail_next.store(n);
    return JPK_OK;
}

// host-logic probe (no device call): the tasks jpk_dev_blocks_compress would form for these block lengths: task t covers blocks
// [first[t], first[t] + count[t]); returns the number of tasks (at most nblocks)
extern "C" int jpk_debug_group_plan(int32_t nblocks, const int32_t *in_len, int32_t *first, int32_t *count)
{
    if (nblocks < 0 || (nblocks > 0 && (!in_len || !first || !count))) return JPK_E_ARG;
    for (int b = 0; b < nblocks; b++) if (in_len[b] < 0) return JPK_E_ARG;
    std::vector<Task> tasks;
    plan_tasks(nblocks, in_len, tasks);
    for (size_t t = 0; t < tasks.size(); t++) { first[t] = tasks[t].first; count[t] = tasks[t].count; }
    return (int)tasks.size();
}

