// ans_enc.hip -- Ans::Encode (ans.cpp:113-234) on gfx950: per 1 MiB chunk
//   sorted-rank coding (rank.cpp:45-90) -> RLE0 (rle.cpp:22-47) -> exponent/mantissa models (model.cpp) ->
//   4-way interleaved byte rANS (rans_byte.hpp:62-110) -> LEB128 header (ans.cpp:272-285).
//
// Parallel restructuring (bytes identical to the reference):
//   rank coding   MTF rank of byte i = #symbols whose last occurrence is later than the previous occurrence of
//                 T[i]; last-occurrence tables are carried across 4 KiB tiles by a per-symbol max-scan, so every
//                 tile is independent, and inside a tile every run head counts its own window (the heads between it and
//                 the previous head of its symbol whose symbol does not come again before it: no recency list, no walk
//                 from head to head); the bucket scatter uses per-tile per-symbol prefix counts.
//   RLE0          run heads found per tile, run lengths through a per-chunk "zeros that follow the tile" table,
//                 output offsets by scans.
//   models        QuasiModel tables only change at fixed per-class symbol counts -> built in parallel from
//                 per-interval histograms; the AdaptiveModel CDF entries are independent scalar recurrences.
//   rANS          pair j lives in state lane j mod 4 -> four independent sequential chains per chunk that record
//                 (bytes, count) per step; byte positions are a prefix sum; payload scattered afterwards.
//
// Units (ans_enc.hpp is what they share; every kernel is defined in one unit, in its anonymous namespace, and launched only from it):
//   ans_enc_front.hip   rank coding (k_enc_hist, k_enc_prep, k_enc_mtf: run_rank) and RLE0 (k_rle_lz, k_rle_ext, k_rle_tiles, k_tile_prefix:
//                       run_rle)
//   ans_enc_model.hip   class ordinals, QuasiModel tables, AdaptiveModel recurrences (k_cls_*, k_quasi_build, k_adapt_*: run_model)
//   ans_enc_chain.hip   the back half: step records (k_pairs: run_pairs), the chains (k_rans_lanes: run_chain), emitted bytes per tile
//                       (k_emit_count, k_emit_prefix: run_emit_counts), headers and offsets (k_headers, k_out_offsets: run_offsets),
//                       placement (k_put_headers, k_put_payload: run_put)
//   ans_enc.hip         the arena layout (enc_layout, enc_plan_bytes), the launch order (k_density, k_order), the compact symbol layout
//                       (k_sym_layout), encode_core with its host steps, and the jpk_* entries
// What each stage hands the next (members of EncBufs, indexed by chunk):
//   run_rank         input bytes -> ranks, freq (the header's Freq[]); its own: tilecnt, lastpos, bstart
//   run_rle          ranks -> rle (RLE0 symbols, one chunk stride apart), rlen; its own: lz, ext, tcount, toff
//   k_sym_layout     rlen -> EncDims::sbase, lbase (where a chunk's symbol slots and lane records start); the two totals -> mailbox
//   run_model        rle, rlen -> ord, qcdf (QuasiModel tables), exph, mantad (AdaptiveModel outputs); its own: clscnt, clstotal, qhist,
//                    cls8, clist, seg_*
//   run_pairs        rle, rlen, ord, qcdf, exph, mantad -> recs (one 16-byte record per step, lane-major, padded with identity steps)
//   run_chain        recs, rlen -> x16 (low half of the state before every step), emask (emit masks), fstate, stamp
//   run_emit_counts  emask, rlen -> etsum (bytes of all later tiles), csize
//   run_offsets      freq, csize, rlen, stamp -> hdr, hsize, outoff; totals and the worst chain's stamps -> mailbox
//   run_put          hdr, hsize, outoff, fstate, x16, emask, etsum, csize -> the output stream(s)
#include <vector>

#include "ans_enc.hpp"
#include "chain_pool.hpp"

using namespace jpk;
using namespace jpk_enc;

namespace {

// `sym_total` / `lane_total`: slots of the symbol-indexed arrays and records of the rANS lanes over all chunks (the compact layout,
// EncDims::sbase; known once the RLE0 stage has run).  0: one slot per byte (the stand-alone probes).
void enc_layout(Arena &a, const EncDims &d, EncBufs &b, int what, size_t sym_total = 0, size_t lane_total = 0)
{
    const size_t tiles = (size_t)d.nch * d.tpc;
    const size_t stride = d.chunk;                 // rle symbols per chunk <= chunk bytes
    const size_t nsym = sym_total ? sym_total : (size_t)d.nch * stride;
    const size_t nlane = lane_total ? lane_total : (size_t)d.nch * 4 * rans_lane_stride(stride);
    const EncBufs keep = b;                        // (a second call adds the model / rANS stage to the rank / RLE0 buffers of the first)
    if (what & LAY_RANK) memset(&b, 0, sizeof b); else b = keep;
    if (what & LAY_RANK) {
        b.tilecnt = a.get<uint32_t>(tiles * 256);
        b.lastpos = a.get<int32_t>(tiles * 256);
        b.freq = a.get<int32_t>((size_t)d.nch * 256);
        b.bstart = a.get<uint32_t>((size_t)d.nch * 256);
        b.ranks = a.get<uint8_t>((size_t)d.nch * stride + 64);
    }
    if (what & LAY_RLE) {
        b.lz = a.get<uint32_t>(tiles);
        b.ext = a.get<uint32_t>(tiles);
        b.tcount = a.get<uint32_t>(tiles);
        b.toff = a.get<uint32_t>(tiles);
        b.rlen = a.get<uint32_t>(d.nch + 1);
        b.rle = a.get<uint16_t>((size_t)d.nch * stride + 64);
    }
    if (what & LAY_MODEL) {
        b.dens = a.get<uint32_t>(d.nch + 64);
        b.cmap = a.get<uint32_t>(d.nch + 64);
        b.clscnt = a.get<uint32_t>(tiles * 8);
        b.clstotal = a.get<uint32_t>((size_t)d.nch * 8);
        b.ord = a.get<uint32_t>(nsym);
        b.qhist = a.get<uint32_t>((size_t)d.nch * 6 * NQ * QSTRIDE);
        b.qcdf = a.get<uint32_t>((size_t)d.nch * 6 * NQ * QSTRIDE);
        b.exph = a.get<uint16_t>(7 * nsym);
        b.mantad = a.get<uint32_t>(nsym);
        b.cls8 = a.get<uint8_t>(nsym + 64);
        b.clist = a.get<uint32_t>(2 * ((nsym + 3) & ~(size_t)3) + 64);
        const size_t segs = (size_t)d.nch * 9 * d.tpc;
        b.seg_flag = a.get<uint32_t>(segs);
        b.seg_lo = a.get<int32_t>(segs);
        b.seg_end = a.get<int32_t>(segs);
        b.seg_start = a.get<int32_t>(segs);
        b.seg_tab = a.get<uint16_t>(segs * 32);
        b.seg_miss = a.get<uint16_t>(segs);
        b.seg_reach = a.get<uint16_t>(segs);
        b.recs = a.get<uint4>(nlane + RANS_SLACK) + (a.planning ? 0 : RANS_SLACK);   // slack in front: k_rans_lanes' prefetches past the last batch
        b.pairs = (what & LAY_PLAIN) ? a.get<uint32_t>((size_t)d.nch * stride * 2) : nullptr;
    }
    if (what & LAY_RANS) {
        b.x16 = a.get<uint16_t>(nlane + 64);       // low half of the state before every step, lane-major like recs
        b.emask = a.get<uint32_t>(nlane / 16 + 64); // emit masks: one word per chain and batch of sixteen steps
        b.etsum = a.get<uint32_t>((size_t)d.nch * emit_tiles_per_chunk(stride));
        b.fstate = a.get<uint32_t>((size_t)d.nch * 4);
        b.csize = a.get<uint32_t>(d.nch);
        b.stamp = a.get<uint64_t>(2 * (size_t)d.nch);
        b.hdr = a.get<uint8_t>((size_t)d.nch * HDR_MAX);
        b.hsize = a.get<uint32_t>(d.nch);
        b.outoff = a.get<uint64_t>(d.nch + 1);
    }
}

EncDims make_dims(uint32_t len, uint32_t chunk)
{
    EncDims d;
    d.len = len;
    d.chunk = chunk;
    d.nch = (len + chunk - 1) / chunk;
    d.tpc = (chunk + ATILE - 1) / ATILE;
    d.ncl = d.nch;
    d.cmap = nullptr;
    d.clen = nullptr;
    d.cblk = nullptr;
    d.bout = nullptr;
    d.sbase = nullptr;
    d.lbase = nullptr;
    return d;
}

// symbol changes per chunk: a cheap proxy for the length of its rANS chain (used to launch the densest chunks first)
__global__ __launch_bounds__(TB) void k_density(const uint8_t *__restrict__ in, EncDims d, uint32_t *__restrict__ dens)
{
    const uint32_t c = blockIdx.y, ts = blockIdx.x * ATILE * 4;
    const uint32_t clen = chunk_len(d, c);
    if (ts >= clen) return;
    const uint32_t te = (ts + ATILE * 4 < clen) ? ts + ATILE * 4 : clen;
    const uint8_t *src = in + (size_t)c * d.chunk;
    uint32_t n = 0;
    for (uint32_t i = ts + threadIdx.x * 16; i < te; i += TB * 16) {
        uint8_t prev = i ? src[i - 1] : 0;
        for (uint32_t k = 0; k < 16 && i + k < te; k++) { uint8_t v = src[i + k]; n += (v != prev); prev = v; }
    }
    n = wave_sum(n);
    if (lane_id() == 0 && n) atomicAdd(&dens[c], n);
}

// launch order of the chunks: densest first, ties by chunk number (rank by counting; one workgroup, nch <= a few thousand)
__global__ __launch_bounds__(256) void k_order(EncDims d, const uint32_t *__restrict__ dens, uint32_t *__restrict__ cmap)
{
    for (uint32_t c = threadIdx.x; c < d.nch; c += blockDim.x) {
        const uint32_t v = dens[c];
        uint32_t r = 0;
        for (uint32_t k = 0; k < d.nch; k++) {
            const uint32_t w = dens[k];
            r += (w > v || (w == v && k < c)) ? 1u : 0u;
        }
        cmap[r] = c;
    }
}

// Text carries ~0.42 RLE0 symbols per byte, the densest data 1.0: the arena is first sized for 0.55 and grows (the stage starts
// over) the first time a denser block arrives.
constexpr uint32_t ENC_PLAN_SYM_256 = 141;

// what the stage plans for `nch` chunks when the input has `sym_per_byte_256` / 256 RLE0 symbols per byte (256 = the worst case)
size_t enc_plan_bytes(const EncDims &d, int nblk, uint32_t sym_per_byte_256)
{
    EncBufs b;
    jpk_ctx dummy;
    Arena plan(&dummy, true);
    enc_layout(plan, d, b, LAY_RANK | LAY_RLE);
    plan.get<uint32_t>((size_t)d.nch + 1);
    plan.get<uint32_t>((size_t)d.nch + 1);
    if (nblk) { plan.get<uint32_t>(d.nch); plan.get<uint32_t>(d.nch); plan.get<uint8_t *>((size_t)nblk); }
    const size_t worst = (size_t)d.nch * d.chunk;
    size_t sym = worst / 256 * sym_per_byte_256 + 256 * (size_t)d.nch;
    if (sym > worst) sym = worst;
    enc_layout(plan, d, b, LAY_MODEL | LAY_RANS, sym, 2 * sym + 4 * 384 * (size_t)d.nch);
    return plan.need;
}

// tables a group of blocks hands in (host side): the core gives them device copies inside its own arena layout
struct GroupTabs { const uint32_t *clen, *cblk; uint8_t *const *bout; int nblk; };

// slots per chunk of the compact symbol layout (EncDims::sbase): its RLE0 symbol count rounded up to 256, prefix sums, totals -> mailbox
__global__ void k_sym_layout(EncDims d, const uint32_t *__restrict__ rlen, uint32_t *__restrict__ sbase, uint32_t *__restrict__ lbase, uint32_t *__restrict__ mail)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t so = 0, lo = 0;
    for (uint32_t c = 0; c < d.nch; c++) {
        sbase[c] = so; lbase[c] = lo;
        const uint32_t cs = (rlen[c] + 255u) & ~255u;
        so += cs;
        lo += 4u * (uint32_t)rans_lane_stride(cs);
    }
    sbase[d.nch] = so; lbase[d.nch] = lo;
    mail[MAIL_SYM_TOTAL] = so; mail[MAIL_LANE_TOTAL] = lo;
}

// ---- the host steps of encode_core -----------------------------------------------------------------------------------------------
// Front with retry: rank coding and RLE0 of every chunk, then the compact layout of everything that is indexed by RLE0 symbol.
// The symbol count of a chunk is known on the device only: one 8-byte read back (the stage's first host synchronisation) sizes
// the model / rANS buffers for what the block HAS -- ~33 bytes of arena per block byte on text instead of the 78 that "every
// byte a symbol" takes.  When the arena turns out too small it grows and the stage starts over (the first dense block of a
// context; jpk_ctx_reserve sizes for text).
int enc_front(jpk_ctx *ctx, const uint8_t *d_in, EncDims &d, EncBufs &b, const GroupTabs *gt)
{
    hipStream_t st = ctx->stream;
    JPK_TRY(jpk_arena_ensure(ctx, ctx->arena_base + enc_plan_bytes(d, gt ? gt->nblk : 0, ENC_PLAN_SYM_256)));
    for (int attempt = 0;; attempt++) {
        Arena real(ctx, false);
        enc_layout(real, d, b, LAY_RANK | LAY_RLE);
        uint32_t *sbase = real.get<uint32_t>((size_t)d.nch + 1), *lbase = real.get<uint32_t>((size_t)d.nch + 1);
        if (gt) {
            uint32_t *d_clen = real.get<uint32_t>(d.nch), *d_cblk = real.get<uint32_t>(d.nch);
            uint8_t **d_bout = real.get<uint8_t *>((size_t)gt->nblk);
            if (ctx->arena_off > ctx->arena_cap) return JPK_E_ALLOC;
            JPK_HIP(hipMemcpyAsync(d_clen, gt->clen, sizeof(uint32_t) * d.nch, hipMemcpyHostToDevice, st));
            JPK_HIP(hipMemcpyAsync(d_cblk, gt->cblk, sizeof(uint32_t) * d.nch, hipMemcpyHostToDevice, st));
            JPK_HIP(hipMemcpyAsync(d_bout, gt->bout, sizeof(uint8_t *) * (size_t)gt->nblk, hipMemcpyHostToDevice, st));
            d.clen = d_clen; d.cblk = d_cblk; d.bout = d_bout;
        }
        if (ctx->arena_off > ctx->arena_cap) return JPK_E_ALLOC;
        d.sbase = nullptr; d.lbase = nullptr;
        JPK_TRY(run_rank(ctx, d_in, d, b));
        JPK_TRY(run_rle(ctx, b.ranks, d, b));
        hipLaunchKernelGGL(k_sym_layout, dim3(1), dim3(64), 0, st, d, b.rlen, sbase, lbase, ctx->d_mail->read);
        uint32_t mail[MAIL_LAYOUT_WORDS];
        JPK_TRY(jpk_read_mail(ctx, mail, MAIL_LAYOUT_WORDS));
        const size_t sym_total = mail[MAIL_SYM_TOTAL], lane_total = mail[MAIL_LANE_TOTAL];
        Arena rest(ctx, true);
        EncBufs dummy = b;
        enc_layout(rest, d, dummy, LAY_MODEL | LAY_RANS, sym_total ? sym_total : 256, lane_total ? lane_total : 512);
        if (ctx->arena_off + rest.need > ctx->arena_cap) {
            if (attempt) return JPK_E_ALLOC;
            JPK_TRY(jpk_arena_ensure(ctx, ctx->arena_off + rest.need));      // frees and re-allocates: the buffers above are gone
            continue;
        }
        enc_layout(real, d, b, LAY_MODEL | LAY_RANS, sym_total ? sym_total : 256, lane_total ? lane_total : 512);
        d.sbase = sbase; d.lbase = lbase;
        break;
    }
    return JPK_OK;
}

// Launch-group decision: into how many groups, each on a stream of its own, the chunks are cut.
// Graded launch groups shorten ONE block (its longest chains start after a sixteenth of the parallel work) but cost throughput
// when other blocks fill the machine anyway (more kernels, more streams on the hardware queues): 4 groups alone, 2 beside one
// other block, 1 beside two or more (default bench, 4 blocks in flight: 3.23 / 3.32 / 3.46 GB/s with 4 / 2 / 1 groups).
// Group streams are created when a block first needs them and then stay with the context (parked while the device is busy
// with other blocks: an idle stream costs nothing, destroying and re-creating it under fluctuating load costs a synchronise)
int enc_launch_groups(jpk_ctx *ctx, int inflight_n, uint32_t nch)
{
    int ngroups = jpk_enc_groups_for(inflight_n, nch);
    static const long groups_env = jpk_env_long("JPK_ENC_GROUPS", 0);
    if (groups_env >= 1 && groups_env <= jpk_ctx::ENC_GROUPS && (uint32_t)groups_env <= nch) ngroups = groups_env;
    for (int g = 0; g + 1 < ngroups; g++)
        if (!ctx->aux[g] && hipStreamCreateWithFlags(&ctx->aux[g], hipStreamNonBlocking) != hipSuccess) { ctx->aux[g] = nullptr; ngroups = g + 1; break; }
    return ngroups;
}

// Graded groups (ngroups >= 2).
// The stage is bounded by the longest rANS chain (the densest chunk), a single wave, and several of the parallel
// kernels in front of it are latency-bound per chunk as well.  The chunks are ordered by a density estimate and cut
// into up to four groups, densest first, and each group runs the whole stage on its own stream: the densest
// chains start after a quarter of the parallel work, beside the parallel stages of the other groups.
int enc_graded_groups(jpk_ctx *ctx, const uint8_t *d_in, const EncDims &d, EncBufs &b, int ngroups)
{
    hipStream_t st = ctx->stream;
    // launch order on the device (no host round trip): density per chunk, rank by counting
    JPK_HIP(hipMemsetAsync(b.dens, 0, (size_t)d.nch * 4, st));
    JPK_LAUNCH(ctx, PROF_ENC_HIST, d.len, k_density, dim3((d.chunk + ATILE * 4 - 1) / (ATILE * 4), d.nch), dim3(TB), d_in, d, b.dens);
    JPK_LAUNCH(ctx, PROF_ENC_HIST, 0, k_order, dim3(1), dim3(256), d, b.dens, b.cmap);
    JPK_HIP(hipEventRecord(ctx->ev_pre[0], st));           // histogram memset + chunk order are in place
    // graded groups, densest first: the first group is small so that the longest chains -- the serial floor of the whole
    // stage -- start after a sixteenth of the parallel work; with four groups: 1/16, 1/8, 1/4 of the chunks and the rest
    uint32_t gsz[jpk_ctx::ENC_GROUPS];
    {
        uint32_t left = d.nch;
        for (int g = 0; g < ngroups; g++) {
            uint32_t n = (g + 1 == ngroups) ? left : d.nch >> (ngroups - g);
            if (n < 2) n = 2;
            if (n > left) n = left;
            gsz[g] = n;
            left -= n;
        }
    }
    uint32_t off = 0;
    int rc = JPK_OK;
    for (int g = 0; g < ngroups && rc == JPK_OK; g++) {
        const uint32_t n = gsz[g];
        if (n == 0) continue;
        EncDims gd = d;
        gd.ncl = n; gd.cmap = b.cmap + off;
        off += n;
        // every buffer of the stage is indexed by chunk, so the groups are independent: each runs on its own stream
        hipStream_t gs = (g + 1 < ngroups) ? ctx->aux[g] : st;
        if (gs != st && hipStreamWaitEvent(gs, ctx->ev_pre[0], 0) != hipSuccess) { rc = JPK_E_DEVICE; break; }
        ctx->stream = gs;
        rc = run_model(ctx, b.rle, b.rlen, gd, b);
        if (rc == JPK_OK) rc = run_pairs(ctx, b.rle, b.rlen, gd, b);
        if (rc == JPK_OK) rc = run_chain(ctx, gd, b);
        if (rc == JPK_OK) rc = run_emit_counts(ctx, gd, b);
        ctx->stream = st;
        if (rc == JPK_OK && gs != st && hipEventRecord(ctx->ev_done[g], gs) != hipSuccess) rc = JPK_E_DEVICE;
    }
    for (int g = 0; g + 1 < ngroups && rc == JPK_OK; g++)
        if (hipStreamWaitEvent(st, ctx->ev_done[g], 0) != hipSuccess) rc = JPK_E_DEVICE;
    if (rc != JPK_OK) {
        // groups already launched keep reading and writing the arena: join them before the caller may reuse it
        for (int g = 0; g + 1 < jpk_ctx::ENC_GROUPS; g++) if (ctx->aux[g]) (void)hipStreamSynchronize(ctx->aux[g]);
        (void)hipStreamSynchronize(st);
    }
    return rc;
}

// One group.  The chain -- one wave per chunk, milliseconds long -- goes to a high-priority stream of the device's chain pool
// (chain_pool.hpp), whose hardware queues are not the ones the wide kernels of the other blocks wait in.  The two streams are
// ordered through the HOST, which is blocked in this call anyway: a hipStreamWaitEvent would put a barrier into the waiting
// stream's hardware queue and stall the streams that share it, which is what the pool is there to avoid.  No pool
// (JPK_CHAIN_STREAMS=0, no stream priorities): everything on the context's stream, as before.
int enc_single_group(jpk_ctx *ctx, const EncDims &d, EncBufs &b)
{
    hipStream_t st = ctx->stream;
    JPK_TRY(run_model(ctx, b.rle, b.rlen, d, b));
    JPK_TRY(run_pairs(ctx, b.rle, b.rlen, d, b));
    JpkChainLease lease(ctx);      // an early return below synchronises the pool stream and gives it back (~JpkChainLease)
    if (lease.held()) {
        JPK_HIP(hipEventRecord(ctx->ev_pre[0], st));
        JPK_HIP(hipEventSynchronize(ctx->ev_pre[0]));               // the model pass is done: the chain's input is in place
        ctx->stream = lease.stream;                                 // (the profiler's events follow the launch)
        const int rc = run_chain(ctx, d, b);
        ctx->stream = st;
        JPK_TRY(rc);
        JPK_HIP(hipGetLastError());
        JPK_HIP(hipEventRecord(ctx->ev_done[0], lease.stream));
        JPK_HIP(hipEventSynchronize(ctx->ev_done[0]));              // the chain is done: the pool stream goes back idle
        lease.done();
    } else {
        JPK_TRY(run_chain(ctx, d, b));
    }
    JPK_TRY(run_emit_counts(ctx, d, b));
    return JPK_OK;
}

// everything of the stage up to the chunks' output offsets, enqueued on ctx->stream (and the group streams): rank coding, RLE0,
// models, the rANS chains, emit counts, headers, offsets.  `d` describes the chunks (one block: make_dims; a group of blocks: the
// per-chunk tables), `inflight_n` the blocks the device is compressing right now (drives the launch grouping).
int encode_core(jpk_ctx *ctx, const uint8_t *d_in, EncDims &d, EncBufs &b, int inflight_n, const GroupTabs *gt = nullptr)
{
    JPK_TRY(enc_front(ctx, d_in, d, b, gt));
    // (clearing the histograms inside k_cls_count instead of a memset of its own: k_cls_ord 64 -> 85 us per launch, round 6 -- not kept)
    JPK_HIP(hipMemsetAsync(b.qhist, 0, (size_t)d.nch * 6 * NQ * QSTRIDE * 4, ctx->stream));
    const int ngroups = enc_launch_groups(ctx, inflight_n, d.nch);
    if (ngroups >= 2) JPK_TRY(enc_graded_groups(ctx, d_in, d, b, ngroups));
    else JPK_TRY(enc_single_group(ctx, d, b));
    return run_offsets(ctx, d, b);
}
}  // namespace

// arena bytes of one Ans::Encode of len bytes of text-like data (jpk_ctx_reserve)
size_t jpk_ans_encode_arena_bytes(uint32_t len)
{
    if (len == 0) return 0;
    const EncDims d = make_dims(len, ANS_CHUNK);
    return enc_plan_bytes(d, 0, ENC_PLAN_SYM_256);
}
// the same for the densest input there is (every byte an RLE0 symbol): what the arena grows to when such a block arrives
size_t jpk_ans_encode_arena_bytes_worst(uint32_t len)
{
    if (len == 0) return 0;
    const EncDims d = make_dims(len, ANS_CHUNK);
    return enc_plan_bytes(d, 0, 256);
}

int jpk_ans_encode_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out, int32_t out_cap, int32_t *out_len)
{
    const JpkCompressInflight inflight(ctx->device);      // blocks of this device in their forward BWT or entropy encode right now, this one included
    *out_len = 0;
    ctx->stats.ans_chunks = 0;
    ctx->stats.ans_rle_symbols = 0;
    if (len == 0) return JPK_OK;
    hipStream_t st = ctx->stream;
    EncDims d = make_dims((uint32_t)len, ANS_CHUNK);
    EncBufs b;
    memset(&b, 0, sizeof b);
    JPK_TRY(encode_core(ctx, d_in, d, b, inflight.n));
    uint32_t mail[MAIL_OFFSETS_WORDS];
    JPK_TRY(jpk_read_mail(ctx, mail, MAIL_OFFSETS_WORDS));
    ctx->stats.enc_chain_cycles = (int64_t)mail_u64(mail, MAIL_CHAIN_CYCLES);
    ctx->stats.enc_chain_ns = (int64_t)mail_u64(mail, MAIL_CHAIN_TICKS) * 10;     // s_memrealtime ticks at 100 MHz
    ctx->stats.enc_chain_steps = ((int64_t)mail[MAIL_CHAIN_RLEN] * 2 + 3) / 4;
    const uint64_t total = mail_u64(mail, MAIL_TOTAL);
    ctx->stats.ans_chunks = d.nch;
    ctx->stats.ans_rle_symbols = (int64_t)mail_u64(mail, MAIL_RLE_SYMBOLS);
    if (ctx->prof_on) {    // symbol-based kernels: units are only known now (RLE0 symbols / rANS pairs of this call)
        const uint64_t rs = (uint64_t)ctx->stats.ans_rle_symbols;
        ctx->prof_units[PROF_ENC_CLASS] += rs;
        ctx->prof_units[PROF_ENC_ADAPTIVE] += rs;
        ctx->prof_units[PROF_ENC_PAIRS] += rs;
        ctx->prof_units[PROF_ENC_RANS] += 2 * rs;
        ctx->prof_units[PROF_ENC_EMIT] += 2 * rs;
    }
    if (total > (uint64_t)out_cap) return JPK_E_CAPACITY;
    JPK_TRY(run_put(ctx, d, b, d_out));
    JPK_HIP(hipStreamSynchronize(st));
    *out_len = (int32_t)total;
    return JPK_OK;
}

// ---- group encode: the images of several (small) blocks through ONE set of grids ---------------------------------------------
// Chunks are independent (ans.cpp:136-140), so the chunks of all blocks of a group run through the same launches; a block's image
// starts at a chunk boundary of the staging buffer `d_stage` (block b at first_chunk[b] * 1 MiB), every chunk knows its length, its
// block and, through the block, its output buffer; offsets restart at every block.  Host synchronisations per group: the symbol layout (encode_core), the chunk sizes, the end of
// the emit kernels, and one more when a block does not fit its buffer.
size_t jpk_ans_encode_group_arena_bytes(uint32_t nchunks, int nblk)
{
    const EncDims d = make_dims(nchunks * ANS_CHUNK, ANS_CHUNK);
    return enc_plan_bytes(d, nblk, ENC_PLAN_SYM_256);
}

// The arena (from ctx->arena_base on) must hold jpk_ans_encode_group_arena_bytes(); the caller has sized it.
int jpk_ans_encode_group_device(jpk_ctx *ctx, int nblk, const uint8_t *d_stage, const uint32_t *first_chunk, const int32_t *mid_len, uint8_t *const *d_out,
                                const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    const JpkCompressInflight inflight(ctx->device);
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> clen, cblk;
    for (int b = 0; b < nblk; b++) {
        out_len[b] = 0;
        status[b] = JPK_OK;
        const uint32_t ml = (uint32_t)mid_len[b], nc = (ml + ANS_CHUNK - 1) / ANS_CHUNK;
        if (clen.size() != first_chunk[b]) return JPK_E_ARG;                   // images are laid out back to back, in block order
        for (uint32_t k = 0; k < nc; k++) {
            clen.push_back(k + 1 < nc ? (uint32_t)ANS_CHUNK : ml - k * (uint32_t)ANS_CHUNK);
            cblk.push_back((uint32_t)b);
        }
    }
    const uint32_t nch = (uint32_t)clen.size();
    if (nch == 0) return JPK_OK;
    EncDims d = make_dims(nch * ANS_CHUNK, ANS_CHUNK);
    EncBufs b;
    memset(&b, 0, sizeof b);
    const GroupTabs gt = {clen.data(), cblk.data(), d_out, nblk};     // (host vectors: they outlive the synchronisations below)
    JPK_TRY(encode_core(ctx, d_stage, d, b, inflight.n, &gt));
    uint8_t **d_bout = const_cast<uint8_t **>(d.bout);
    // sizes: header + payload of every chunk; one copy, the group's only host synchronisation before the payload is placed
    std::vector<uint32_t> hs(nch), cs(nch);
    JPK_HIP(hipMemcpyAsync(hs.data(), b.hsize, sizeof(uint32_t) * nch, hipMemcpyDeviceToHost, st));
    JPK_HIP(hipMemcpyAsync(cs.data(), b.csize, sizeof(uint32_t) * nch, hipMemcpyDeviceToHost, st));
    JPK_HIP(hipStreamSynchronize(st));
    std::vector<uint64_t> tot((size_t)nblk, 0);
    for (uint32_t c = 0; c < nch; c++) tot[cblk[c]] += (uint64_t)hs[c] + cs[c];
    bool all_fit = true;
    for (int k = 0; k < nblk; k++)
        if (tot[k] > (uint64_t)out_cap[k]) { status[k] = JPK_E_CAPACITY; all_fit = false; }
    if (!all_fit) {
        // a block that does not fit its buffer is not written at all: its entry of the output table becomes null and the two emit
        // kernels skip its chunks; the blocks that fit are emitted as usual (no scratch sink, no whole-group failure)
        std::vector<uint8_t *> outs(d_out, d_out + nblk);
        for (int k = 0; k < nblk; k++) if (status[k] != JPK_OK) outs[k] = nullptr;
        JPK_HIP(hipMemcpyAsync(d_bout, outs.data(), sizeof(uint8_t *) * (size_t)nblk, hipMemcpyHostToDevice, st));
        JPK_HIP(hipStreamSynchronize(st));                                     // (`outs` is a local: the copy must have read it)
    }
    JPK_TRY(run_put(ctx, d, b, nullptr));
    JPK_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < nblk; k++) if (status[k] == JPK_OK) out_len[k] = (int32_t)tot[k];
    ctx->stats.ans_chunks = (int32_t)nch;
    return JPK_OK;
}

// Postcoder::Encode (rank.cpp:45-90) for one buffer of any length, in place
int jpk_rank_encode_device(jpk_ctx *ctx, uint8_t *d_t, int32_t *d_freq, int32_t len)
{
    if (len == 0) {
        JPK_HIP(hipMemsetAsync(d_freq, 0, 256 * 4, ctx->stream));
        return JPK_OK;
    }
    const EncDims d = make_dims((uint32_t)len, (uint32_t)len);
    EncBufs b;
    Arena plan(ctx, true);
    enc_layout(plan, d, b, LAY_RANK);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    enc_layout(real, d, b, LAY_RANK);
    JPK_TRY(run_rank(ctx, d_t, d, b));
    JPK_HIP(hipMemcpyAsync(d_t, b.ranks, (size_t)len, hipMemcpyDeviceToDevice, ctx->stream));
    JPK_HIP(hipMemcpyAsync(d_freq, b.freq, 256 * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return JPK_OK;
}

// RLE::encode (rle.cpp:22-47) of one chunk
int jpk_rle_encode_device(jpk_ctx *ctx, const uint8_t *d_ranks, int32_t len, uint16_t *d_rle, int32_t *rlen)
{
    *rlen = 0;
    if (len == 0) return JPK_OK;
    const EncDims d = make_dims((uint32_t)len, (uint32_t)len);
    EncBufs b;
    Arena plan(ctx, true);
    enc_layout(plan, d, b, LAY_RLE);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    enc_layout(real, d, b, LAY_RLE);
    JPK_TRY(run_rle(ctx, d_ranks, d, b));
    JPK_HIP(hipMemcpyAsync(ctx->d_mail->read, b.rlen, 4, hipMemcpyDeviceToDevice, ctx->stream));
    uint32_t n = 0;
    JPK_TRY(jpk_read_mail(ctx, &n, 1));
    JPK_HIP(hipMemcpyAsync(d_rle, b.rle, (size_t)n * 2, hipMemcpyDeviceToDevice, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    *rlen = (int32_t)n;
    return JPK_OK;
}

// model pass of one chunk: rle symbols -> packed pairs
int jpk_model_pairs_device(jpk_ctx *ctx, const uint16_t *d_rle, int32_t rlen, uint32_t *d_pairs)
{
    if (rlen == 0) return JPK_OK;
    const EncDims d = make_dims((uint32_t)rlen, (uint32_t)rlen);
    EncBufs b;
    Arena plan(ctx, true);
    enc_layout(plan, d, b, LAY_RLE | LAY_MODEL | LAY_PLAIN);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    enc_layout(real, d, b, LAY_RLE | LAY_MODEL | LAY_PLAIN);
    uint32_t n = (uint32_t)rlen;
    JPK_HIP(hipMemcpyAsync(b.rlen, &n, 4, hipMemcpyHostToDevice, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    JPK_HIP(hipMemsetAsync(b.qhist, 0, (size_t)d.nch * 6 * NQ * QSTRIDE * 4, ctx->stream));
    JPK_TRY(run_model(ctx, d_rle, b.rlen, d, b));
    JPK_TRY(run_pairs(ctx, d_rle, b.rlen, d, b));
    JPK_HIP(hipMemcpyAsync(d_pairs, b.pairs, (size_t)rlen * 8, hipMemcpyDeviceToDevice, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    return JPK_OK;
}
