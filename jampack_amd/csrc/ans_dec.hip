// ans_dec.hip -- Ans::Decode (ans.cpp:236-270) on gfx950.
//   header walk (ans.cpp:254-261, ReadHeader :287-302)           one wave per block (terminator ballot), chunk chain serial by format
//   rANS + model decode (Threaded_Decode, ans.cpp:30-92)          one wave per chunk; lanes = CDF entries
//   RLE0 decode (rle.cpp:52-74)                                   one workgroup per chunk, scan based
//   sorted-rank decode (rank.cpp:96-151)                          one wave per chunk; list positions 0..63 one per lane,
//                                                                 64..255 packed four to a lane
// Batches of blocks run ONE grid per serial kernel over the chunks of all blocks (longest chains first beyond 1024).
// The entropy decoder is sequential inside a chunk by construction of the format (shared byte pointer of the
// four rANS states, adaptive models, bucket hopping of the rank decoder); parallelism comes from the chunks.
//
// Units (ans_dec.hpp is what they share; every kernel is defined in one unit, in its anonymous namespace, and launched only from it):
//   ans_dec_rans.hip    the rANS + model chains (k_dec_rans: run_rans), with the issue costs they are scheduled for
//   ans_dec_rank.hip    RLE0 decode (k_dec_rle: run_rle) and the sorted-rank chains (k_dec_rank: run_rank)
//   ans_dec.hip         the header walk (k_dec_headers), the launch order of a large batch (k_dec_order), the host steps of the batch
//                       and the jpk_* entries
// What each step of jpk_ans_decode_batch hands the next:
//   dec_count_pass         the blocks' streams -> MAIL_* words per block (k_dec_headers<false>; synchronises)
//   dec_plan               the mail -> chunks and sizes per block, DecBlock::cbase, the totals
//   dec_layout             the plan -> DecBufs and the blocks' rle / ranks arrays, all in the arena
//   dec_upload_and_clear   the block table goes up; status words and rank arrays start as zeros
//   dec_fill_and_order     the streams -> info, freq (k_dec_headers<true>); info -> order (k_dec_order, large batches only)
//   run_rans               payload -> rle;  run_rle: rle -> ranks;  run_rank: ranks, freq -> the blocks' outputs
//   dec_collect            status words -> status[b], out_len[b] (synchronises)
#include <vector>

#include "ans_dec.hpp"

using namespace jpk;
using namespace jpk_dec;

namespace {

// One wave.  The chunk chain is serial by format (chunk c+1 starts behind chunk c's payload, ans.cpp:254-261), but a header is
// not: it is 259 LEB128 values (256 frequencies, olen, clen, rlen; ReadHeader ans.cpp:287-302) and every value ENDS in the one
// byte with bit 7 set (utils.cpp:70-90).  The wave walks a header 64 bytes at a time: one ballot marks the terminators, their
// running count numbers the values, and the lane that holds a terminator decodes that value from the up to four bytes in
// front of it.
// One wave per block.  WRITE = false: count the chunks and total the sizes only (mail); WRITE = true: also fill info / freq at
// the block's global chunk base.  mail of block b: mail[MAIL_STRIDE b + ...], the MAIL_* words of ans_dec.hpp.
template <bool WRITE>
__global__ __launch_bounds__(64) void k_dec_headers(const DecBlock *__restrict__ blocks, ChunkInfo *__restrict__ info_all, int32_t *__restrict__ freq_all,
                                                   uint32_t *__restrict__ mail_all)
{
    const DecBlock B = blocks[blockIdx.x];
    const uint8_t *__restrict__ in = B.in;
    const uint32_t len = (uint32_t)B.in_len, max_chunks = B.max_chunks;
    const uint64_t out_cap = B.out_cap;
    ChunkInfo *info = WRITE ? info_all + B.cbase : nullptr;
    int32_t *freq = WRITE ? freq_all + (size_t)B.cbase * 256 : nullptr;
    uint32_t *mail = mail_all + MAIL_STRIDE * blockIdx.x;
    const int l = lane_id();
    uint64_t ip = 0, op = 0, rp = 0;
    uint32_t nch = 0;
    int status = 0;
    while (ip < len && status == 0) {
        if (nch >= max_chunks) { status = JPK_E_CORRUPT; break; }
        uint32_t nval = 0;                       // values decoded so far (wave-uniform)
        uint64_t pos = ip;                       // first byte of the current 64-byte window
        uint32_t olen = 0, clen = 0, rlen = 0;
        uint32_t fsum = 0;                       // per-lane partial sum of the frequencies
        bool bad = false;
        uint32_t since = 0;                      // bytes since the last terminator at the start of the window (a value has <= 5 bytes)
        while (nval < 259u) {
            if (pos >= len) { bad = true; break; }
            const uint64_t p = pos + (uint64_t)l;
            const uint32_t byte = (p < len) ? in[p] : 0u;
            const uint64_t term = __ballot(p < len && (byte & 0x80u));
            const uint32_t before = (uint32_t)__popcll(term & ((1ull << l) - 1ull));
            const uint32_t vidx = nval + before;                         // index of the value that ends at my byte
            if (((term >> l) & 1ull) && vidx < 259u) {
                // bytes of my value: from the byte after the previous terminator to me (at most 5)
                const uint64_t prevmask = term & ((1ull << l) - 1ull);
                const uint32_t nlead = prevmask ? (uint32_t)l - (63u - (uint32_t)__clzll((long long)prevmask)) - 1u : (uint32_t)l + since;
                if (nlead > 4u) bad = true;
                else {
                    uint32_t x = 0;
                    for (uint32_t k = nlead; k > 0; k--) x = (x << 7) | in[p - k];
                    x = (x << 7) | (byte & 0x7fu);
                    if (nlead > 0) x += pre::LEB_OFF[nlead - 1];
                    if (vidx < 256u) {
                        if (x > (uint32_t)ANS_CHUNK) bad = true;
                        if (WRITE) freq[(size_t)nch * 256 + vidx] = (int32_t)x;
                        fsum += x;
                    } else if (vidx == 256u) olen = x;
                    else if (vidx == 257u) clen = x;
                    else rlen = x;
                }
            }
            const uint32_t nt = (uint32_t)__popcll(term);
            if (nval + nt >= 259u) {
                // the header ends at the terminator of value 258: position of the (259 - nval)-th terminator of this window
                uint64_t t = term;
                for (uint32_t k = 259u - nval - 1u; k > 0; k--) t &= t - 1ull;
                pos += (uint64_t)__builtin_ctzll(t) + 1ull;
                nval = 259u;
            } else {
                since = nt ? (uint32_t)__clzll((long long)term) : since + 64u;      // continuation bytes behind the window's last terminator
                if (since > 4u) { bad = true; break; }            // a value has at most four of them
                nval += nt;
                pos += 64;
            }
        }
        bad = __ballot(bad) != 0ull;
        // the three length fields were decoded by whichever lanes held their terminators
        olen = wave_sum(olen); clen = wave_sum(clen); rlen = wave_sum(rlen);
        const uint64_t total = (uint64_t)wave_sum(fsum);
        ip = pos;
        // rlen > olen: RLE0 never emits more symbols than bytes (a run of k binary digits stands for >= k zeros, every other symbol
        // for one byte), so RLE::decode would end in "rle mismatch!" (rle.cpp:73) -- and the buffers below are sized by olen
        if (bad || olen > (uint32_t)ANS_CHUNK || rlen > olen || ip > len || (uint64_t)clen > len - ip || clen < 16 ||
            total != (uint64_t)olen) {                                       // ans.cpp:297-298, rank.cpp:104-108
            status = JPK_E_CORRUPT;
            break;
        }
        if (op + olen > out_cap) { status = JPK_E_CAPACITY; break; }
        if (WRITE && l == 0) {
            ChunkInfo ci;
            ci.in_off = ip; ci.clen = clen; ci.olen = olen; ci.rlen = rlen; ci.blk = blockIdx.x; ci.out_off = op; ci.rle_off = rp;
            info[nch] = ci;
        }
        ip += clen; op += olen; rp += rlen;
        nch++;
    }
    if (l == 0) {
        mail[MAIL_STATUS] = (uint32_t)status;
        mail[MAIL_CHUNKS] = nch;
        mail[MAIL_OUT_TOTAL] = (uint32_t)op; mail[MAIL_OUT_TOTAL + 1] = (uint32_t)(op >> 32);
        mail[MAIL_RLE_TOTAL] = (uint32_t)rp; mail[MAIL_RLE_TOTAL + 1] = (uint32_t)(rp >> 32);
    }
}

// Launch order of the chains of a large batch: longest first (by RLE0 symbols, what both serial kernels' time follows), so that
// the chains that set the length of the stage are not the ones that had to wait for a free slot.  One pass of counting: 4096
// buckets of 256 symbols, longest bucket first; the order inside a bucket is arrival order (any order is a valid launch order:
// it only decides which chain starts first, never a byte).  One workgroup, any number of chunks.
constexpr int ORD_BUCKETS = 4096, ORD_TB = 1024;
__global__ __launch_bounds__(ORD_TB) void k_dec_order(const ChunkInfo *__restrict__ info, uint32_t n, uint32_t *__restrict__ order)
{
    __shared__ uint32_t h[ORD_BUCKETS];
    __shared__ uint32_t sm[ORD_TB / 64 + 1];
    for (int i = threadIdx.x; i < ORD_BUCKETS; i += ORD_TB) h[i] = 0;
    __syncthreads();
    auto bucket = [](uint32_t rlen) { const uint32_t b = rlen >> 8; return (uint32_t)(ORD_BUCKETS - 1) - (b < (uint32_t)ORD_BUCKETS ? b : (uint32_t)(ORD_BUCKETS - 1)); };
    for (uint32_t t = threadIdx.x; t < n; t += ORD_TB) atomicAdd(&h[bucket(info[t].rlen)], 1u);
    __syncthreads();
    // exclusive scan of the bucket counts, four consecutive buckets per thread
    uint32_t v[ORD_BUCKETS / ORD_TB], acc = 0;
#pragma unroll
    for (int k = 0; k < ORD_BUCKETS / ORD_TB; k++) { v[k] = h[threadIdx.x * (ORD_BUCKETS / ORD_TB) + k]; acc += v[k]; }
    const uint32_t inc = block_incl_scan<OpSum>(acc, sm, nullptr);
    uint32_t run = inc - acc;
#pragma unroll
    for (int k = 0; k < ORD_BUCKETS / ORD_TB; k++) { h[threadIdx.x * (ORD_BUCKETS / ORD_TB) + k] = run; run += v[k]; }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < n; t += ORD_TB) order[atomicAdd(&h[bucket(info[t].rlen)], 1u)] = t;
}

// ---- the host steps of the batch ----------------------------------------------------------------------------------------------

// The one place that knows where the block table and the mail of a batch sit: at the head of the arena, behind arena_skip.  `end` is the
// first arena byte behind them; the pointers hold once the arena has been ensured to `end` or beyond, and until it next grows (an
// ensure may move it: call again).
struct DecHead { size_t end; DecBlock *tab; uint32_t *mail; };
DecHead dec_head(const jpk_ctx *ctx, int nblk, size_t arena_skip)
{
    const size_t tab_bytes = jpk_align((size_t)nblk * sizeof(DecBlock) + 64), mail_bytes = jpk_align((size_t)nblk * MAIL_STRIDE * 4 + 64);
    DecHead h;
    h.end = arena_skip + tab_bytes + mail_bytes;
    h.tab = ctx->arena ? reinterpret_cast<DecBlock *>(ctx->arena + arena_skip) : nullptr;
    h.mail = ctx->arena ? reinterpret_cast<uint32_t *>(ctx->arena + arena_skip + tab_bytes) : nullptr;
    return h;
}

// pass 1 of the batch: the block table goes to the head of the arena (behind arena_skip), one k_dec_headers<false> wave per block
// counts the chunks and totals the sizes; mail[MAIL_STRIDE b ..] comes back to the host (synchronises the stream)
int dec_count_pass(jpk_ctx *ctx, const std::vector<DecBlock> &hb, size_t arena_skip, std::vector<uint32_t> &mail)
{
    const int nblk = (int)hb.size();
    hipStream_t st = ctx->stream;
    const size_t need = dec_head(ctx, nblk, arena_skip).end + 4096;
    if (arena_skip && !jpk_arena_fits(ctx, need)) return JPK_E_ALLOC;
    JPK_TRY(jpk_arena_ensure(ctx, need));
    const DecHead head = dec_head(ctx, nblk, arena_skip);
    JPK_HIP(hipMemcpyAsync(head.tab, hb.data(), (size_t)nblk * sizeof(DecBlock), hipMemcpyHostToDevice, st));
    JPK_LAUNCH(ctx, PROF_DEC_HEADERS, 0, (k_dec_headers<false>), dim3(nblk), dim3(64), head.tab, (ChunkInfo *)nullptr, (int32_t *)nullptr, head.mail);
    JPK_HIP(hipGetLastError());
    mail.assign((size_t)nblk * MAIL_STRIDE, 0u);
    JPK_HIP(hipMemcpyAsync(mail.data(), head.mail, mail.size() * 4, hipMemcpyDeviceToHost, st));
    JPK_HIP(hipStreamSynchronize(st));
    if (ctx->prof_on) jpk_prof_resolve(ctx);
    return JPK_OK;
}

DecBlock dec_block(const uint8_t *in, int32_t in_len, uint64_t out_cap)
{
    DecBlock b;
    memset(&b, 0, sizeof(DecBlock));
    b.in = in;
    b.in_len = in_len;
    b.out_cap = out_cap;
    b.max_chunks = (uint32_t)in_len / 275u + 2u;      // a chunk is >= 259 header bytes + 16 state bytes
    return b;
}

// what pass 1 found: decoded bytes and RLE0 symbols per block (0 for a block whose walk failed), and the totals over the batch
struct DecPlan {
    std::vector<uint64_t> blk_out, blk_rle;
    uint64_t chunks = 0, rle = 0, out = 0;
};
// mail -> plan.  A block whose walk failed gets its status here and takes no further part (in_len = 0: pass 2 finds no chunk in it);
// every other block gets its first global chunk index and, as max_chunks, one more than the chunks it has.
DecPlan dec_plan(const std::vector<uint32_t> &mail, std::vector<DecBlock> &hb, int32_t *status)
{
    const int nblk = (int)hb.size();
    DecPlan p;
    p.blk_out.assign((size_t)nblk, 0);
    p.blk_rle.assign((size_t)nblk, 0);
    for (int b = 0; b < nblk; b++) {
        const uint32_t *m = &mail[(size_t)b * MAIL_STRIDE];
        hb[b].cbase = (uint32_t)p.chunks;
        if ((int32_t)m[MAIL_STATUS] != 0) { status[b] = (int32_t)m[MAIL_STATUS]; hb[b].in_len = 0; continue; }
        p.blk_out[b] = mail_u64(m, MAIL_OUT_TOTAL);
        p.blk_rle[b] = mail_u64(m, MAIL_RLE_TOTAL);
        hb[b].max_chunks = m[MAIL_CHUNKS] + 1u;
        p.chunks += m[MAIL_CHUNKS];
        p.rle += p.blk_rle[b];
        p.out += p.blk_out[b];
    }
    return p;
}

// buffers behind the head: status, chunk table, frequencies, order; per block the packed RLE0 symbols and the rank array.  Fills `bufs`
// and the blocks' rle / ranks pointers; layout_end: the first arena byte behind the last block's rank array.
int dec_layout(jpk_ctx *ctx, size_t arena_skip, const DecPlan &plan, std::vector<DecBlock> &hb, DecBufs &bufs, size_t &layout_end)
{
    const int nblk = (int)hb.size();
    size_t off = dec_head(ctx, nblk, arena_skip).end;
    auto take = [&](size_t bytes) { size_t o = off; off += jpk_align(bytes + 64); return o; };
    const size_t o_status = take((size_t)nblk * 4), o_info = take((size_t)plan.chunks * sizeof(ChunkInfo)), o_freq = take((size_t)plan.chunks * 256 * 4);
    const size_t o_order = take((size_t)plan.chunks * 4);
    std::vector<size_t> o_rle((size_t)nblk), o_ranks((size_t)nblk);
    for (int b = 0; b < nblk; b++) { o_rle[b] = take(plan.blk_rle[b] * 2); o_ranks[b] = take(plan.blk_out[b]); }
    // A caller that keeps buffers of its own at the start of the arena (arena_skip != 0) has sized it for the worst case of the
    // streams' declared sizes; an arena that would have to grow -- and therefore move -- under those buffers is refused.
    if (arena_skip && !jpk_arena_fits(ctx, off + 4096)) return JPK_E_ALLOC;
    JPK_TRY(jpk_arena_ensure(ctx, off + 4096));            // may move the arena: every pointer is formed below
    const DecHead head = dec_head(ctx, nblk, arena_skip);
    bufs.tab = head.tab;
    bufs.mail = head.mail;
    bufs.status = reinterpret_cast<uint32_t *>(ctx->arena + o_status);
    bufs.info = reinterpret_cast<ChunkInfo *>(ctx->arena + o_info);
    bufs.freq = reinterpret_cast<int32_t *>(ctx->arena + o_freq);
    bufs.order = reinterpret_cast<uint32_t *>(ctx->arena + o_order);
    for (int b = 0; b < nblk; b++) {
        hb[b].rle = reinterpret_cast<uint16_t *>(ctx->arena + o_rle[b]);
        hb[b].ranks = ctx->arena + o_ranks[b];
    }
    layout_end = off;
    return JPK_OK;
}

int dec_upload_and_clear(jpk_ctx *ctx, const std::vector<DecBlock> &hb, const DecBufs &bufs, size_t layout_end)
{
    hipStream_t st = ctx->stream;
    JPK_HIP(hipMemcpyAsync(bufs.tab, hb.data(), hb.size() * sizeof(DecBlock), hipMemcpyHostToDevice, st));
    JPK_HIP(hipMemsetAsync(bufs.status, 0, hb.size() * 4, st));
    // the rank arrays start as zeros: RLE0 decode writes only the non-zero ranks (k_dec_rle); they are contiguous in the arena
    // (one memset from the first block's to the end of the layout)
    JPK_HIP(hipMemsetAsync(hb[0].ranks, 0, (size_t)(ctx->arena + layout_end - hb[0].ranks), st));
    return JPK_OK;
}

// pass 2 fills the chunk table and the frequencies; more chains than run at once are launched longest first.  Returns the order the
// serial kernels take (null: chunk order).
const uint32_t *dec_fill_and_order(jpk_ctx *ctx, int nblk, unsigned g, const DecBufs &bufs)
{
    JPK_LAUNCH(ctx, PROF_DEC_HEADERS, 0, (k_dec_headers<true>), dim3(nblk), dim3(64), bufs.tab, bufs.info, bufs.freq, bufs.mail);
    if (g <= DEC_CHAINS_AT_ONCE) return nullptr;
    JPK_LAUNCH(ctx, PROF_DEC_HEADERS, 0, k_dec_order, dim3(1), dim3(ORD_TB), bufs.info, g, bufs.order);
    return bufs.order;
}

// The two serial kernels are one wave per chunk.  While the chains fit one per SIMD (<= DEC_CHAINS_AT_ONCE) a 40 KB LDS reservation
// keeps them to four workgroups per CU; larger batches run without it, because two chains on a SIMD fill each other's issue
// bubbles and a second round of workgroups would wait for the first (64 blocks: 3.5 -> 4.8 GB/s, tools/dec_scaling.py).
size_t dec_chain_lds(unsigned g)
{
    static const int lds_env = (int)jpk_env_long("JPK_DEC_LDS", -1, 0, 65536);
    return (size_t)(lds_env >= 0 ? lds_env : (g <= DEC_CHAINS_AT_ONCE ? 40960 : 0));
}

// the stages' verdicts come back (synchronises the stream): any ST_* bit makes a block JPK_E_CORRUPT, every other block that passed
// the walk has its length
int dec_collect(jpk_ctx *ctx, const DecBufs &bufs, const DecPlan &plan, int32_t *status, int32_t *out_len)
{
    const size_t nblk = plan.blk_out.size();
    std::vector<uint32_t> hs(nblk);
    JPK_HIP(hipMemcpyAsync(hs.data(), bufs.status, nblk * 4, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof_on) jpk_prof_resolve(ctx);
    for (size_t b = 0; b < nblk; b++) {
        if (status[b] != JPK_OK) continue;
        if (hs[b] & (ST_RANS_CHECK | ST_RLE_MISMATCH)) { status[b] = JPK_E_CORRUPT; continue; }
        out_len[b] = (int32_t)plan.blk_out[b];
    }
    return JPK_OK;
}

}  // namespace

// the decoded size of each of nblk Ans streams from pass 1 of the batch decoder alone (no capacity applies): decoded[b], or
// status[b] = JPK_E_CORRUPT where the chunk headers are malformed
int jpk_ans_decoded_sizes(jpk_ctx *ctx, int nblk, const uint8_t *const *d_in, const int32_t *in_len, int64_t *decoded, int32_t *status)
{
    if (nblk <= 0) return JPK_OK;
    std::vector<DecBlock> hb((size_t)nblk);
    for (int b = 0; b < nblk; b++) hb[b] = dec_block(d_in[b], in_len[b], ~0ull);
    std::vector<uint32_t> mail;
    JPK_TRY(dec_count_pass(ctx, hb, 0, mail));
    for (int b = 0; b < nblk; b++) {
        const uint32_t *m = &mail[(size_t)b * MAIL_STRIDE];
        status[b] = (int32_t)m[MAIL_STATUS];
        decoded[b] = status[b] == JPK_OK ? (int64_t)mail_u64(m, MAIL_OUT_TOTAL) : 0;
    }
    return JPK_OK;
}

// Ans::Decode of `nblk` independent blocks in one pass: header walk (count), buffers, header walk (fill), then ONE grid per
// serial kernel over the chunks of all blocks.  status[b] = JPK_OK / JPK_E_CORRUPT / JPK_E_CAPACITY per block; a corrupt block
// does not stop the others.  arena_skip: bytes at the start of the arena the caller keeps for itself.
int jpk_ans_decode_batch(jpk_ctx *ctx, int nblk, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap,
                         int32_t *out_len, int32_t *status, size_t arena_skip)
{
    std::vector<DecBlock> hb((size_t)nblk);
    for (int b = 0; b < nblk; b++) {
        out_len[b] = 0;
        status[b] = JPK_OK;
        hb[b] = dec_block(d_in[b], in_len[b], (uint64_t)out_cap[b]);
        hb[b].out = d_out[b];
    }
    // ---- pass 1: count the chunks, total the sizes ----
    std::vector<uint32_t> mail;
    JPK_TRY(dec_count_pass(ctx, hb, arena_skip, mail));
    const DecPlan plan = dec_plan(mail, hb, status);
    ctx->stats.ans_chunks = (int64_t)plan.chunks;
    ctx->stats.ans_rle_symbols = (int64_t)plan.rle;
    if (plan.chunks == 0) return JPK_OK;

    DecBufs bufs;
    size_t layout_end;
    JPK_TRY(dec_layout(ctx, arena_skip, plan, hb, bufs, layout_end));
    JPK_TRY(dec_upload_and_clear(ctx, hb, bufs, layout_end));
    // ---- pass 2: fill the chunk table, then one grid per stage over all chunks ----
    const unsigned g = (unsigned)plan.chunks;
    const uint32_t *order = dec_fill_and_order(ctx, nblk, g, bufs);
    const size_t chain_lds = dec_chain_lds(g);
    JPK_TRY(run_rans(ctx, bufs, order, g, 2 * plan.rle, chain_lds));
    JPK_TRY(run_rle(ctx, bufs, g, plan.rle));
    JPK_TRY(run_rank(ctx, bufs, order, g, plan.out, chain_lds));
    JPK_HIP(hipGetLastError());
    return dec_collect(ctx, bufs, plan, status, out_len);
}

int jpk_ans_decode_device(jpk_ctx *ctx, const uint8_t *d_in, int32_t len, uint8_t *d_out, int32_t out_cap, int32_t *out_len)
{
    *out_len = 0;
    if (len == 0) return JPK_OK;
    int32_t status = JPK_OK;
    JPK_TRY(jpk_ans_decode_batch(ctx, 1, &d_in, &len, &d_out, &out_cap, out_len, &status, 0));
    return status;
}

// Postcoder::Decode (rank.cpp:96-151) for one buffer (len <= 2^31), in place
int jpk_rank_decode_device(jpk_ctx *ctx, uint8_t *d_r, const int32_t *d_freq, int32_t len)
{
    if (len == 0) return JPK_OK;
    hipStream_t st = ctx->stream;
    Arena plan(ctx, true);
    plan.get<ChunkInfo>(1);
    plan.get<DecBlock>(1);
    plan.get<uint8_t>((size_t)len + 64);
    plan.get<int32_t>(256);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    ChunkInfo *info = real.get<ChunkInfo>(1);
    DecBlock *tab = real.get<DecBlock>(1);
    uint8_t *tmp = real.get<uint8_t>((size_t)len + 64);
    int32_t *hf = real.get<int32_t>(256);
    // validate sum(freq) == len on the host (rank.cpp:104-108)
    int32_t f[256];
    JPK_HIP(hipMemcpyAsync(f, d_freq, sizeof f, hipMemcpyDeviceToHost, st));
    JPK_HIP(hipStreamSynchronize(st));
    int64_t tot = 0;
    for (int s = 0; s < 256; s++) { if (f[s] < 0) return JPK_E_CORRUPT; tot += f[s]; }
    if (tot != len) return JPK_E_CORRUPT;
    JPK_HIP(hipMemcpyAsync(hf, d_freq, sizeof f, hipMemcpyDeviceToDevice, st));
    ChunkInfo ci;
    memset(&ci, 0, sizeof ci);
    ci.olen = (uint32_t)len;
    DecBlock hb;
    memset(&hb, 0, sizeof hb);
    hb.ranks = d_r;
    hb.out = tmp;
    JPK_HIP(hipMemcpyAsync(info, &ci, sizeof ci, hipMemcpyHostToDevice, st));
    JPK_HIP(hipMemcpyAsync(tab, &hb, sizeof hb, hipMemcpyHostToDevice, st));
    JPK_HIP(hipStreamSynchronize(st));
    DecBufs bufs = {};
    bufs.tab = tab;
    bufs.info = info;
    bufs.freq = hf;
    bufs.status = &ctx->d_mail->dec.status;
    JPK_TRY(run_rank(ctx, bufs, nullptr, 1, 0, 0));       // one chain, chunk order, no LDS reservation
    JPK_HIP(hipGetLastError());
    JPK_HIP(hipMemcpyAsync(d_r, tmp, (size_t)len, hipMemcpyDeviceToDevice, st));
    JPK_HIP(hipStreamSynchronize(st));
    return JPK_OK;
}
