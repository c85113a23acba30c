// prestage_dev.hip -- the decoders of the three stages the stock CLI runs in front of the BWT (Jampack::Decomp, jampack.cpp:47-60), on gfx950,
// for batches of blocks that already sit in HBM behind the batched rANS decode + inverse BWT:
//   k_pre_lz77     Lz77::Decompress (lz77.cpp:678-714)   one workgroup per block: every lane parses the token, all lanes copy
//   k_lz77_sizes   the raw size of that stage's output alone (jpk_dev_blocks_lz77_sizes): one wave per block walks the tokens, no copies
//   k_lzx_plan     the same stage as two launches (jpk_dev_blocks_lz77_expand; the rule is lz_expand.hpp): one wave per block turns the
//   k_lzx_copy     tokens into segment records, then every thread fills aligned 16-byte words of the output from the records
//   k_lzd_plan     the same two launches with the deep rule (jpk_dev_blocks_lz77_expand_deep, the staged reader's last stage): a record
//   k_lzd_copy     budget in output bytes, lzx::DEEP_CHASE hops, and a copy that leaves a block as soon as it is marked serial
//   k_lpx<false>   Lpx::Decode      (lpx.cpp:101-169)    one workgroup per part: one lane runs the adaptive model in LDS, the others move tiles
//                  (k_pre_lpx in the profiler's table and in DESIGN 4.7)
//   k_pre_filters  Filters::Decode  (filters.cpp:442-490) one workgroup per 64 KiB filter block, scans in LDS
// and the kernels of the writer of such frames (writing; the stage chain of jpk_cli_stages_encode):
//   k_enc_wrap     raw block -> S2: the LZ77 end token and the 00 00 header of every 64 KiB filter piece around the unchanged bytes,
//                  organised by destination like k_jam_pack: a thread owns aligned 16-byte words of the output
//   k_lpx<true>    Lpx::Encode      (lpx.cpp:56-99, 148-158) one workgroup per part, the other instance of the decoder's kernel (k_enc_lpx
//                  in the profiler's table)
//   k_enc_filters  S1 -> S2 with a filter chosen per 64 KiB piece (JPK_CLI_FILTERS: in the place of k_enc_wrap): the piece and the 65
//                  histograms of the candidates in LDS, the integer cost, the choice, the transformed piece by destination
// and the dedupe of the writer's first LZ77 stage (jpk_lz77_dedupe; the rule is dedupe.hpp, shared with the host form):
//   k_dd_anchor    every aligned 64-byte window into its slot of the block's table, atomicMin on the position
//   k_dd_cand      one workgroup per tile of 1024 positions: fingerprints of all positions by six doubling steps in LDS, the candidate offset
//                  of every position (halo of one window on either side), the tile's heads compacted in position order
//   k_dd_extend    one thread per head: its run
//   k_dd_select    one workgroup per block: the greedy chain over the runs, token records with their output offsets
//   k_dd_emit      token headers and literal runs by destination, as k_enc_wrap
// Each is bit-identical to its host form in prestage.cpp (statuses included), and by construction where a rule decides a byte or a status:
// the LEB128 code, the LZ77 token, the LPX model, part cut and step, the filter sizes and the LPC recurrence are prestage_rules.hpp, the
// dedupe is dedupe.hpp, and both forms compile them.  What is written here is the device shape around the rules: the copies, the scans,
// the tiles and the word assembly.  Each keeps the host file's bounds checks: every read is checked
// against in_len and every write against out_cap before it is made, in 64-bit arithmetic.  No workgroup waits for another one, every
// loop is bounded by the stream length or the output capacity, and a bad stream sets the block's mail word and ends the workgroup.
#include <vector>

#include "common.hpp"
#include "dedupe.hpp"
#include "lz_expand.hpp"
#include "prestage_rules.hpp"

namespace {

// one block of a batch: wg0 = the workgroups of the blocks in front of it (k_lpx, k_pre_filters: several workgroups per block)
struct PreJob { const uint8_t *in; uint8_t *out; int32_t in_len; int32_t out_cap; uint32_t wg0; uint32_t pad; };

constexpr int PRE_TB = 256;
using pre::FBS;
using pre::LPX_RING;
using pre::LPX_TILE;

// the block of workgroup w: the last job with wg0 <= w (jobs without workgroups share the wg0 of their successor and are skipped by it)
__device__ __forceinline__ uint32_t job_of(const PreJob *__restrict__ jobs, uint32_t n, uint32_t w)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (jobs[mid].wg0 <= w) lo = mid; else hi = mid; }
    return lo;
}

// ---- LZ77 ----------------------------------------------------------------------------------------------------------------------
// A token is at most 16 bytes (token, three LEB128 values of up to five bytes): every wave loads the 16 bytes at `pos` once, lane l the
// byte (l & 15), and reads them back by index, so the parse is the same in every lane and costs one load per token.
__device__ __forceinline__ uint32_t win_byte(uint32_t w, int j) { return (uint32_t)__shfl((int)w, j, 64); }

// mail[2 b] = status, mail[2 b + 1] = out_len.  The match copy out[op + k] = out[op - off + k mod off] reads only bytes below op, which
// the tokens in front of this one (and this token's literals) wrote: one fence + barrier per token, between the literal copy and the
// match copy, orders all of them -- the literals of the next token touch no byte a match of this one reads or writes.
__global__ __launch_bounds__(PRE_TB) void k_pre_lz77(const PreJob *__restrict__ jobs, uint32_t *__restrict__ mail)
{
    const PreJob jb = jobs[blockIdx.x];
    const uint8_t *in = jb.in;
    uint8_t *out = jb.out;
    const int64_t in_len = jb.in_len, out_cap = jb.out_cap;
    const uint32_t tid = threadIdx.x;
    uint32_t *res = mail + 2 * (size_t)blockIdx.x;
    int64_t pos = 0, op = 0;
    int status = JPK_OK;
    while (pos < in_len) {
        const int64_t wi = pos + (int64_t)(tid & 15u);
        const uint32_t w = wi < in_len ? in[wi] : 0u;
        pre::Token t;
        if (!pre::parse_token([w](int j) { return win_byte(w, j); }, in_len - pos, &t)) { status = JPK_E_CORRUPT; break; }
        const int32_t off = t.off;
        const int64_t len = t.len, lit = t.lit;
        pos += t.used;
        if (off == 0) {                                                // end marker: raw remainder
            const int64_t rest = in_len - pos;
            if (op + rest > out_cap) { status = JPK_E_CAPACITY; break; }
            for (int64_t k = tid; k < rest; k += PRE_TB) out[op + k] = in[pos + k];
            op += rest;
            break;
        }
        if (off < 0 || lit > in_len - pos) { status = JPK_E_CORRUPT; break; }
        if (lit + len > out_cap - op) { status = JPK_E_CAPACITY; break; }
        for (int64_t k = tid; k < lit; k += PRE_TB) out[op + k] = in[pos + k];
        op += lit;
        pos += lit;
        if ((int64_t)off > op) { status = JPK_E_CORRUPT; break; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __syncthreads();
        {
            const uint32_t L = (uint32_t)len, O = (uint32_t)off;       // len <= out_cap - op, off <= op: both below 2^31
            uint8_t *dst = out + op;
            const uint8_t *src = dst - O;
            if (O >= L) {
                for (uint32_t k = tid; k < L; k += PRE_TB) dst[k] = src[k];
            } else {
                uint32_t r = tid % O;
                const uint32_t step = (uint32_t)PRE_TB % O;
                for (uint32_t k = tid; k < L; k += PRE_TB) {
                    dst[k] = src[r];
                    r += step;
                    if (r >= O) r -= O;
                }
            }
        }
        op += len;
    }
    if (tid == 0) { res[0] = (uint32_t)status; res[1] = status == JPK_OK ? (uint32_t)op : 0u; }
}

// The raw size of a block without its bytes (jpk_dev_blocks_lz77_sizes; the rule is lzx::Size of lz_expand.hpp, which jpk_lz77_size
// compiles too): one wave per block walks the tokens as k_pre_lz77 does, with its checks in its order, and copies nothing.  mail as
// k_pre_lz77, the two words stored by lane 0 -- the only stores; jb.out is not looked at.  No LDS, no barrier.  Every iteration moves
// pos by the token's bytes (two at least) or ends the walk, so the loop ends at in_len on any stream.
__global__ __launch_bounds__(64) void k_lz77_sizes(const PreJob *__restrict__ jobs, uint32_t *__restrict__ mail)
{
    const PreJob jb = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const int64_t in_len = jb.in_len;
    lzx::Size s;
    while (lzx::more(s, in_len)) {
        const int64_t wi = s.pos + (int64_t)(tid & 15u);
        const uint32_t w = wi < in_len ? jb.in[wi] : 0u;
        pre::Token t;
        const bool parsed = pre::parse_token([w](int j) { return win_byte(w, j); }, in_len - s.pos, &t);
        lzx::step(s, parsed, t, in_len, (int64_t)jb.out_cap);
    }
    if (tid == 0) {
        uint32_t *res = mail + 2 * (size_t)blockIdx.x;
        res[0] = (uint32_t)s.status;
        res[1] = (uint32_t)lzx::out_len(s);
    }
}

// ---- the parallel LZ77 expander ------------------------------------------------------------------------------------------------
// Two launches for a batch ("Staged frames"); what decides a byte or a status is lz_expand.hpp.  A block that fails a check
// of the plan, needs more records than it has, or holds a byte more than lzx::MAX_CHASE matches away from its literal is left to
// k_pre_lz77, which gives it its bytes and its status: nothing here loops on a hostile stream, and no workgroup waits for another.
struct LzxJob { const uint8_t *in; uint8_t *out; lzx::Seg *segs; int32_t in_len; int32_t out_cap; uint32_t cap; uint32_t pad; };
constexpr uint32_t LZX_WORDS = 4;                                     // 16-byte words per thread, as k_enc_wrap
constexpr uint32_t LZX_INFO = 4;                                      // info words per block: serial (plan), out_len, records, serial (copy)

// One wave per block: the token walk of k_pre_lz77 without its copies; lane 0 stores the records.  DEEP: the budget of lzx::deep_step
// behind every token in the place of the record cap alone.
template <bool DEEP> __device__ __forceinline__ void lzx_plan_block(const LzxJob *__restrict__ jobs, uint32_t *__restrict__ info)
{
    const LzxJob jb = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const int64_t in_len = jb.in_len;
    lzx::Seg *segs = jb.segs;
    lzx::Plan p;
    while (lzx::more(p, in_len)) {
        const int64_t wi = p.pos + (int64_t)(tid & 15u);
        const uint32_t w = wi < in_len ? jb.in[wi] : 0u;
        pre::Token t;
        const bool parsed = pre::parse_token([w](int j) { return win_byte(w, j); }, in_len - p.pos, &t);
        auto put = [segs, tid](uint32_t i, const lzx::Seg &sg) { if (tid == 0) segs[i] = sg; };
        if (DEEP) lzx::deep_step(p, parsed, t, in_len, (int64_t)jb.out_cap, jb.cap, put);
        else lzx::step(p, parsed, t, in_len, (int64_t)jb.out_cap, jb.cap, put);
    }
    if (tid == 0) {
        uint32_t *r = info + LZX_INFO * (size_t)blockIdx.x;
        r[0] = p.serial ? 1u : 0u;
        r[1] = p.serial ? 0u : (uint32_t)p.op;
        r[2] = p.nseg;
    }
}

__global__ __launch_bounds__(64) void k_lzx_plan(const LzxJob *__restrict__ jobs, uint32_t *__restrict__ info) { lzx_plan_block<false>(jobs, info); }

// The plan of the deep expander (jpk_dev_blocks_lz77_expand_deep): the same walk; a block is given up behind the first token that leaves
// it with more than op / 128 + 4 records, so the walk of a dense stream ends within its first tokens and that of any stream after at
// most out_cap / 128 + 4 records' worth of tokens.  Every iteration moves pos by the token's bytes or ends the walk.
__global__ __launch_bounds__(64) void k_lzd_plan(const LzxJob *__restrict__ jobs, uint32_t *__restrict__ info) { lzx_plan_block<true>(jobs, info); }

// Organised by destination as k_dd_emit: grid (workgroups of the largest out_cap, blocks), a workgroup owns LZX_WORDS * PRE_TB aligned
// 16-byte words of its block's output.  A word that lies inside one record follows the matches as a whole -- lzx::back of its first byte,
// while its 16 bytes stay inside one record and inside one period -- down to a literal run, which it reads through two aligned loads when
// both lie inside the input; every other word resolves its bytes one by one (lzx::source).  Whole words are stored once, the partial words
// at the two ends with byte stores: nothing outside [out, out + out_len) is written, and every read is of an input byte a record covers.
// HOPS is the cap of the chase.  WATCH: the thread reads the block's two serial words -- the plan's and the one a thread of this launch
// sets on finding a byte too deep -- in front of every word it resolves and returns when either is set, so a block on its way to the
// serial kernel costs what was in flight and not a whole copy.  The read for a word is issued one word early (for the first word, on
// entry) and is in flight while the word in front of it resolves: it costs no round trip of its own.
template <uint32_t HOPS, bool WATCH> __device__ __forceinline__ void lzx_copy_block(const LzxJob *__restrict__ jobs, uint32_t *__restrict__ info)
{
    const LzxJob jb = jobs[blockIdx.y];
    uint32_t *inf = info + LZX_INFO * (size_t)blockIdx.y;
    const uint32_t total = inf[1], nseg = inf[2];
    if (inf[0] || total == 0u) return;
    uint32_t stop = WATCH ? __hip_atomic_load(&inf[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const lzx::Seg *__restrict__ segs = jb.segs;
    const uintptr_t base = (uintptr_t)jb.out & ~(uintptr_t)15, r_lo = (uintptr_t)jb.in, r_hi = r_lo + (uint32_t)jb.in_len;
    const uint32_t lead = (uint32_t)((uintptr_t)jb.out - base);
    const uint64_t words = ((uint64_t)lead + total + 15u) / 16u;
    const uint64_t w0 = (uint64_t)blockIdx.x * (LZX_WORDS * PRE_TB) + threadIdx.x;
#pragma unroll 1
    for (uint32_t t = 0; t < LZX_WORDS; t++) {
        const uint64_t w = w0 + (uint64_t)t * PRE_TB;
        if (w >= words) break;
        if (WATCH) {
            if (stop) return;
            stop = __hip_atomic_load(&inf[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | __hip_atomic_load(&inf[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const int64_t p0 = (int64_t)(w * 16u) - (int64_t)lead;
        uint8_t *dst = reinterpret_cast<uint8_t *>(base + w * 16u);
        const bool whole = p0 >= 0 && (uint64_t)p0 + 16u <= total;
        const uint32_t first = p0 < 0 ? 0u : (uint32_t)p0;
        uint32_t idx = lzx::find(segs, nseg, first);
        lzx::Seg sg = segs[idx];
        if (whole) {
            uint32_t p = first, i = idx;
            lzx::Seg s = sg;
            bool word = true, deep = false;
            for (uint32_t k = 0;; k++) {
                if ((uint64_t)p + 16u > (uint64_t)s.out + s.len) { word = false; break; }       // the word crosses into the next record
                if (!s.match) break;
                if (k == HOPS) { deep = true; break; }
                const uint32_t r = (p - s.out) % s.src;
                if ((uint64_t)r + 16u > s.src) { word = false; break; }                         // the word crosses the period's end
                p = s.out - s.src + r;
                i = lzx::find(segs, i, p);
                s = segs[i];
            }
            if (deep) { inf[3] = 1u; continue; }
            if (word) {
                const uint8_t *src = jb.in + s.src + (p - s.out);
                const uintptr_t a = (uintptr_t)src & ~(uintptr_t)15;
                uint4 v;
                if (a >= r_lo && a + (((uintptr_t)src & 15u) ? 32u : 16u) <= r_hi) {
                    v = load16_unaligned(src);
                } else {
                    uint32_t b[16];
#pragma unroll
                    for (int j = 0; j < 16; j++) b[j] = src[j];
                    v.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
                    v.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
                    v.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
                    v.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
                }
                *reinterpret_cast<uint4 *>(dst) = v;
                continue;
            }
        }
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        bool deep = false;
#pragma unroll 1
        for (uint32_t j = 0; j < 16u; j++) {
            const int64_t p = p0 + (int64_t)j;
            if (p < 0 || (uint64_t)p >= total) continue;
            while (idx + 1 < nseg && (uint64_t)p >= (uint64_t)sg.out + sg.len) sg = segs[++idx];
            uint32_t io = 0;
            if (!lzx::source(segs, idx, sg, (uint32_t)p, HOPS, &io)) { deep = true; break; }
            const uint32_t byte = jb.in[io];
            if (!whole) dst[j] = (uint8_t)byte;
            const uint32_t sh = byte << (8u * (j & 3u)), q = j >> 2;
            v[0] |= q == 0u ? sh : 0u; v[1] |= q == 1u ? sh : 0u; v[2] |= q == 2u ? sh : 0u; v[3] |= q == 3u ? sh : 0u;
        }
        if (deep) { inf[3] = 1u; continue; }
        if (whole) *reinterpret_cast<uint4 *>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

__global__ __launch_bounds__(PRE_TB) void k_lzx_copy(const LzxJob *__restrict__ jobs, uint32_t *__restrict__ info)
{
    lzx_copy_block<lzx::MAX_CHASE, false>(jobs, info);
}

// The copy of the deep expander: lzx::DEEP_CHASE hops, and the block's serial words in front of every word.  Every loop is bounded by the
// hop cap, the record count (the binary search, the walk to the next record) or the 16 bytes of a word: on a hostile stream the launch
// does O(records + DEEP_CHASE * log records * bytes) work and waits for nothing.
__global__ __launch_bounds__(PRE_TB) void k_lzd_copy(const LzxJob *__restrict__ jobs, uint32_t *__restrict__ info)
{
    lzx_copy_block<lzx::DEEP_CHASE, true>(jobs, info);
}

// ---- LPX -----------------------------------------------------------------------------------------------------------------------
// One workgroup per part (pre::part_of: a block is cut into parts of len / 4 bytes, each with a fresh model).  The model is byte-serial and
// adaptive -- every byte's prediction depends on the tables the byte in front of it left -- so the chain of a part is ONE lane running
// pre::step, with the three tables (15 KiB), one tile (16 KiB) and a ring of the last 64 KiB + one tile of PLAIN bytes (80 KiB) in LDS: 111
// KiB, one workgroup per CU; the other lanes only move tiles between HBM and LDS.  A stretch may cross a tile edge (pre::Walk::run).
//   decode  the tile holds the input, lane 0 leaves the output in the ring (its predictions read it), all lanes write the ring's tile out
//   encode  the whole input is known, so the chain reads only input bytes: all lanes load a tile straight into the ring, lane 0 leaves the
//           error bytes in the tile, all lanes write the tile out.  token != 0: the job's output is S3 inside an S4 buffer and part 0 puts
//           the LZ77 end token into the two bytes in front of it.
template <bool ENC> __global__ __launch_bounds__(PRE_TB) void k_lpx(const PreJob *__restrict__ jobs, uint32_t n, uint32_t token)
{
    __shared__ pre::Record table[3][256];
    __shared__ uint8_t tile[LPX_TILE];
    __shared__ uint8_t ring[LPX_RING];
    const uint32_t tid = threadIdx.x;
    const PreJob jb = jobs[job_of(jobs, n, blockIdx.x)];
    const uint32_t pi = blockIdx.x - jb.wg0;
    uint32_t start, plen;
    if (!pre::part_of((uint32_t)jb.in_len, pi, &start, &plen)) return;
    const uint8_t *in = jb.in + start;
    uint8_t *out = jb.out + start;
    if (ENC && token && pi == 0 && tid == 0) { jb.out[-2] = pre::END_TOKEN[0]; jb.out[-1] = pre::END_TOKEN[1]; }
    for (uint32_t k = tid; k < 3u * 256u; k += PRE_TB) table[k >> 8][k & 255u] = pre::fresh_record();
    pre::Walk w;
    for (uint32_t base = 0; base < plen; base += LPX_TILE) {
        const uint32_t cnt = plen - base < LPX_TILE ? plen - base : LPX_TILE;
        const uint32_t rb = base % LPX_RING;
        for (uint32_t k = tid; k < cnt; k += PRE_TB) {
            const uint32_t q = rb + k;
            if constexpr (ENC) ring[q >= LPX_RING ? q - LPX_RING : q] = in[base + k];
            else tile[k] = in[base + k];
        }
        __syncthreads();                                               // (orders the table set-up and the last tile's reads as well)
        if (tid == 0) {
            uint32_t wi = rb;                                          // ring index of position i
            for (uint32_t k = 0; k < cnt; k++) {
                const uint8_t o = pre::step<ENC>(table, w, base + k, ENC ? ring[wi] : tile[k], [&](uint32_t d) { return ring[pre::ring_back(wi, d)]; });
                if constexpr (ENC) tile[k] = o;
                else ring[wi] = o;
                wi = wi + 1 == LPX_RING ? 0u : wi + 1;
            }
        }
        __syncthreads();
        for (uint32_t k = tid; k < cnt; k += PRE_TB) {
            const uint32_t q = rb + k;
            out[base + k] = ENC ? tile[k] : ring[q >= LPX_RING ? q - LPX_RING : q];
        }
    }
}

// ---- filters -------------------------------------------------------------------------------------------------------------------
// Running sums with stride W in LDS, in place: s[k0 + m W + c] += s[k0 + (m - 1) W + c] for m = 1 .. M - 1, every channel c < W on
// its own (mod 256).  Thread t owns channel t mod W and the (t / W)-th run of rows: partial sums, their prefix over the runs in front
// of its own, then the running sum over its rows.  All threads of the workgroup call it.
__device__ __forceinline__ void scan_stride(uint8_t *s, uint32_t *part, uint32_t k0, uint32_t W, uint32_t M)
{
    const uint32_t tid = threadIdx.x, ch = tid % W, sg = tid / W, nseg = (uint32_t)PRE_TB / W;
    const uint32_t rows = (M + nseg - 1) / nseg;
    const uint32_t m0 = sg < nseg ? (sg * rows < M ? sg * rows : M) : M, m1 = m0 + rows < M ? m0 + rows : M;
    uint32_t sum = 0;
    for (uint32_t m = m0; m < m1; m++) sum += s[k0 + m * W + ch];
    part[tid] = sum;
    __syncthreads();
    uint32_t acc = 0;
    if (sg < nseg) for (uint32_t g = 0; g < sg; g++) acc += part[g * W + ch];
    for (uint32_t m = m0; m < m1; m++) {
        acc += s[k0 + m * W + ch];
        s[k0 + m * W + ch] = (uint8_t)acc;
    }
    __syncthreads();
}

// One workgroup per filter block: block j of a stream starts at j (65536 + 2) and writes at j 65536 (all blocks but the last are full).
// mail[b] (preset to 0xFFFFFFFF) takes the minimum of (j << 1 | capacity) over the blocks that fail, so that the host reports what
// jpk_filters_decode reports: the status of the FIRST failing block, its header checked before its capacity.
__global__ __launch_bounds__(PRE_TB) void k_pre_filters(const PreJob *__restrict__ jobs, uint32_t n, uint32_t *__restrict__ mail)
{
    __shared__ uint8_t s[FBS];
    __shared__ uint32_t part[PRE_TB];
    const uint32_t tid = threadIdx.x;
    const uint32_t b = job_of(jobs, n, blockIdx.x);
    const PreJob jb = jobs[b];
    const int64_t in_len = jb.in_len, out_cap = jb.out_cap;
    const uint32_t j = blockIdx.x - jb.wg0;
    const int64_t i0 = (int64_t)j * (FBS + 2);
    if (i0 >= in_len) return;
    if (i0 + 2 > in_len) { if (tid == 0) atomicMin(&mail[b], j << 1); return; }
    const uint32_t type = jb.in[i0], width = jb.in[i0 + 1];
    if (type >= 3 || width > 32) { if (tid == 0) atomicMin(&mail[b], j << 1); return; }       // "unsupported configuration", filters.cpp:455
    const uint32_t len = in_len - (i0 + 2) < (int64_t)FBS ? (uint32_t)(in_len - (i0 + 2)) : FBS;
    const int64_t op = (int64_t)j * FBS;
    if (op + len > out_cap) { if (tid == 0) atomicMin(&mail[b], (j << 1) | 1u); return; }
    const uint8_t *src = jb.in + i0 + 2;
    uint8_t *dst = jb.out + op;
    if (width == 0) {
        for (uint32_t k = tid; k < len; k += PRE_TB) dst[k] = src[k];
        return;
    }
    for (uint32_t k = tid; k < len; k += PRE_TB) s[k] = src[k];
    __syncthreads();
    if (type == 2) {                                                   // InlineUndelta: running sum per channel in place, behind a raw head
        const uint32_t k0 = len % width;
        scan_stride(s, part, k0, width, (len - k0) / width);
        for (uint32_t k = tid; k < len; k += PRE_TB) dst[k] = s[k];
        return;
    }
    if (type == 0) {                                                   // DeltaDecode: running sum over the whole block
        scan_stride(s, part, 0, 1, len);
    } else {                                                           // LpcDecode: serial
        if (tid == 0) pre::lpc_decode(s, s, len);
        __syncthreads();
    }
    // Unreorder: channel c holds bytes c, c + width, ...: it has len / width elements, one more when c < len mod width
    const uint32_t q = len / width, r = len % width;
    for (uint32_t k = tid; k < len; k += PRE_TB) {
        const uint32_t c = k % width;
        dst[k] = s[c * q + (c < r ? c : r) + k / width];
    }
}

// ---- the stored forms: raw block -> S2 ----------------------------------------------------------------------------------------------
constexpr uint32_t WRAP_PIECE = FBS + 2;                              // one filter piece in S2: header + 64 KiB of S1
constexpr uint32_t WRAP_WORDS = 4;                                    // 16-byte words per thread: a workgroup writes 16 KiB

// byte p of S2 (prestage.cpp: S1 = 04 80 | R, every 64 KiB piece of S1 behind 00 00); TOK = false: `in` is S1 itself (the dedupe wrote it)
template <bool TOK> __device__ __forceinline__ uint32_t wrap_byte(uint32_t p, const uint8_t *__restrict__ in)
{
    const uint32_t pj = p / WRAP_PIECE, r = p % WRAP_PIECE;
    if (r < 2u) return 0u;
    const uint32_t s1 = pj * FBS + r - 2u;
    if (!TOK) return in[s1];
    return s1 < 2u ? (s1 == 0u ? pre::END_TOKEN[0] : pre::END_TOKEN[1]) : in[s1 - 2u];
}

// Job: in = R (in_len bytes), out = S2 (out_cap = |S2| bytes), wg0 as for the other kernels; a workgroup owns WRAP_WORDS * PRE_TB
// consecutive aligned 16-byte words of the job's output (word w = the 16 bytes at base + 16 w, base = out rounded down to 16).  A whole
// word whose bytes all come from R -- S2[p] = R[p - 2 j - 4] inside piece j, behind its header and behind the token -- moves through two
// aligned 16-byte loads when both lie inside R; every other word (a header, the token, the ends of R or of S2) is assembled byte by byte,
// whole words stored once, the partial words at the two ends with byte stores.  Nothing outside [out, out + |S2|) is written.
template <bool TOK> __global__ __launch_bounds__(PRE_TB) void k_enc_wrap(const PreJob *__restrict__ jobs, uint32_t n)
{
    const PreJob jb = jobs[job_of(jobs, n, blockIdx.x)];
    const uint32_t total = (uint32_t)jb.out_cap;
    const uintptr_t base = (uintptr_t)jb.out & ~(uintptr_t)15, r_lo = (uintptr_t)jb.in, r_hi = r_lo + (uint32_t)jb.in_len;
    const uint32_t lead = (uint32_t)((uintptr_t)jb.out - base);
    const uint32_t words = (uint32_t)(((uint64_t)lead + total + 15u) / 16u);
    const uint64_t w0 = (uint64_t)(blockIdx.x - jb.wg0) * (WRAP_WORDS * PRE_TB) + threadIdx.x;
#pragma unroll
    for (uint32_t t = 0; t < WRAP_WORDS; t++) {
        const uint64_t w = w0 + (uint64_t)t * PRE_TB;
        if (w >= words) break;
        const int64_t p0 = (int64_t)(w * 16u) - (int64_t)lead;         // S2 position of the word's first byte (< 0: before the block)
        uint8_t *dst = reinterpret_cast<uint8_t *>(base + w * 16u);
        const bool whole = p0 >= 0 && (uint64_t)p0 + 16u <= total;
        if (whole) {
            const uint32_t pj = (uint32_t)p0 / WRAP_PIECE, r = (uint32_t)p0 % WRAP_PIECE;
            if (r >= 2u && r + 16u <= WRAP_PIECE && (!TOK || pj > 0u || r >= 4u)) {
                const uint8_t *src = jb.in + ((uint32_t)p0 - 2u * pj - (TOK ? 4u : 2u));
                const uintptr_t a = (uintptr_t)src & ~(uintptr_t)15;
                if (a >= r_lo && a + (((uintptr_t)src & 15u) ? 32u : 16u) <= r_hi) {
                    *reinterpret_cast<uint4 *>(dst) = load16_unaligned(src);
                    continue;
                }
            }
        }
        uint32_t b[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            b[j] = 0;
            if (p < 0 || (uint64_t)p >= total) continue;
            b[j] = wrap_byte<TOK>((uint32_t)p, jb.in);
            if (!whole) dst[j] = (uint8_t)b[j];
        }
        if (whole) {
            uint4 v;
            v.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            v.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            v.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            v.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
            *reinterpret_cast<uint4 *>(dst) = v;
        }
    }
}

// ---- the filter choice: S1 -> S2 (Filters::Encode with the rule of prestage_rules.hpp, DESIGN 4.7 "Filters") ---------------------------
constexpr uint32_t FLT_RAW = pre::FILTER_CANDS;                       // histogram and cost of the raw piece, behind the 64 candidates'
constexpr uint32_t FLT_HISTS = pre::FILTER_CANDS + 1;

// One workgroup per 64 KiB piece of S1; piece j of a block reads at j 65536 and writes at j (65536 + 2).  Job: in = R (TOK: S1 = 04 80 | R)
// or S1 itself (the dedupe's, the batch entry's), in_len its bytes, out = S2, out_cap its room.  The piece (64 KiB) and 65 histograms of 256
// words (65 KiB) live in LDS: one workgroup per CU.
//   1 the raw histogram and, per width w, that of the differences x[k] - x[k - w]: a thread takes four positions from nine aligned words
//   2 the differences copied for type 2, then one thread per candidate applies pre::filter_fixups to its histogram
//   3 a wave per candidate, a lane per four byte values: pre::cost_term summed over the wave (integer sums: any order gives the host's)
//   4 thread 0 walks pre::filter_choose and writes the header; all threads write pre::filter_byte by destination
// Every piece byte read is below len, every write inside [out, out + out_cap).
template <bool TOK> __global__ __launch_bounds__(PRE_TB) void k_enc_filters(const PreJob *__restrict__ jobs, uint32_t n)
{
    __shared__ __attribute__((aligned(16))) uint8_t s[FBS];
    __shared__ uint32_t hist[FLT_HISTS][256];
    __shared__ long long cost[FLT_HISTS];
    __shared__ uint32_t pick[2];
    const uint32_t tid = threadIdx.x;
    const PreJob jb = jobs[job_of(jobs, n, blockIdx.x)];
    const int64_t s1 = (int64_t)jb.in_len + (TOK ? 2 : 0);
    const uint32_t j = blockIdx.x - jb.wg0;
    const int64_t i0 = (int64_t)j * FBS;
    if (i0 >= s1) return;
    const uint32_t len = s1 - i0 < (int64_t)FBS ? (uint32_t)(s1 - i0) : FBS;
    const int64_t op = (int64_t)j * (FBS + 2);
    if (op + 2 + (int64_t)len > (int64_t)jb.out_cap) return;           // the host sized the output: cannot happen, and nothing is written if it does
    uint8_t *dst = jb.out + op;
    for (uint32_t k = tid; k < len; k += PRE_TB) {
        const int64_t g = i0 + k;
        if (TOK) s[k] = g < 2 ? (g == 0 ? pre::END_TOKEN[0] : pre::END_TOKEN[1]) : jb.in[g - 2];
        else s[k] = jb.in[g];
    }
    for (uint32_t k = tid; k < FLT_HISTS * 256u; k += PRE_TB) (&hist[0][0])[k] = 0u;
    __syncthreads();
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(s);
    for (uint32_t b4 = tid; b4 * 4u < len; b4 += PRE_TB) {             // positions 4 b4 .. 4 b4 + 3 and the 32 bytes in front of them
        uint32_t wd[9];
#pragma unroll
        for (int i = 0; i < 9; i++) wd[i] = b4 + (uint32_t)i >= 8u ? s32[b4 + (uint32_t)i - 8u] : 0u;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t k = b4 * 4u + (uint32_t)e;
            if (k < len) {
                const uint32_t v = (wd[8] >> (8 * e)) & 255u;
                atomicAdd(&hist[FLT_RAW][v], 1u);
#pragma unroll
                for (int w = 1; w <= (int)pre::FILTER_WIDTHS; w++) {
                    const int o = 32 + e - w;                          // byte k - w in wd
                    if ((uint32_t)w <= k) atomicAdd(&hist[w - 1][(v - ((wd[o >> 2] >> (8 * (o & 3))) & 255u)) & 255u], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < pre::FILTER_WIDTHS * 256u; k += PRE_TB) (&hist[pre::FILTER_WIDTHS][0])[k] = (&hist[0][0])[k];
    __syncthreads();
    const uint8_t *x = s;
    const auto get = [x](uint32_t i) { return (uint32_t)x[i]; };
    if (tid < pre::FILTER_CANDS) {
        uint32_t *h = hist[tid];                                       // this thread's alone
        pre::filter_fixups(get, len, tid < pre::FILTER_WIDTHS ? 0u : 2u, (tid % pre::FILTER_WIDTHS) + 1u, [h](uint8_t b, int d) { h[b] += (uint32_t)d; });
    }
    __syncthreads();
    const uint32_t lg_len = pre::lg12(len), lane = tid & 63u;
    for (uint32_t c = tid >> 6; c < FLT_HISTS; c += PRE_TB / 64) {
        long long a = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) a += pre::cost_term(hist[c][lane + 64u * q], lg_len);
        for (int off = 32; off; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) cost[c] = a;
    }
    __syncthreads();
    if (tid == 0) {
        const long long *cs = cost;
        const pre::FilterChoice ch = pre::filter_choose((int64_t)cs[FLT_RAW], [cs](uint32_t type, uint32_t w) {
            return (int64_t)cs[(type / 2u) * pre::FILTER_WIDTHS + w - 1u];
        });
        pick[0] = ch.type; pick[1] = ch.width;
        dst[0] = (uint8_t)ch.type; dst[1] = (uint8_t)ch.width;
    }
    __syncthreads();
    const uint32_t type = pick[0], width = pick[1];
    for (uint32_t k = tid; k < len; k += PRE_TB) dst[2 + k] = pre::filter_byte(get, len, type, width, k);
}

// pieces of S1: the workgroups k_enc_filters needs for a block
inline uint64_t filter_pieces(int64_t s1) { return (uint64_t)((s1 + FBS - 1) / FBS); }

// ---- the dedupe ------------------------------------------------------------------------------------------------------------------
// One block of a batch.  Every k_dd_* grid is (workgroups of the largest block, blocks): a workgroup past its block's end leaves at once.
struct DdJob {
    const uint8_t *in; uint8_t *out; uint32_t *table; uint4 *heads; uint32_t *cnt; dd::Tok *toks;
    uint32_t n; int32_t bits; uint32_t total; uint32_t ntok;        // total, ntok: set for k_dd_emit (total == 0: the block is skipped)
};
constexpr uint32_t DD_HALO = dd::W;                                   // candidate offsets of one window on either side of the tile
constexpr uint32_t DD_NP = dd::TILE + 2 * DD_HALO;                    // positions whose offset a tile computes
constexpr uint32_t DD_NH = DD_NP + dd::W;                             // fingerprint cells (the last W - 1 feed the doubling only)

__global__ __launch_bounds__(PRE_TB) void k_dd_anchor(const DdJob *__restrict__ jobs)
{
    const DdJob jb = jobs[blockIdx.y];
    const uint64_t q = ((uint64_t)blockIdx.x * PRE_TB + threadIdx.x) * dd::W;
    if (q + dd::W > jb.n) return;
    atomicMin(&jb.table[dd::slot(dd::fp_at(jb.in, (uint32_t)q), jb.bits)], (uint32_t)q);
}

// heads[tile * TILE_HEADS + k] = (p, d, 0, 0) for the tile's first TILE_HEADS heads in position order, cnt[tile] = their number
__global__ __launch_bounds__(PRE_TB) void k_dd_cand(const DdJob *__restrict__ jobs)
{
    __shared__ uint32_t ha[DD_NH], hb[DD_NH];
    __shared__ uint32_t wsum[PRE_TB / 64];
    const DdJob jb = jobs[blockIdx.y];
    const uint32_t tid = threadIdx.x, n = jb.n;
    const uint64_t t0 = (uint64_t)blockIdx.x * dd::TILE;
    if (t0 >= n) return;
    const int64_t g0 = (int64_t)t0 - DD_HALO;                          // cell i stands for position g0 + i
    for (uint32_t i = tid; i < DD_NH; i += PRE_TB) {
        const int64_t g = g0 + i;
        ha[i] = (g >= 0 && g < (int64_t)n) ? (uint32_t)jb.in[g] + 1u : 0u;
    }
    __syncthreads();
    uint32_t *src = ha, *dst = hb;
    uint32_t mul = dd::MUL;
#pragma unroll
    for (uint32_t k = 1; k < dd::W; k <<= 1) {                         // h2k(p) = hk(p) MUL^k + hk(p + k)
        for (uint32_t i = tid; i + k < DD_NH; i += PRE_TB) dst[i] = src[i] * mul + src[i + k];
        __syncthreads();
        uint32_t *t = src; src = dst; dst = t;
        mul *= mul;
    }
    // src[i] = fp(g0 + i) for i < DD_NP (every cell it was summed from exists); dst receives the candidate offsets
    for (uint32_t i = tid; i < DD_NP; i += PRE_TB) {
        const int64_t p = g0 + i;
        dst[i] = (p >= (int64_t)dd::W && p + (int64_t)dd::W <= (int64_t)n) ? dd::cand_fp(jb.in, n, jb.table, jb.bits, (uint32_t)p, src[i]) : 0u;
    }
    __syncthreads();
    // thread t owns positions t0 + 4 t .. + 3: flags, an exclusive scan over the workgroup, the first TILE_HEADS are written
    uint32_t flag[4], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t i = DD_HALO + 4u * tid + k;
        flag[k] = dd::is_head((uint32_t)(t0 + 4u * tid + k), dst[i - dd::W], dst[i], dst[i + dd::W]) ? 1u : 0u;
        mine += flag[k];
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
        if ((tid & 63u) >= (uint32_t)o) incl += v;
    }
    if ((tid & 63u) == 63u) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < PRE_TB / 64; w++) { if (w < (tid >> 6)) base += wsum[w]; all += wsum[w]; }
    uint32_t at = base + incl - mine;
    uint4 *heads = jb.heads + (size_t)blockIdx.x * dd::TILE_HEADS;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (flag[k]) {
            if (at < dd::TILE_HEADS) heads[at] = make_uint4((uint32_t)(t0 + 4u * tid + k), dst[DD_HALO + 4u * tid + k], 0u, 0u);
            at++;
        }
    }
    if (tid == 0) jb.cnt[blockIdx.x] = all < dd::TILE_HEADS ? all : dd::TILE_HEADS;
}

// heads[i] = (p, d, 0, 0) -> (s, d, e, 0)
__global__ __launch_bounds__(PRE_TB) void k_dd_extend(const DdJob *__restrict__ jobs)
{
    const DdJob jb = jobs[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * PRE_TB + threadIdx.x;
    const uint64_t tile = i / dd::TILE_HEADS;
    if (tile >= dd::tiles(jb.n) || (uint32_t)(i % dd::TILE_HEADS) >= jb.cnt[tile]) return;
    const uint4 h = jb.heads[i];
    const dd::Run r = dd::extend(jb.in, jb.n, jb.table, jb.bits, h.x, h.y);
    jb.heads[i] = make_uint4(r.s, r.d, r.e, 0u);
}

// One workgroup per block: all threads bring the runs of DD_SEL_TILES tiles into LDS, thread 0 walks them in order (dd::Select).
// mail[2 b] = |S1'|, mail[2 b + 1] = token records (the end token included).
constexpr uint32_t DD_SEL_TILES = PRE_TB / dd::TILE_HEADS;
__global__ __launch_bounds__(PRE_TB) void k_dd_select(const DdJob *__restrict__ jobs, uint32_t *__restrict__ mail)
{
    __shared__ uint4 rec[PRE_TB];
    __shared__ uint32_t scnt[DD_SEL_TILES];
    const DdJob jb = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x, ntiles = dd::tiles(jb.n);
    dd::Select sel(jb.toks, true);
    for (uint32_t tb = 0; tb < ntiles; tb += DD_SEL_TILES) {
        const uint32_t tile = tb + tid / dd::TILE_HEADS;
        if (tid < DD_SEL_TILES) scnt[tid] = tb + tid < ntiles ? jb.cnt[tb + tid] : 0u;
        if (tile < ntiles) rec[tid] = jb.heads[(size_t)tb * dd::TILE_HEADS + tid];
        __syncthreads();
        if (tid == 0) {
            for (uint32_t t = 0; t < DD_SEL_TILES; t++)
                for (uint32_t k = 0; k < scnt[t]; k++) {
                    const uint4 v = rec[t * dd::TILE_HEADS + k];
                    dd::Run r;
                    r.s = v.x; r.d = v.y; r.e = v.z;
                    sel.add(r);
                }
        }
        __syncthreads();
    }
    if (tid == 0) {
        mail[2 * (size_t)blockIdx.x] = sel.finish(jb.n);
        mail[2 * (size_t)blockIdx.x + 1] = sel.ntok;
    }
}

// byte p of S1' behind token record i (the last one with out_off <= p)
__device__ __forceinline__ uint32_t dd_byte(const DdJob &jb, const dd::Tok &t, uint32_t p)
{
    const uint32_t r = p - t.out_off;
    return r < t.hlen ? t.hdr[r] : jb.in[t.lit_src + (r - t.hlen)];
}

// A workgroup owns WRAP_WORDS * PRE_TB aligned 16-byte words of the block's output, as k_enc_wrap.  A whole word inside one literal run
// moves through two aligned loads when both lie inside the block; every other word is assembled byte by byte.  Nothing outside
// [out, out + total) is written.
__global__ __launch_bounds__(PRE_TB) void k_dd_emit(const DdJob *__restrict__ jobs)
{
    const DdJob jb = jobs[blockIdx.y];
    const uint32_t total = jb.total;
    if (total == 0u) return;
    const uintptr_t base = (uintptr_t)jb.out & ~(uintptr_t)15, r_lo = (uintptr_t)jb.in, r_hi = r_lo + jb.n;
    const uint32_t lead = (uint32_t)((uintptr_t)jb.out - base);
    const uint64_t words = ((uint64_t)lead + total + 15u) / 16u;
    const uint64_t w0 = (uint64_t)blockIdx.x * (WRAP_WORDS * PRE_TB) + threadIdx.x;
#pragma unroll 1
    for (uint32_t t = 0; t < WRAP_WORDS; t++) {
        const uint64_t w = w0 + (uint64_t)t * PRE_TB;
        if (w >= words) break;
        const int64_t p0 = (int64_t)(w * 16u) - (int64_t)lead;
        uint8_t *dst = reinterpret_cast<uint8_t *>(base + w * 16u);
        const bool whole = p0 >= 0 && (uint64_t)p0 + 16u <= total;
        const uint32_t first = p0 < 0 ? 0u : (uint32_t)p0;
        uint32_t lo = 0, hi = jb.ntok;                                 // the last record with out_off <= first (record 0 starts at 0)
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (jb.toks[mid].out_off <= first) lo = mid; else hi = mid; }
        dd::Tok tk = jb.toks[lo];
        if (whole) {
            const uint32_t r = first - tk.out_off;
            if (r >= tk.hlen && (uint64_t)(r - tk.hlen) + 16u <= tk.lit) {
                const uint8_t *src = jb.in + tk.lit_src + (r - tk.hlen);
                const uintptr_t a = (uintptr_t)src & ~(uintptr_t)15;
                if (a >= r_lo && a + (((uintptr_t)src & 15u) ? 32u : 16u) <= r_hi) {
                    *reinterpret_cast<uint4 *>(dst) = load16_unaligned(src);
                    continue;
                }
            }
        }
        uint32_t b[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            b[j] = 0;
            if (p < 0 || (uint64_t)p >= total) continue;
            while (lo + 1 < jb.ntok && (uint64_t)p >= (uint64_t)tk.out_off + tk.hlen + tk.lit) tk = jb.toks[++lo];
            b[j] = dd_byte(jb, tk, (uint32_t)p);
            if (!whole) dst[j] = (uint8_t)b[j];
        }
        if (whole) {
            uint4 v;
            v.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            v.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            v.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            v.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
            *reinterpret_cast<uint4 *>(dst) = v;
        }
    }
}

// jobs + mail words of one call in the context's arena
struct PreCall {
    PreJob *d_jobs = nullptr;
    uint32_t *d_mail = nullptr;
};

int pre_upload(jpk_ctx *ctx, const std::vector<PreJob> &jobs, size_t mail_words, int mail_fill, PreCall *pc)
{
    Arena plan(ctx, true);
    plan.get<PreJob>(jobs.size());
    plan.get<uint32_t>(mail_words + 1);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    pc->d_jobs = real.get<PreJob>(jobs.size());
    pc->d_mail = real.get<uint32_t>(mail_words + 1);
    JPK_HIP(hipMemcpyAsync(pc->d_jobs, jobs.data(), jobs.size() * sizeof(PreJob), hipMemcpyHostToDevice, ctx->stream));
    if (mail_words) JPK_HIP(hipMemsetAsync(pc->d_mail, mail_fill, mail_words * 4, ctx->stream));
    return JPK_OK;
}

int pre_enter(jpk_ctx *ctx)
{
    if (!ctx) return JPK_E_ARG;
    JPK_HIP(hipSetDevice(ctx->device));
    return JPK_OK;
}

int pre_finish(jpk_ctx *ctx, const uint32_t *d_mail, std::vector<uint32_t> &mail)
{
    JPK_HIP(hipGetLastError());
    if (!mail.empty()) JPK_HIP(hipMemcpyAsync(mail.data(), d_mail, mail.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof_on) jpk_prof_resolve(ctx);
    return JPK_OK;
}

int pre_finish(jpk_ctx *ctx)
{
    std::vector<uint32_t> none;
    return pre_finish(ctx, nullptr, none);
}

// the per-block arguments of a batch entry (the array pointers themselves have been checked)
bool blocks_args_ok(int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap)
{
    for (int b = 0; b < n; b++)
        if (in_len[b] < 0 || out_cap[b] < 0 || (in_len[b] > 0 && !d_in[b]) || (out_cap[b] > 0 && !d_out[b])) return false;
    return true;
}

// the answer of a batch entry: per block in status[] when it is given one (stp == status), else the first status that is not JPK_OK
int finish_statuses(int32_t n, const int32_t *status, const int32_t *stp)
{
    if (status) return JPK_OK;
    for (int b = 0; b < n; b++) if (stp[b] != JPK_OK) return stp[b];
    return JPK_OK;
}

// The dedupe of n blocks in two halves around its one host read.  dd_find: table, heads, runs and selection of every block (in_len[b] < 0:
// skipped); s1_len[b] = |S1'|.  dd_emit: writes S1' of every block with outs[b] != nullptr.  The scratch lives in ctx's arena from dd_find
// until dd_emit has been enqueued; both synchronise the stream.
constexpr int DD_GRID_Y = 32768;
struct DdCall {
    std::vector<DdJob> jobs;
    DdJob *d_jobs = nullptr;
    uint32_t max_n = 0;
    uint64_t bytes = 0;
};

int dd_find(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *in_len, DdCall *dc, int32_t *s1_len)
{
    dc->jobs.assign((size_t)n, DdJob{});
    size_t table_words = 0, head_recs = 0, cnt_words = 0, tok_recs = 0;
    for (int b = 0; b < n; b++) {
        const uint32_t len = in_len[b] < 0 ? 0u : (uint32_t)in_len[b];
        table_words += (size_t)1 << dd::table_bits(len);
        head_recs += (size_t)dd::tiles(len) * dd::TILE_HEADS;
        cnt_words += jpk_align((size_t)dd::tiles(len), 4);
        tok_recs += dd::max_toks(len);
        if (len > dc->max_n) dc->max_n = len;
        dc->bytes += len;
    }
    Arena plan(ctx, true);
    plan.get<DdJob>((size_t)n);
    plan.get<uint32_t>(2 * (size_t)n);
    plan.get<uint32_t>(table_words);
    plan.get<uint4>(head_recs);
    plan.get<uint32_t>(cnt_words);
    plan.get<dd::Tok>(tok_recs);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    dc->d_jobs = real.get<DdJob>((size_t)n);
    uint32_t *d_mail = real.get<uint32_t>(2 * (size_t)n);
    uint32_t *tables = real.get<uint32_t>(table_words);
    uint4 *heads = real.get<uint4>(head_recs);
    uint32_t *cnts = real.get<uint32_t>(cnt_words);
    dd::Tok *toks = real.get<dd::Tok>(tok_recs);
    size_t to = 0, ho = 0, co = 0, ko = 0;
    for (int b = 0; b < n; b++) {
        const uint32_t len = in_len[b] < 0 ? 0u : (uint32_t)in_len[b];
        DdJob &j = dc->jobs[(size_t)b];
        j.in = len ? d_in[b] : nullptr; j.out = nullptr;
        j.table = tables + to; j.heads = heads + ho; j.cnt = cnts + co; j.toks = toks + ko;
        j.n = len; j.bits = dd::table_bits(len); j.total = 0; j.ntok = 0;
        to += (size_t)1 << j.bits; ho += (size_t)dd::tiles(len) * dd::TILE_HEADS; co += jpk_align((size_t)dd::tiles(len), 4); ko += dd::max_toks(len);
    }
    JPK_HIP(hipMemcpyAsync(dc->d_jobs, dc->jobs.data(), (size_t)n * sizeof(DdJob), hipMemcpyHostToDevice, ctx->stream));
    JPK_HIP(hipMemsetAsync(tables, 0xFF, table_words * 4, ctx->stream));
    const unsigned ntiles = dd::tiles(dc->max_n);
    for (int b0 = 0; b0 < n; b0 += DD_GRID_Y) {
        const unsigned nb = (unsigned)std::min(DD_GRID_Y, n - b0);
        const DdJob *jobs = dc->d_jobs + b0;
        if (ntiles) {
            JPK_LAUNCH(ctx, PROF_DD_ANCHOR, dc->bytes, k_dd_anchor, dim3(jpk_grid(dd::anchors(dc->max_n) + 1, PRE_TB), nb), dim3(PRE_TB), jobs);
            JPK_LAUNCH(ctx, PROF_DD_CAND, dc->bytes, k_dd_cand, dim3(ntiles, nb), dim3(PRE_TB), jobs);
            JPK_LAUNCH(ctx, PROF_DD_EXTEND, dc->bytes, k_dd_extend, dim3(jpk_grid((size_t)ntiles * dd::TILE_HEADS, PRE_TB), nb), dim3(PRE_TB), jobs);
        }
        JPK_LAUNCH(ctx, PROF_DD_SELECT, dc->bytes, k_dd_select, dim3(nb), dim3(PRE_TB), jobs, d_mail + 2 * (size_t)b0);
    }
    std::vector<uint32_t> mail(2 * (size_t)n);
    JPK_TRY(pre_finish(ctx, d_mail, mail));
    for (int b = 0; b < n; b++) {
        s1_len[b] = (int32_t)mail[2 * (size_t)b];
        dc->jobs[(size_t)b].ntok = mail[2 * (size_t)b + 1];
    }
    return JPK_OK;
}

int dd_emit(jpk_ctx *ctx, int n, DdCall *dc, uint8_t *const *outs, const int32_t *s1_len)
{
    uint64_t max_words = 0;
    for (int b = 0; b < n; b++) {
        DdJob &j = dc->jobs[(size_t)b];
        j.out = outs[b];
        j.total = outs[b] ? (uint32_t)s1_len[b] : 0u;
        if (j.total) max_words = std::max<uint64_t>(max_words, (((uintptr_t)j.out & 15u) + (uint64_t)j.total + 15u) / 16u);
    }
    if (max_words) {
        JPK_HIP(hipMemcpyAsync(dc->d_jobs, dc->jobs.data(), (size_t)n * sizeof(DdJob), hipMemcpyHostToDevice, ctx->stream));
        for (int b0 = 0; b0 < n; b0 += DD_GRID_Y)
            JPK_LAUNCH(ctx, PROF_DD_EMIT, dc->bytes, k_dd_emit, dim3(jpk_grid(max_words, WRAP_WORDS * PRE_TB), (unsigned)std::min(DD_GRID_Y, n - b0)), dim3(PRE_TB),
                       dc->d_jobs + b0);
    }
    return pre_finish(ctx);
}

}  // namespace

namespace {
// k_pre_lz77 on n blocks, one launch: stp[b] and out_len[b] as jpk_lz77_decompress gives them
int lz77_serial(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap, int32_t *out_len,
                int32_t *stp)
{
    std::vector<PreJob> jobs((size_t)n);
    uint64_t bytes = 0;
    for (int b = 0; b < n; b++) {
        jobs[(size_t)b] = PreJob{d_in[b], d_out[b], in_len[b], out_cap[b], (uint32_t)b, 0u};
        bytes += (uint32_t)in_len[b];
    }
    PreCall pc;
    JPK_TRY(pre_upload(ctx, jobs, 2 * (size_t)n, 0, &pc));
    JPK_LAUNCH(ctx, PROF_PRE_LZ77, bytes, k_pre_lz77, dim3((unsigned)n), dim3(PRE_TB), pc.d_jobs, pc.d_mail);
    std::vector<uint32_t> mail(2 * (size_t)n);
    JPK_TRY(pre_finish(ctx, pc.d_mail, mail));
    for (int b = 0; b < n; b++) {
        stp[b] = (int32_t)mail[2 * (size_t)b];
        out_len[b] = stp[b] == JPK_OK ? (int32_t)mail[2 * (size_t)b + 1] : 0;
    }
    return JPK_OK;
}
}  // namespace

extern "C" int jpk_dev_blocks_lz77_decompress(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                              const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    JPK_TRY(pre_enter(ctx));
    if (n < 0 || (n > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len))) return JPK_E_ARG;
    if (n == 0) return JPK_OK;
    if (!blocks_args_ok(n, d_in, in_len, d_out, out_cap)) return JPK_E_ARG;
    std::vector<int32_t> st_local((size_t)n);
    int32_t *stp = status ? status : st_local.data();
    JPK_TRY(lz77_serial(ctx, n, d_in, in_len, d_out, out_cap, out_len, stp));
    return finish_statuses(n, status, stp);
}

// The raw sizes of n blocks without their bytes: k_lz77_sizes in one launch, one read-back of the results.
extern "C" int jpk_dev_blocks_lz77_sizes(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, const int32_t *out_cap, int32_t *out_len,
                                         int32_t *status)
{
    if (!ctx || n < 0 || (n > 0 && (!d_in || !in_len || !out_cap || !out_len))) return JPK_E_ARG;
    for (int b = 0; b < n; b++)
        if (in_len[b] < 0 || out_cap[b] < 0 || (in_len[b] > 0 && !d_in[b])) return JPK_E_ARG;
    JPK_TRY(pre_enter(ctx));
    if (n == 0) return JPK_OK;
    std::vector<PreJob> jobs((size_t)n);
    uint64_t bytes = 0;
    for (int b = 0; b < n; b++) {
        jobs[(size_t)b] = PreJob{d_in[b], nullptr, in_len[b], out_cap[b], (uint32_t)b, 0u};
        bytes += (uint32_t)in_len[b];
    }
    PreCall pc;
    JPK_TRY(pre_upload(ctx, jobs, 2 * (size_t)n, 0, &pc));
    JPK_LAUNCH(ctx, PROF_LZ77_SIZES, bytes, k_lz77_sizes, dim3((unsigned)n), dim3(64), pc.d_jobs, pc.d_mail);
    std::vector<uint32_t> mail(2 * (size_t)n);
    JPK_TRY(pre_finish(ctx, pc.d_mail, mail));
    std::vector<int32_t> st_local((size_t)n);
    int32_t *stp = status ? status : st_local.data();
    for (int b = 0; b < n; b++) {
        stp[b] = (int32_t)mail[2 * (size_t)b];
        out_len[b] = stp[b] == JPK_OK ? (int32_t)mail[2 * (size_t)b + 1] : 0;
    }
    return finish_statuses(n, status, stp);
}

namespace {
// The same stage through a plan and a copy launch, and k_pre_lz77 for the blocks they leave to it: one host read of the plan's lengths and
// both kernels' flags, a second one only when a block went the serial way.  The records live in ctx's arena: lzx::seg_cap(in_len) per
// block, or lzx::deep_seg_cap(out_cap) with `deep` (k_lzd_plan + k_lzd_copy).  The arguments have been checked.  *par / *ser: the blocks
// that took either way.
int lz77_expand_run(jpk_ctx *ctx, bool deep, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap,
                    int32_t *out_len, int32_t *status, int32_t *par, int32_t *ser_n)
{
    *par = 0; *ser_n = 0;
    if (n == 0) return JPK_OK;
    std::vector<LzxJob> jobs((size_t)n);
    size_t seg_recs = 0;
    uint64_t bytes = 0, max_words = 0;
    for (int b = 0; b < n; b++) {
        const uint32_t cap = deep ? lzx::deep_seg_cap(out_cap[b]) : lzx::seg_cap(in_len[b]);
        jobs[(size_t)b] = LzxJob{d_in[b], d_out[b], nullptr, in_len[b], out_cap[b], cap, 0u};
        seg_recs += cap;
        bytes += (uint32_t)in_len[b];
        max_words = std::max<uint64_t>(max_words, (((uintptr_t)d_out[b] & 15u) + (uint64_t)out_cap[b] + 15u) / 16u);
    }
    Arena plan(ctx, true);
    plan.get<LzxJob>((size_t)n);
    plan.get<uint32_t>(LZX_INFO * (size_t)n);
    plan.get<lzx::Seg>(seg_recs);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    LzxJob *d_jobs = real.get<LzxJob>((size_t)n);
    uint32_t *d_info = real.get<uint32_t>(LZX_INFO * (size_t)n);
    lzx::Seg *segs = real.get<lzx::Seg>(seg_recs);
    size_t so = 0;
    for (int b = 0; b < n; b++) { jobs[(size_t)b].segs = segs + so; so += jobs[(size_t)b].cap; }
    JPK_HIP(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(LzxJob), hipMemcpyHostToDevice, ctx->stream));
    JPK_HIP(hipMemsetAsync(d_info, 0, LZX_INFO * (size_t)n * 4, ctx->stream));
    if (deep) JPK_LAUNCH(ctx, PROF_LZD_PLAN, bytes, k_lzd_plan, dim3((unsigned)n), dim3(64), d_jobs, d_info);
    else JPK_LAUNCH(ctx, PROF_LZX_PLAN, bytes, k_lzx_plan, dim3((unsigned)n), dim3(64), d_jobs, d_info);
    if (max_words)
        for (int b0 = 0; b0 < n; b0 += DD_GRID_Y) {
            const dim3 grid(jpk_grid(max_words, LZX_WORDS * PRE_TB), (unsigned)std::min(DD_GRID_Y, n - b0));
            if (deep) JPK_LAUNCH(ctx, PROF_LZD_COPY, bytes, k_lzd_copy, grid, dim3(PRE_TB), d_jobs + b0, d_info + LZX_INFO * (size_t)b0);
            else JPK_LAUNCH(ctx, PROF_LZX_COPY, bytes, k_lzx_copy, grid, dim3(PRE_TB), d_jobs + b0, d_info + LZX_INFO * (size_t)b0);
        }
    std::vector<uint32_t> info(LZX_INFO * (size_t)n);
    JPK_TRY(pre_finish(ctx, d_info, info));
    std::vector<int32_t> st_local((size_t)n);
    int32_t *stp = status ? status : st_local.data();
    std::vector<int> ser;
    for (int b = 0; b < n; b++) {
        const uint32_t *r = &info[LZX_INFO * (size_t)b];
        if (r[0] || r[3]) { ser.push_back(b); continue; }
        stp[b] = JPK_OK;
        out_len[b] = (int32_t)r[1];
    }
    if (!ser.empty()) {
        const size_t m = ser.size();
        std::vector<const uint8_t *> sin(m);
        std::vector<uint8_t *> sout(m);
        std::vector<int32_t> slen(m), scap(m), sgot(m), sst(m);
        for (size_t q = 0; q < m; q++) { sin[q] = d_in[ser[q]]; sout[q] = d_out[ser[q]]; slen[q] = in_len[ser[q]]; scap[q] = out_cap[ser[q]]; }
        JPK_TRY(lz77_serial(ctx, (int32_t)m, sin.data(), slen.data(), sout.data(), scap.data(), sgot.data(), sst.data()));
        for (size_t q = 0; q < m; q++) { stp[ser[q]] = sst[q]; out_len[ser[q]] = sgot[q]; }
    }
    *ser_n = (int32_t)ser.size();
    *par = n - *ser_n;
    return finish_statuses(n, status, stp);
}
}  // namespace

extern "C" int jpk_dev_blocks_lz77_expand(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                          const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    if (!ctx || n < 0 || (n > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len))) return JPK_E_ARG;
    if (!blocks_args_ok(n, d_in, in_len, d_out, out_cap)) return JPK_E_ARG;
    JPK_TRY(pre_enter(ctx));
    ctx->lzx_parallel = 0; ctx->lzx_serial = 0;
    return lz77_expand_run(ctx, false, n, d_in, in_len, d_out, out_cap, out_len, status, &ctx->lzx_parallel, &ctx->lzx_serial);
}

extern "C" int jpk_debug_lz77_expand_last(jpk_ctx *ctx, int32_t *parallel, int32_t *serial)
{
    if (!ctx || !parallel || !serial) return JPK_E_ARG;
    *parallel = ctx->lzx_parallel;
    *serial = ctx->lzx_serial;
    return JPK_OK;
}

// The deep expander behind its argument checks (the staged pass of jam_archive.hip calls it with job arrays of its own making)
int jpk_lz77_expand_deep_device(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out, const int32_t *out_cap,
                                int32_t *out_len, int32_t *status)
{
    JPK_TRY(pre_enter(ctx));
    ctx->lzd_parallel = 0; ctx->lzd_serial = 0;
    return lz77_expand_run(ctx, true, n, d_in, in_len, d_out, out_cap, out_len, status, &ctx->lzd_parallel, &ctx->lzd_serial);
}

extern "C" int jpk_dev_blocks_lz77_expand_deep(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                               const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    if (!ctx || n < 0 || (n > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len))) return JPK_E_ARG;
    if (!blocks_args_ok(n, d_in, in_len, d_out, out_cap)) return JPK_E_ARG;
    return jpk_lz77_expand_deep_device(ctx, n, d_in, in_len, d_out, out_cap, out_len, status);
}

extern "C" int jpk_debug_lz77_deep_last(jpk_ctx *ctx, int32_t *parallel, int32_t *serial)
{
    if (!ctx || !parallel || !serial) return JPK_E_ARG;
    *parallel = ctx->lzd_parallel;
    *serial = ctx->lzd_serial;
    return JPK_OK;
}

extern "C" int jpk_debug_lz77_deep_limits(int32_t *hops, int32_t *bytes_per_record, int32_t *slack)
{
    if (!hops || !bytes_per_record || !slack) return JPK_E_ARG;
    *hops = (int32_t)lzx::DEEP_CHASE;
    *bytes_per_record = (int32_t)lzx::DEEP_BYTES;
    *slack = (int32_t)lzx::DEEP_SLACK;
    return JPK_OK;
}

extern "C" int jpk_dev_blocks_lz77_dedupe(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                          const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    if (!ctx || n < 0 || (n > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len))) return JPK_E_ARG;
    if (!blocks_args_ok(n, d_in, in_len, d_out, out_cap)) return JPK_E_ARG;
    JPK_TRY(pre_enter(ctx));
    if (n == 0) return JPK_OK;
    DdCall dc;
    std::vector<int32_t> s1((size_t)n), st_local((size_t)n);
    std::vector<uint8_t *> outs((size_t)n);
    int32_t *stp = status ? status : st_local.data();
    JPK_TRY(dd_find(ctx, n, d_in, in_len, &dc, s1.data()));
    for (int b = 0; b < n; b++) {
        stp[b] = s1[(size_t)b] > out_cap[b] ? JPK_E_CAPACITY : JPK_OK;   // nothing of a block that does not fit is written
        outs[(size_t)b] = stp[b] == JPK_OK ? d_out[b] : nullptr;
        out_len[b] = stp[b] == JPK_OK ? s1[(size_t)b] : 0;
    }
    JPK_TRY(dd_emit(ctx, n, &dc, outs.data(), s1.data()));
    return finish_statuses(n, status, stp);
}

namespace {
// Lpx::Decode / Lpx::Encode of n blocks, one launch
int lpx_batch(jpk_ctx *ctx, bool encode, int32_t n, const uint8_t *const *d_in, const int32_t *len, uint8_t *const *d_out, int32_t *status)
{
    JPK_TRY(pre_enter(ctx));
    if (n < 0 || (n > 0 && (!d_in || !len || !d_out))) return JPK_E_ARG;
    if (n == 0) return JPK_OK;
    std::vector<PreJob> jobs((size_t)n);
    uint64_t wgs = 0, bytes = 0;
    for (int b = 0; b < n; b++) {
        if (len[b] < 0 || (len[b] > 0 && (!d_in[b] || !d_out[b]))) return JPK_E_ARG;
        jobs[(size_t)b] = PreJob{d_in[b], d_out[b], len[b], len[b], (uint32_t)wgs, 0u};
        wgs += pre::parts((uint32_t)len[b]);
        bytes += (uint32_t)len[b];
    }
    if (wgs > 0x7fffffffull) return JPK_E_ARG;
    if (wgs) {
        PreCall pc;
        JPK_TRY(pre_upload(ctx, jobs, 0, 0, &pc));
        if (encode) JPK_LAUNCH(ctx, PROF_ENC_LPX, bytes, k_lpx<true>, dim3((unsigned)wgs), dim3(PRE_TB), pc.d_jobs, (uint32_t)n, 0u);
        else JPK_LAUNCH(ctx, PROF_PRE_LPX, bytes, k_lpx<false>, dim3((unsigned)wgs), dim3(PRE_TB), pc.d_jobs, (uint32_t)n, 0u);
        JPK_TRY(pre_finish(ctx));
    }
    if (status) for (int b = 0; b < n; b++) status[b] = JPK_OK;      // any byte string is a valid stream / a valid input
    return JPK_OK;
}
}  // namespace

extern "C" int jpk_dev_blocks_lpx_decode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *len, uint8_t *const *d_out, int32_t *status)
{
    return lpx_batch(ctx, false, n, d_in, len, d_out, status);
}

extern "C" int jpk_dev_blocks_lpx_encode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *len, uint8_t *const *d_out, int32_t *status)
{
    return lpx_batch(ctx, true, n, d_in, len, d_out, status);
}

// The stage chain of jpk_cli_stages_encode_ex for n blocks in HBM: k_enc_wrap R -> S2 into d_mid[b] (jpk_cli_stages_bound - 2 bytes; d_mid
// == nullptr: in the context's arena), k_lpx<true> S2 -> S3 two bytes into d_out[b], with the second end token in front of it.
// in_len[b] < 0: the block is skipped.  The caller has checked that every jpk_cli_stages_bound fits its buffer and an int32.
// flags & JPK_CLI_DEDUPE: dd_find and dd_emit first, S1' into d_out[b] (|S1'| < |S4|: it fits), and k_enc_wrap reads S1' from there at the
// length the host has read; k_lpx<true> overwrites it behind k_enc_wrap in stream order.  s4_len[b] (nullable) = |S4|.
// flags & JPK_CLI_FILTERS: k_enc_filters, one workgroup per piece of S1, takes the place of k_enc_wrap on the same two sources.
namespace {
using pre::s4_of_s1;

// found != nullptr: dd_find has run for these blocks (its scratch is still in the arena) and found_s1[] holds its lengths
// lpx == false: the chain ends at S2 in d_mid[b] (staged frames), d_out[b] is the dedupe's room alone -- without the dedupe it is not
// read and may be null -- and s4_len[b] = |S2|
int cli_stages_run(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_mid, uint8_t *const *d_out, uint32_t flags,
                   int32_t *s4_len, DdCall *found, const int32_t *found_s1, bool lpx = true)
{
    const bool dedupe = (flags & JPK_CLI_DEDUPE) != 0, filters = (flags & JPK_CLI_FILTERS) != 0;
    std::vector<int32_t> s1((size_t)n);
    for (int b = 0; b < n; b++) s1[(size_t)b] = in_len[b] < 0 ? -1 : in_len[b] + 2;
    if (dedupe) {
        DdCall own;
        std::vector<uint8_t *> outs((size_t)n);
        for (int b = 0; b < n; b++) outs[(size_t)b] = in_len[b] < 0 ? nullptr : d_out[b];
        if (found) for (int b = 0; b < n; b++) s1[(size_t)b] = found_s1[b];
        else JPK_TRY(dd_find(ctx, n, d_in, in_len, &own, s1.data()));
        for (int b = 0; b < n; b++) if (in_len[b] < 0) s1[(size_t)b] = -1;
        JPK_TRY(dd_emit(ctx, n, found ? found : &own, outs.data(), s1.data()));
    }
    std::vector<PreJob> wj((size_t)n), lj((size_t)n);
    std::vector<size_t> moff((size_t)n, 0);
    size_t mid_bytes = 0;
    if (!d_mid)
        for (int b = 0; b < n; b++)
            if (in_len[b] >= 0) { moff[(size_t)b] = mid_bytes; mid_bytes += jpk_align((size_t)jpk_cli_stages_bound(in_len[b]) + 64); }
    Arena plan(ctx, true);
    plan.get<PreJob>(2 * (size_t)n);
    plan.get<uint8_t>(mid_bytes);
    JPK_TRY(jpk_arena_ensure(ctx, plan.need));
    Arena real(ctx, false);
    PreJob *d_jobs = real.get<PreJob>(2 * (size_t)n);
    uint8_t *mids = real.get<uint8_t>(mid_bytes);
    uint64_t wwg = 0, lwg = 0, bytes = 0;
    for (int b = 0; b < n; b++) {
        if (s4_len) s4_len[b] = in_len[b] < 0 ? 0 : (int32_t)s4_of_s1(s1[(size_t)b]) - (lpx ? 0 : 2);
        if (in_len[b] < 0) {
            wj[(size_t)b] = PreJob{nullptr, nullptr, 0, 0, (uint32_t)wwg, 0u};
            lj[(size_t)b] = PreJob{nullptr, nullptr, 0, 0, (uint32_t)lwg, 0u};
            continue;
        }
        const int32_t s2 = (int32_t)(s4_of_s1(s1[(size_t)b]) - 2);
        uint8_t *mid = d_mid ? d_mid[b] : mids + moff[(size_t)b];
        wj[(size_t)b] = dedupe ? PreJob{d_out[b], mid, s1[(size_t)b], s2, (uint32_t)wwg, 0u} : PreJob{d_in[b], mid, in_len[b], s2, (uint32_t)wwg, 0u};
        lj[(size_t)b] = PreJob{mid, lpx ? d_out[b] + 2 : nullptr, s2, s2, (uint32_t)lwg, 0u};
        const uint64_t words = (((uintptr_t)mid & 15u) + (uint64_t)s2 + 15u) / 16u;
        wwg += filters ? filter_pieces(s1[(size_t)b]) : (words + WRAP_WORDS * PRE_TB - 1) / (WRAP_WORDS * PRE_TB);
        lwg += pre::parts((uint32_t)s2);
        bytes += (uint32_t)s2;
    }
    if (wwg > 0x7fffffffull || lwg > 0x7fffffffull) return JPK_E_ARG;
    if (wwg) {
        JPK_HIP(hipMemcpyAsync(d_jobs, wj.data(), (size_t)n * sizeof(PreJob), hipMemcpyHostToDevice, ctx->stream));
        JPK_HIP(hipMemcpyAsync(d_jobs + n, lj.data(), (size_t)n * sizeof(PreJob), hipMemcpyHostToDevice, ctx->stream));
        if (filters && dedupe) JPK_LAUNCH(ctx, PROF_ENC_FILTERS, bytes, k_enc_filters<false>, dim3((unsigned)wwg), dim3(PRE_TB), d_jobs, (uint32_t)n);
        else if (filters) JPK_LAUNCH(ctx, PROF_ENC_FILTERS, bytes, k_enc_filters<true>, dim3((unsigned)wwg), dim3(PRE_TB), d_jobs, (uint32_t)n);
        else if (dedupe) JPK_LAUNCH(ctx, PROF_ENC_WRAP, bytes, k_enc_wrap<false>, dim3((unsigned)wwg), dim3(PRE_TB), d_jobs, (uint32_t)n);
        else JPK_LAUNCH(ctx, PROF_ENC_WRAP, bytes, k_enc_wrap<true>, dim3((unsigned)wwg), dim3(PRE_TB), d_jobs, (uint32_t)n);
        if (lpx) JPK_LAUNCH(ctx, PROF_ENC_LPX, bytes, k_lpx<true>, dim3((unsigned)lwg), dim3(PRE_TB), d_jobs + n, (uint32_t)n, 1u);
    }
    return pre_finish(ctx);
}
}  // namespace

int jpk_cli_stages_device(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_mid, uint8_t *const *d_out,
                          uint32_t flags, int32_t *s4_len)
{
    return cli_stages_run(ctx, n, d_in, in_len, d_mid, d_out, flags, s4_len, nullptr, nullptr);
}

int jpk_staged_stages_device(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_mid, uint8_t *const *d_tmp,
                             uint32_t flags, int32_t *s2_len)
{
    if (!d_mid) return JPK_E_ARG;
    return cli_stages_run(ctx, n, d_in, in_len, d_mid, d_tmp, flags, s2_len, nullptr, nullptr, false);
}

// With the dedupe a block's |S4| is known when its S1' is: dd_find for all blocks, the capacity answer, then the rest for those that fit
extern "C" int jpk_dev_blocks_cli_stages_encode_ex(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                                   const int32_t *out_cap, int32_t *out_len, int32_t *status, uint32_t flags)
{
    if (!ctx || n < 0 || (n > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len)) || !JPK_CLI_FLAGS_OK(flags)) return JPK_E_ARG;
    if (!blocks_args_ok(n, d_in, in_len, d_out, out_cap)) return JPK_E_ARG;
    for (int b = 0; b < n; b++) if (jpk_cli_stages_bound(in_len[b]) > 0x7fffffff) return JPK_E_ARG;
    JPK_TRY(pre_enter(ctx));
    if (n == 0) return JPK_OK;
    std::vector<int32_t> lens((size_t)n), st_local((size_t)n), s1((size_t)n);
    int32_t *stp = status ? status : st_local.data();
    DdCall dc;
    const bool dedupe = (flags & JPK_CLI_DEDUPE) != 0;
    if (dedupe) {
        // the lengths alone first: a block that does not fit must stay unwritten, and S1' is staged in its own output buffer
        JPK_TRY(dd_find(ctx, n, d_in, in_len, &dc, s1.data()));
    } else {
        for (int b = 0; b < n; b++) s1[(size_t)b] = in_len[b] + 2;
    }
    for (int b = 0; b < n; b++) {
        const int64_t total = s4_of_s1(s1[(size_t)b]);
        stp[b] = total > out_cap[b] ? JPK_E_CAPACITY : JPK_OK;        // nothing of a block that does not fit is written
        lens[(size_t)b] = stp[b] == JPK_OK ? in_len[b] : -1;
        out_len[b] = stp[b] == JPK_OK ? (int32_t)total : 0;
    }
    JPK_TRY(cli_stages_run(ctx, n, d_in, lens.data(), nullptr, d_out, flags, nullptr, dedupe ? &dc : nullptr, s1.data()));
    return finish_statuses(n, status, stp);
}

extern "C" int jpk_dev_blocks_cli_stages_encode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                                const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    return jpk_dev_blocks_cli_stages_encode_ex(ctx, n, d_in, in_len, d_out, out_cap, out_len, status, 0u);
}

// Filters::Encode of n blocks of S1 with the writer's choice, one launch; the lengths do not depend on the choice, so nothing is read back
extern "C" int jpk_dev_blocks_filters_encode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                             const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    JPK_TRY(pre_enter(ctx));
    if (n < 0 || (n > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len))) return JPK_E_ARG;
    if (n == 0) return JPK_OK;
    if (!blocks_args_ok(n, d_in, in_len, d_out, out_cap)) return JPK_E_ARG;
    std::vector<PreJob> jobs((size_t)n);
    std::vector<int32_t> st_local((size_t)n);
    int32_t *stp = status ? status : st_local.data();
    uint64_t wgs = 0, bytes = 0;
    for (int b = 0; b < n; b++) {
        const int64_t total = (int64_t)in_len[b] + 2 * (int64_t)filter_pieces(in_len[b]);
        if (total > 0x7fffffff) return JPK_E_ARG;
        stp[b] = total > out_cap[b] ? JPK_E_CAPACITY : JPK_OK;         // nothing of a block that does not fit is written
        out_len[b] = stp[b] == JPK_OK ? (int32_t)total : 0;
        jobs[(size_t)b] = stp[b] == JPK_OK ? PreJob{d_in[b], d_out[b], in_len[b], (int32_t)total, (uint32_t)wgs, 0u} : PreJob{nullptr, nullptr, 0, 0, (uint32_t)wgs, 0u};
        if (stp[b] == JPK_OK) { wgs += filter_pieces(in_len[b]); bytes += (uint32_t)in_len[b]; }
    }
    if (wgs > 0x7fffffffull) return JPK_E_ARG;
    if (wgs) {
        PreCall pc;
        JPK_TRY(pre_upload(ctx, jobs, 0, 0, &pc));
        JPK_LAUNCH(ctx, PROF_ENC_FILTERS, bytes, k_enc_filters<false>, dim3((unsigned)wgs), dim3(PRE_TB), pc.d_jobs, (uint32_t)n);
        JPK_TRY(pre_finish(ctx));
    }
    return finish_statuses(n, status, stp);
}

extern "C" int jpk_dev_blocks_filters_decode(jpk_ctx *ctx, int32_t n, const uint8_t *const *d_in, const int32_t *in_len, uint8_t *const *d_out,
                                             const int32_t *out_cap, int32_t *out_len, int32_t *status)
{
    JPK_TRY(pre_enter(ctx));
    if (n < 0 || (n > 0 && (!d_in || !in_len || !d_out || !out_cap || !out_len))) return JPK_E_ARG;
    if (n == 0) return JPK_OK;
    if (!blocks_args_ok(n, d_in, in_len, d_out, out_cap)) return JPK_E_ARG;
    std::vector<PreJob> jobs((size_t)n);
    std::vector<uint32_t> nfb((size_t)n);
    uint64_t wgs = 0, bytes = 0;
    for (int b = 0; b < n; b++) {
        jobs[(size_t)b] = PreJob{d_in[b], d_out[b], in_len[b], out_cap[b], (uint32_t)wgs, 0u};
        nfb[(size_t)b] = pre::filter_blocks(in_len[b]);
        wgs += nfb[(size_t)b];
        bytes += (uint32_t)in_len[b];
    }
    if (wgs > 0x7fffffffull) return JPK_E_ARG;
    std::vector<uint32_t> mail((size_t)n, 0xFFFFFFFFu);
    if (wgs) {
        PreCall pc;
        JPK_TRY(pre_upload(ctx, jobs, (size_t)n, 0xFF, &pc));
        JPK_LAUNCH(ctx, PROF_PRE_FILTERS, bytes, k_pre_filters, dim3((unsigned)wgs), dim3(PRE_TB), pc.d_jobs, (uint32_t)n, pc.d_mail);
        JPK_TRY(pre_finish(ctx, pc.d_mail, mail));
    }
    std::vector<int32_t> st_local((size_t)n);
    int32_t *stp = status ? status : st_local.data();
    for (int b = 0; b < n; b++) {
        const uint32_t m = mail[(size_t)b];
        stp[b] = m == 0xFFFFFFFFu ? JPK_OK : ((m & 1u) ? JPK_E_CAPACITY : JPK_E_CORRUPT);
        out_len[b] = stp[b] == JPK_OK ? in_len[b] - 2 * (int32_t)nfb[(size_t)b] : 0;
    }
    return finish_statuses(n, status, stp);
}
