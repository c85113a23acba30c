// jam_archive.hip -- whole .jam archives of the C ABI (include/jampack_abi.h): the frame walks, the batched compress and decompress
// calls of plain and stock-CLI archives with their host-buffer forms, the index + range reads, and the index, the salvage and the repair of damaged
// archives (the rule they share with the kernels: jam_resync.hpp), and the update of byte ranges (its plan: jam_update_plan.hpp).  Host drivers only: the kernels
// are in jam.hip, prestage_dev.hip and checksum.hip, the batch engines in abi_blocks.hip and the context pool in abi_pool.hip.
#include <algorithm>
#include <atomic>
#include <new>
#include <vector>

#include "common.hpp"
#include "jam_resync.hpp"
#include "jam_update_plan.hpp"

// ---- whole .jam archives: Jampack::Compress / Jampack::Decompress (jampack.cpp:186-336) through the batch engines --------------
// Compress, per pass (jam_compress_frames, the form the update shares: a pointer, a length, a BlockSize and a kind per frame): one batched
// checksum of the pass's slices (the crcs stay on the device for the pack and come to the host for an index), jpk_dev_blocks_compress into payload slots
// in ctx->jam_scratch, the frame offsets on the host (64-bit), one k_jam_pack launch that writes the frames.  Decompress: the frame
// walk (k_jam_walk, one launch + one read-back per JPK_JAM_PASS_FRAMES frames) and the decoded sizes (pass 1 of the batch decoder)
// over the whole archive first -- that is what makes the capacity answer exact and leaves d_out untouched when it is too small --
// then per pass jpk_dev_blocks_decompress with every frame decoded in place in d_out (its payload read in place in the archive),
// one batched checksum of the outputs, and the comparison with the header crcs (jam_plain_group; the pass loop is jam_decode, which
// the stock-CLI and the staged archives share: a plain archive is its pass without a chained frame).  A pass holds at most JPK_JAM_PASS_FRAMES frames
// and JAM_PASS_RAW raw bytes, which bounds the scratch of both directions for archives of any length.
// The stock-CLI writer (jpk_dev_jam_cli_compress) is the same pass with the stage chain in front of the batch compress: k_enc_wrap from
// the raw slices into a slot A per frame, k_enc_lpx from A into a slot B, and the B slots are the batch's inputs; the crcs stay those
// of the raw slices.  With JPK_CLI_DEDUPE the k_dd_* launches come first (raw slice -> S1' in slot B), the pass's S1' lengths are read
// on the host once, and the batch's input lengths are those of the S4 that k_enc_wrap / k_enc_lpx then make of them.  With JPK_CLI_FILTERS
// k_enc_filters stands where k_enc_wrap does; the lengths are the same.
// The writer of staged frames (jpk_dev_jam_staged_compress; DESIGN 4.6, "Staged frames") is that pass with the chain stopped at S2: no k_enc_lpx,
// the A slots are the batch's inputs, and the pack writes BlockSize | JPK_JAM_STAGED.  Its reader takes plain and staged frames in one archive.

// (JamFrame, one frame of an archive as the walks see it, and the checks a walk applies to it: jam_resync.hpp)

namespace {
constexpr uint64_t JAM_PASS_RAW = 4ull << 30;
// what an archive call reads or writes: plain frames, frames of the stock CLI, or (reading) plain and staged frames in any order
constexpr int JAM_PLAIN = 0, JAM_CLI = 1, JAM_STAGED = 2;

int jam_pass_frames(int32_t block_size)
{
    const uint64_t k = JAM_PASS_RAW / (uint64_t)block_size;
    return k < (uint64_t)JPK_JAM_PASS_FRAMES ? (int)k : JPK_JAM_PASS_FRAMES;
}

// the slots of a frame that goes through pre-stage decoders: the reference's stage buffers, 1.05 x BlockSize + 4096 (jampack.cpp:156)
int32_t jam_cli_cap(int32_t block_size) { return jrs::cli_cap(block_size); }

// host walk of an archive in host memory: the frames in front of the first bad one (*bad = its index, -1: none) -- a bad header (1..14
// trailing bytes are one), bad chunk headers in the payload, or a payload that declares too much (jrs::frame_at); JAM_CLI: frames of the
// stock CLI, f.raw = the entropy-decoded bytes (the input of the pre-stage decoders), and so for the staged frames of JAM_STAGED
void jam_walk_host(const uint8_t *in, int64_t in_len, std::vector<JamFrame> &fr, int32_t *bad, int kind = JAM_PLAIN)
{
    *bad = -1;
    int64_t o = 0;
    while (o < in_len) {
        JamFrame f;
        if (!jrs::frame_at(in, in_len, o, kind == JAM_STAGED, kind == JAM_CLI, &f)) { *bad = (int32_t)fr.size(); return; }
        fr.push_back(f);
        o = f.payload_off + f.psize;
    }
}

// a header the walk kernel or the scan found, with the status and the bytes of its payload from jpk_ans_decoded_sizes: the frame as the
// host walk gives it, or false -- the payload has bad chunk headers or declares too much (cli: measured against the slot of a chained frame)
bool jam_frame_of(const JamWalkFrame &w, int32_t st, int64_t dec, bool cli, JamFrame *f)
{
    const bool staged = (w.block_size & JPK_JAM_STAGED) != 0;       // (only a walk or a scan with staged_ok lets such a field through)
    const int32_t bs = w.block_size & ~JPK_JAM_STAGED;
    if (st != JPK_OK || !jrs::decoded_ok(dec, bs, cli || staged)) return false;
    *f = JamFrame{(int64_t)w.payload_off, w.psize, w.crc, bs, dec - JPK_TRAILER_BYTES, staged};
    return true;
}

// the same walk of an archive in HBM: k_jam_walk per JPK_JAM_PASS_FRAMES frames, then their decoded sizes in one launch.  It starts at
// offset `start`; *stop (nullable) = the offset of the frame it stopped at, in_len when it reached the end
int jam_walk_dev(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, std::vector<JamFrame> &fr, int32_t *bad, int kind = JAM_PLAIN, int64_t start = 0,
                 int64_t *stop = nullptr)
{
    *bad = -1;
    if (stop) *stop = in_len;
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->jam_scratch, &ctx->jam_scratch_cap, (size_t)JPK_JAM_PASS_FRAMES * sizeof(JamWalkFrame)));
    JamWalkFrame *d_tab = reinterpret_cast<JamWalkFrame *>(ctx->jam_scratch);
    std::vector<JamWalkFrame> h(JPK_JAM_PASS_FRAMES);
    std::vector<const uint8_t *> ins;
    std::vector<int32_t> lens, st;
    std::vector<int64_t> dec;
    uint64_t o = (uint64_t)start;
    while (o < (uint64_t)in_len) {
        JPK_TRY(jpk_jam_walk_enqueue(ctx, d_in, (uint64_t)in_len, o, JPK_JAM_PASS_FRAMES, d_tab, ctx->d_mail->read, kind == JAM_STAGED));
        JPK_HIP(hipMemcpyAsync(h.data(), d_tab, h.size() * sizeof(JamWalkFrame), hipMemcpyDeviceToHost, ctx->stream));
        uint32_t m[4];
        JPK_TRY(jpk_read_mail(ctx, m, 4));                   // synchronises: the table is on the host too
        const int n = (int)m[0];
        ins.resize((size_t)n); lens.resize((size_t)n); st.resize((size_t)n); dec.resize((size_t)n);
        for (int i = 0; i < n; i++) { ins[i] = d_in + h[i].payload_off; lens[i] = h[i].psize; }
        JPK_TRY(jpk_ans_decoded_sizes(ctx, n, ins.data(), lens.data(), dec.data(), st.data()));
        for (int i = 0; i < n; i++) {
            JamFrame f;
            if (!jam_frame_of(h[i], st[i], dec[i], kind == JAM_CLI, &f)) {
                *bad = (int32_t)fr.size();
                if (stop) *stop = (int64_t)h[i].payload_off - JPK_JAM_HEADER_BYTES;
                return JPK_OK;
            }
            fr.push_back(f);
        }
        o = ((uint64_t)m[3] << 32) | m[2];
        if (m[1]) { *bad = (int32_t)fr.size(); if (stop) *stop = (int64_t)o; return JPK_OK; }
    }
    return JPK_OK;
}

// items [k, e) of n form the pass that starts at item k: at most JPK_JAM_PASS_FRAMES of them and JAM_PASS_RAW bytes of weight(i) in
// all (one item at least)
template <class W> size_t jam_pass_end(size_t n, size_t k, W weight)
{
    size_t e = k;
    uint64_t sum = 0;
    while (e < n && e - k < (size_t)JPK_JAM_PASS_FRAMES && (e == k || sum + (uint64_t)weight(e) <= JAM_PASS_RAW)) sum += (uint64_t)weight(e++);
    return e;
}

// what a frame weighs in a decompress pass and in the size answers: its raw bytes, or (cli: known only behind its last stage) its BlockSize
int64_t jam_weight(const JamFrame &f, bool cli) { return (cli || f.staged) ? f.block_size : f.raw; }
size_t jam_pass_end(const std::vector<JamFrame> &fr, size_t k, bool cli)
{
    return jam_pass_end(fr.size(), k, [&](size_t i) { return jam_weight(fr[i], cli); });
}
int64_t jam_sum(const std::vector<JamFrame> &fr, size_t k, size_t e, bool cli)
{
    int64_t sum = 0;
    for (size_t i = k; i < e; i++) sum += jam_weight(fr[i], cli);
    return sum;
}

// the crcs of n device segments on the host: one batched checksum into d_crc, one read-back, synchronised
int jam_crcs(jpk_ctx *ctx, int n, const uint8_t *const *d_in, const int32_t *len, uint32_t *d_crc, uint32_t *crc)
{
    JPK_TRY(jpk_checksums_device(ctx, n, d_in, len, d_crc));
    JPK_HIP(hipMemcpyAsync(crc, d_crc, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    return JPK_OK;
}

// appends the piece src[0..len) -> dst (readable around src: [lo, hi)) to tab; *words = the destination words of the pieces so far
void jam_piece_add(std::vector<JamGatherPiece> &tab, uint64_t *words, const uint8_t *src, uint8_t *dst, uint64_t len, const uint8_t *lo, const uint8_t *hi)
{
    tab.push_back(JamGatherPiece{src, dst, len, *words, lo, hi});
    *words += (((uint64_t)(uintptr_t)dst & 15u) + len + 15u) / 16u;
}

// delivers the pieces of tab (through d_tab) with one launch, synchronised
int jam_gather(jpk_ctx *ctx, JamGatherPiece *d_tab, const std::vector<JamGatherPiece> &tab, uint64_t words, uint64_t bytes)
{
    if (tab.empty()) return JPK_OK;
    JPK_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(JamGatherPiece), hipMemcpyHostToDevice, ctx->stream));
    JPK_TRY(jpk_jam_gather_enqueue(ctx, d_tab, (uint32_t)tab.size(), words, bytes));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    return JPK_OK;
}

// what the decompress entries report.  zero: on entry; stop: frame f failed with rc, len verified bytes in front of it; done: every
// frame the walk found is out, and a walk that stopped at a bad frame makes the call JPK_E_CORRUPT
struct JamResult { int64_t *out_len; int32_t *frames, *bad_frame; };
void jam_result_zero(const JamResult &r)
{
    *r.out_len = 0;
    if (r.frames) *r.frames = 0;
    if (r.bad_frame) *r.bad_frame = -1;
}
int jam_result_stop(const JamResult &r, int64_t len, int32_t f, int rc)
{
    *r.out_len = len;
    if (r.frames) *r.frames = f;
    if (r.bad_frame) *r.bad_frame = f;
    return rc;
}
int jam_result_done(const JamResult &r, int64_t len, size_t frames, int32_t bad)
{
    *r.out_len = len;
    if (r.frames) *r.frames = (int32_t)frames;
    if (bad < 0) return JPK_OK;
    if (r.bad_frame) *r.bad_frame = bad;
    return JPK_E_CORRUPT;
}

// what the batch compress is given for a raw slice of len bytes: the slice, or its S4 (cli; prestage.cpp) -- and the payload it can give
int32_t jam_bwt_len(int32_t len, bool cli) { return cli ? (int32_t)jpk_cli_stages_bound(len) : len; }
int64_t jam_frame_bound(int32_t len, bool cli) { return JPK_JAM_HEADER_BYTES + (int64_t)jpk_multi_comp_cap(jam_bwt_len(len, cli)); }

// One frame of a compress pass: its raw bytes, wherever they lie in HBM, the BlockSize it is written under and its kind (JAM_PLAIN,
// JAM_CLI or JAM_STAGED) -- and what the pass makes of it: the payload slot in ctx->jam_scratch (at least 16 readable bytes behind the
// payload: the aligned loads of k_jam_pack and k_jam_splice), the payload's size and the crc of the raw bytes
struct JamNewFrame { const uint8_t *in; int32_t len; int32_t block_size; int kind; };
struct JamPayload { const uint8_t *slot; int32_t psize; uint32_t crc; };

// The compress pass in its general form: n <= JPK_JAM_PASS_FRAMES frames, each with a pointer, a length, a BlockSize and a kind of its
// own.  One batched checksum of the raw frames (jampack.cpp:31; the crcs stay in the first n words of ctx->jam_scratch and come to the host
// too), the stage chain of the stock-CLI frames and that of the staged ones -- S2 in slot A is a staged frame's BWT input, S4 in slot B a
// stock-CLI frame's; slot B is also the dedupe's room --, then ONE batch compress of all frames into their payload slots.  *table = room
// for JPK_JAM_PASS_FRAMES JamPackFrame entries in the scratch, the caller's.  Synchronised.
int jam_compress_frames(jpk_ctx *ctx, const std::vector<JamNewFrame> &fr, uint32_t flags, int32_t in_flight, std::vector<JamPayload> &made, uint8_t **table)
{
    const size_t n = fr.size();
    std::vector<const uint8_t *> ins(n), bwt_in(n);
    std::vector<uint8_t *> slots(n), sa(n, nullptr), sb(n, nullptr);
    std::vector<int32_t> lens(n), blens(n), caps(n), outl(n), st(n);
    const size_t o_frames = jpk_align((size_t)JPK_JAM_PASS_FRAMES * 4), o_slots = o_frames + jpk_align((size_t)JPK_JAM_PASS_FRAMES * sizeof(JamPackFrame));
    auto slot_b = [flags](int kind) { return kind == JAM_CLI || (kind == JAM_STAGED && (flags & JPK_CLI_DEDUPE) != 0); };
    size_t need = o_slots;
    for (size_t i = 0; i < n; i++) {
        const bool cli = fr[i].kind != JAM_PLAIN;
        ins[i] = fr[i].in;
        lens[i] = fr[i].len;
        blens[i] = jam_bwt_len(lens[i], cli);
        caps[i] = (int32_t)jpk_multi_comp_cap(blens[i]);
        need += jpk_align((size_t)caps[i] + 64);          // (>= 16 bytes behind every payload: k_jam_pack's aligned loads)
        if (cli) need += (slot_b(fr[i].kind) ? 2 : 1) * jpk_align((size_t)blens[i] + 64);     // slot A (S2) and slot B (S4)
    }
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->jam_scratch, &ctx->jam_scratch_cap, need));
    uint32_t *d_crc = reinterpret_cast<uint32_t *>(ctx->jam_scratch);
    *table = ctx->jam_scratch + o_frames;
    size_t off = o_slots;
    for (size_t i = 0; i < n; i++) {
        slots[i] = ctx->jam_scratch + off; off += jpk_align((size_t)caps[i] + 64);
        bwt_in[i] = ins[i];
        if (fr[i].kind != JAM_PLAIN) {
            sa[i] = ctx->jam_scratch + off; off += jpk_align((size_t)blens[i] + 64);
            if (slot_b(fr[i].kind)) { sb[i] = ctx->jam_scratch + off; off += jpk_align((size_t)blens[i] + 64); }
            bwt_in[i] = fr[i].kind == JAM_STAGED ? sa[i] : sb[i];
        }
    }
    // crcs of the inputs (jampack.cpp:31) first, in stream order in front of the batch (its workers wait for ctx's stream)
    std::vector<uint32_t> crc(n);
    JPK_TRY(jam_crcs(ctx, (int)n, ins.data(), lens.data(), d_crc, crc.data()));
    // the stage chain of one kind: its frames side by side, their BWT inputs' lengths back into blens
    for (int kind : {JAM_CLI, JAM_STAGED}) {
        std::vector<size_t> at;
        std::vector<const uint8_t *> kin;
        std::vector<uint8_t *> ka, kb;
        std::vector<int32_t> klen;
        for (size_t i = 0; i < n; i++)
            if (fr[i].kind == kind) { at.push_back(i); kin.push_back(ins[i]); klen.push_back(lens[i]); ka.push_back(sa[i]); kb.push_back(sb[i]); }
        if (at.empty()) continue;
        std::vector<int32_t> got(at.size());
        if (kind == JAM_CLI) JPK_TRY(jpk_cli_stages_device(ctx, (int)at.size(), kin.data(), klen.data(), ka.data(), kb.data(), flags, got.data()));
        else JPK_TRY(jpk_staged_stages_device(ctx, (int)at.size(), kin.data(), klen.data(), ka.data(), kb.data(), flags, got.data()));
        for (size_t q = 0; q < at.size(); q++) blens[at[q]] = got[q];
    }
    JPK_TRY(jpk_dev_blocks_compress(ctx, (int)n, bwt_in.data(), blens.data(), slots.data(), caps.data(), outl.data(), st.data(), in_flight));
    for (size_t i = 0; i < n; i++) if (st[i] != JPK_OK) return st[i];
    made.resize(n);
    for (size_t i = 0; i < n; i++) made[i] = JamPayload{slots[i], outl[i], crc[i]};
    return JPK_OK;
}

// one compress pass of the whole-archive writers: consecutive block_size slices of d_in[0..len) (the last one short), all of one kind ->
// frames at d_out[0..*pass_len) through one k_jam_pack launch.  done (nullable) receives the frames as an index holds them, payload_off
// counted from the pass's first byte
int jam_compress_pass(jpk_ctx *ctx, const uint8_t *d_in, int64_t len, int32_t block_size, uint8_t *d_out, int64_t out_room, int64_t *pass_len,
                      int32_t in_flight, int kind, uint32_t flags, std::vector<JamFrame> *done = nullptr)
{
    const int n = (int)((len + block_size - 1) / block_size);
    std::vector<JamNewFrame> in((size_t)n);
    for (int i = 0; i < n; i++) in[i] = JamNewFrame{d_in + (int64_t)i * block_size, (int32_t)std::min<int64_t>(block_size, len - (int64_t)i * block_size), block_size, kind};
    std::vector<JamPayload> made;
    uint8_t *table = nullptr;
    JPK_TRY(jam_compress_frames(ctx, in, flags, in_flight, made, &table));
    std::vector<JamPackFrame> fr((size_t)n);
    uint64_t pos = 0;
    for (int i = 0; i < n; i++) {
        fr[i].slot = made[i].slot; fr[i].off = pos; fr[i].psize = made[i].psize; fr[i].pad = 0;
        pos += (uint64_t)JPK_JAM_HEADER_BYTES + (uint64_t)made[i].psize;
    }
    if ((int64_t)pos > out_room) return JPK_E_CAPACITY;
    JamPackFrame *d_frames = reinterpret_cast<JamPackFrame *>(table);
    JPK_HIP(hipMemcpyAsync(d_frames, fr.data(), (size_t)n * sizeof(JamPackFrame), hipMemcpyHostToDevice, ctx->stream));
    JPK_TRY(jpk_jam_pack_enqueue(ctx, d_frames, n, reinterpret_cast<const uint32_t *>(ctx->jam_scratch), kind == JAM_STAGED ? (block_size | JPK_JAM_STAGED) : block_size,
                                 d_out, pos));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    if (done)
        for (int i = 0; i < n; i++)
            done->push_back(JamFrame{(int64_t)fr[i].off + JPK_JAM_HEADER_BYTES, made[i].psize, made[i].crc, block_size, in[i].len, kind == JAM_STAGED});
    *pass_len = (int64_t)pos;
    return JPK_OK;
}
}  // namespace

namespace {
int64_t jam_compress_bound(int64_t in_len, int32_t block_size, bool cli)
{
    if (in_len < 0 || !jpk_jam_block_size_ok(block_size)) return JPK_E_ARG;
    const int64_t full = in_len / block_size, rest = in_len % block_size;
    return full * jam_frame_bound(block_size, cli) + (rest ? jam_frame_bound((int32_t)rest, cli) : 0);
}

int jam_compress_dev(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                     int32_t in_flight, int kind, uint32_t flags = 0u)
{
    // (JPK_ENTER taken apart: the argument checks come before the first device call)
    if (!ctx || !out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && (!d_in || !d_out)) || !JPK_CLI_FLAGS_OK(flags)) return JPK_E_ARG;
    if (!jpk_jam_block_size_ok(block_size)) return JPK_E_ARG;                     // InitComp, jampack.cpp:70
    JPK_HIP(hipSetDevice(ctx->device));
    *out_len = 0;
    const int64_t step = (int64_t)jam_pass_frames(block_size) * block_size;
    int64_t pos = 0;
    for (int64_t o = 0; o < in_len; o += step) {
        int64_t n = 0;
        JPK_TRY(jam_compress_pass(ctx, d_in + o, std::min(step, in_len - o), block_size, d_out + pos, out_cap - pos, &n, in_flight, kind, flags));
        pos += n;
    }
    *out_len = pos;
    return JPK_OK;
}
}  // namespace

extern "C" int64_t jpk_jam_compress_bound(int64_t in_len, int32_t block_size) { return jam_compress_bound(in_len, block_size, false); }
extern "C" int64_t jpk_jam_cli_compress_bound(int64_t in_len, int32_t block_size) { return jam_compress_bound(in_len, block_size, true); }
extern "C" int64_t jpk_jam_staged_compress_bound(int64_t in_len, int32_t block_size) { return jam_compress_bound(in_len, block_size, true); }

extern "C" int jpk_dev_jam_compress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                    int32_t in_flight)
{
    return jam_compress_dev(ctx, d_in, in_len, block_size, d_out, out_cap, out_len, in_flight, JAM_PLAIN);
}

extern "C" int jpk_dev_jam_cli_compress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap,
                                        int64_t *out_len, int32_t in_flight)
{
    return jam_compress_dev(ctx, d_in, in_len, block_size, d_out, out_cap, out_len, in_flight, JAM_CLI);
}

extern "C" int jpk_dev_jam_cli_compress_ex(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap,
                                           int64_t *out_len, int32_t in_flight, uint32_t flags)
{
    return jam_compress_dev(ctx, d_in, in_len, block_size, d_out, out_cap, out_len, in_flight, JAM_CLI, flags);
}

extern "C" int jpk_dev_jam_staged_compress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t block_size, uint8_t *d_out, int64_t out_cap,
                                           int64_t *out_len, int32_t in_flight, uint32_t flags)
{
    return jam_compress_dev(ctx, d_in, in_len, block_size, d_out, out_cap, out_len, in_flight, JAM_STAGED, flags);
}

namespace {
// jpk_jam_frames / jpk_jam_cli_frames: the host walk, *len = the raw bytes (cli: the sum of BlockSize) of the frames it found
int jam_frames(const uint8_t *in, int64_t in_len, int32_t *frames, int64_t *len, int32_t *bad_frame, int kind)
{
    const bool cli = kind == JAM_CLI;
    if (in_len < 0 || (in_len > 0 && !in)) return JPK_E_ARG;
    std::vector<JamFrame> fr;
    int32_t bad = -1;
    jam_walk_host(in, in_len, fr, &bad, kind);
    if (frames) *frames = (int32_t)fr.size();
    if (len) *len = jam_sum(fr, 0, fr.size(), cli);
    if (bad_frame) *bad_frame = bad;
    return bad >= 0 ? JPK_E_CORRUPT : JPK_OK;
}

int jam_compress_host(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight, int kind,
                      uint32_t flags = 0u)
{
    const bool cli = kind != JAM_PLAIN;
    if (!out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && (!in || !out)) || !JPK_CLI_FLAGS_OK(flags)) return JPK_E_ARG;
    if (!jpk_jam_block_size_ok(block_size)) return JPK_E_ARG;
    *out_len = 0;
    jpk_ctx *ctx;
    JPK_TRY(jpk_host_enter(&ctx, 0));
    // staged one pass at a time: the device call makes the same passes, so the frames are those of one call over the whole input
    const int64_t step = (int64_t)jam_pass_frames(block_size) * block_size;
    int64_t pos = 0;
    for (int64_t o = 0; o < in_len; o += step) {
        const int64_t len = std::min(step, in_len - o), bound = jam_compress_bound(len, block_size, cli);
        JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_in, &ctx->stage_in_cap, (size_t)len + 64));
        JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_res, &ctx->stage_res_cap, (size_t)bound + 64));
        JPK_HIP(hipMemcpyAsync(ctx->stage_in, in + o, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
        int64_t n = 0;
        JPK_TRY(jam_compress_dev(ctx, ctx->stage_in, len, block_size, ctx->stage_res, bound, &n, in_flight, kind, flags));
        if (n > out_cap - pos) return JPK_E_CAPACITY;
        JPK_HIP(hipMemcpyAsync(out + pos, ctx->stage_res, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        JPK_HIP(hipStreamSynchronize(ctx->stream));
        pos += n;
    }
    *out_len = pos;
    return JPK_OK;
}
}  // namespace

extern "C" int jpk_jam_frames(const uint8_t *in, int64_t in_len, int32_t *frames, int64_t *raw_len, int32_t *bad_frame)
{
    return jam_frames(in, in_len, frames, raw_len, bad_frame, JAM_PLAIN);
}

extern "C" int jpk_jam_cli_frames(const uint8_t *in, int64_t in_len, int32_t *frames, int64_t *raw_bound, int32_t *bad_frame)
{
    return jam_frames(in, in_len, frames, raw_bound, bad_frame, JAM_CLI);
}

extern "C" int jpk_jam_staged_frames(const uint8_t *in, int64_t in_len, int32_t *frames, int64_t *raw_bound, int32_t *bad_frame)
{
    return jam_frames(in, in_len, frames, raw_bound, bad_frame, JAM_STAGED);
}

extern "C" int jpk_jam_staged_compress(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight,
                                       uint32_t flags)
{
    return jam_compress_host(in, in_len, block_size, out, out_cap, out_len, in_flight, JAM_STAGED, flags);
}

extern "C" int jpk_jam_compress(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight)
{
    return jam_compress_host(in, in_len, block_size, out, out_cap, out_len, in_flight, JAM_PLAIN);
}

extern "C" int jpk_jam_cli_compress(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight)
{
    return jam_compress_host(in, in_len, block_size, out, out_cap, out_len, in_flight, JAM_CLI);
}

extern "C" int jpk_jam_cli_compress_ex(const uint8_t *in, int64_t in_len, int32_t block_size, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t in_flight,
                                       uint32_t flags)
{
    return jam_compress_host(in, in_len, block_size, out, out_cap, out_len, in_flight, JAM_CLI, flags);
}

// the frame table behind jpk_jam_index (the range reads below; the stock-CLI calls make one from what they decode)
struct jpk_jam_index {
    std::vector<JamFrame> fr;
    std::vector<int64_t> raw_off;      // fr.size() + 1 entries: raw_off[k] = the raw bytes in front of frame k, the last one = raw_len
    int64_t archive_len = 0;
    int32_t bad = -1;
    int32_t kind = JPK_JAM_INDEX_PLAIN;    // JPK_JAM_INDEX_CLI: frames of the stock CLI, fr[k].raw from a decode (jam_decode)
                                           // JPK_JAM_INDEX_STAGED: plain and staged frames (fr[k].staged), a staged one's raw from its token walk or a decode
    // what a recovered index skipped (jpk_(dev_)jam_index_recover), in archive order: `frame` recovered frames lie in front of the gap; with
    // the frames' spans [payload_off - 15, payload_off + psize) the gaps tile [0, archive_len).  Empty for every other creator.
    struct Gap { int64_t archive_off, archive_len; int32_t frame, why; };
    std::vector<Gap> gaps;
};

namespace {
jpk_jam_index *jam_index_make(const std::vector<JamFrame> &fr, int64_t in_len, int32_t bad, int32_t kind = JPK_JAM_INDEX_PLAIN)
{
    jpk_jam_index *ix = new (std::nothrow) jpk_jam_index;
    if (!ix) return nullptr;
    try {
        ix->fr = fr;
        ix->raw_off.reserve(fr.size() + 1);
    } catch (const std::bad_alloc &) { delete ix; return nullptr; }
    int64_t raw = 0;
    for (const JamFrame &f : fr) {
        ix->raw_off.push_back(raw);
        raw += f.raw;
    }
    ix->raw_off.push_back(raw);
    ix->archive_len = in_len;
    ix->bad = bad;
    ix->kind = kind;
    return ix;
}

// the last step of every index creator: the index of fr, and the frame it stops in front of
int jam_index_finish(const std::vector<JamFrame> &fr, int64_t in_len, int32_t bad, int32_t kind, jpk_jam_index **index, int32_t *bad_frame)
{
    if (!(*index = jam_index_make(fr, in_len, bad, kind))) return JPK_E_ALLOC;
    if (bad_frame) *bad_frame = bad;
    return JPK_OK;
}
}  // namespace

// ---- whole archives of the stock CLI: every frame through the four pre-stage decoders on the device (prestage_dev.hip) -------------
// Per pass: jpk_dev_blocks_decompress into slot A of every frame, then Lz77 A -> B, Lpx B -> A, Filters A -> B, Lz77 B -> A (the
// order of Jampack::Decomp(), jampack.cpp:51-57), one batched checksum of the A slots against the header crcs, one k_jam_gather
// launch that packs the verified frames back to back into d_out.  A frame's raw size is known only behind its last stage; every stage
// works on the frames in front of the first one that has failed so far, which is where the call stops.  A pass holds at most
// JPK_JAM_PASS_FRAMES frames and JAM_PASS_RAW bytes of BlockSize.
// jam_cli_pass is that stage chain for the frames of one pass; the whole-archive call, the index creation (the same pass without an
// output: the raw sizes are what it is after) and the range reader (a sparse set of frames, the last stage straight into a caller's
// buffer where a range holds the whole frame) run it.
namespace {
// The frames of one pass and where their stages work.  Stage 0 decodes ins[i] into a[i], the stages go A -> B -> A -> B, and the last
// one, the second Lz77::Decompress, writes at most dst_cap[i] bytes to dst[i] (slot A again, or any address of a caller's buffer:
// k_pre_lz77 writes by bytes, k_lzd_copy by bytes at the two ends).  The slots hold caps[i] bytes each.  crc[i] is the header's, d_crc n words of device memory.
//   prefix  every stage runs on the frames in front of the first one that has failed so far (a whole archive stops there); otherwise
//           on all surviving frames, compacted after every stage -- a frame that failed a stage has no lengths for the next one
//   exact   a frame whose raw size is not dst_cap[i] is JPK_E_CORRUPT (the reader: dst_cap is the indexed raw size)
//   staged  staged frames: the list without the first Lz77 and the Lpx stage -- stage 0 into A, Filters A -> B, and
//           Lz77 B -> dst through the deep expander (k_lzd_plan + k_lzd_copy at any address of dst; k_pre_lz77 only for the frames they
//           leave to it: a bad stream, one denser than the dedupe writes, or a byte more than lzx::DEEP_CHASE hops from its literal)
//   sizes   the last stage is k_lz77_sizes: raw[i] is what that Lz77::Decompress would give within dst_cap[i], nothing is expanded and
//           nothing is checked against a crc (dst, crc and d_crc are not looked at) -- the index of staged frames that does not verify
struct CliPass {
    int n;
    const uint8_t *const *ins; const int32_t *lens;
    uint8_t *const *a; uint8_t *const *b; const int32_t *caps;
    uint8_t *const *dst; const int32_t *dst_cap;
    const uint32_t *crc; uint32_t *d_crc;
    bool prefix = false, exact = false, staged = false, sizes = false;
};

// st[i] = JPK_OK and raw[i] = the raw size of a frame that went through every stage and matches its crc -- it is at dst[i] --, else the
// status of the stage it failed (with prefix: also of every frame behind the first failing one, none of which is decoded to the end).
// A stage that runs out of its slot (1.05 x BlockSize + 4096, or dst_cap behind the last stage) met a bad frame: JPK_E_CORRUPT, never
// JPK_E_CAPACITY, which is kept for a caller's out_cap.
int jam_cli_pass(jpk_ctx *ctx, const CliPass &p, int32_t *raw, int32_t *st)
{
    const size_t n = (size_t)p.n;
    std::vector<int> live(n);
    std::vector<const uint8_t *> src(n);
    std::vector<uint8_t *> out(n);
    std::vector<int32_t> len(n), cap(n), got(n), s(n);
    for (size_t i = 0; i < n; i++) { live[i] = (int)i; len[i] = p.lens[i]; st[i] = JPK_OK; raw[i] = 0; }
    // the job arrays of the next stage: the surviving frames, in order
    auto aim = [&](const uint8_t *const *from, uint8_t *const *to, const int32_t *c) {
        for (size_t q = 0; q < live.size(); q++) { src[q] = from[live[q]]; out[q] = to[live[q]]; cap[q] = c[live[q]]; }
        return (int32_t)live.size();
    };
    // behind a stage: s[q] / got[q] of the frames it ran on -> st[], and the survivors with their new lengths
    auto settle = [&]() {
        size_t w = 0;
        for (size_t q = 0; q < live.size(); q++) {
            const int i = live[q];
            if (s[q] != JPK_OK) {
                st[i] = s[q] == JPK_E_CAPACITY ? JPK_E_CORRUPT : s[q];
                if (!p.prefix) continue;
                for (size_t r = q + 1; r < live.size(); r++) st[live[r]] = st[i];
                break;
            }
            live[w] = i; len[w] = got[q]; w++;
        }
        live.resize(w);
    };
    int32_t m = aim(p.ins, p.a, p.caps);
    if (m) {
        JPK_TRY(jpk_dev_blocks_decompress(ctx, m, src.data(), len.data(), out.data(), cap.data(), got.data(), s.data()));           // Ans::Decode + InverseBwt
        settle();
    }
    if (!p.staged && (m = aim(p.a, p.b, p.caps))) {
        JPK_TRY(jpk_dev_blocks_lz77_decompress(ctx, m, src.data(), len.data(), out.data(), cap.data(), got.data(), s.data()));      // Lz->Decompress
        settle();
    }
    if (!p.staged && (m = aim(p.b, p.a, p.caps))) JPK_TRY(jpk_dev_blocks_lpx_decode(ctx, m, src.data(), len.data(), out.data(), s.data()));      // LocalModel->Decode (never fails)
    if ((m = aim(p.a, p.b, p.caps))) {
        JPK_TRY(jpk_dev_blocks_filters_decode(ctx, m, src.data(), len.data(), out.data(), cap.data(), got.data(), s.data()));       // Filter->Decode
        settle();
    }
    if ((m = aim(p.b, p.dst, p.dst_cap))) {
        // Lz->Decompress; a frame that decodes to more than dst_cap (its BlockSize, or its indexed raw size) is a bad frame
        if (p.sizes) JPK_TRY(jpk_dev_blocks_lz77_sizes(ctx, m, src.data(), len.data(), cap.data(), got.data(), s.data()));
        else if (p.staged) JPK_TRY(jpk_lz77_expand_deep_device(ctx, m, src.data(), len.data(), out.data(), cap.data(), got.data(), s.data()));
        else JPK_TRY(jpk_dev_blocks_lz77_decompress(ctx, m, src.data(), len.data(), out.data(), cap.data(), got.data(), s.data()));
        if (p.exact) for (int32_t q = 0; q < m; q++) if (s[(size_t)q] == JPK_OK && got[(size_t)q] != cap[(size_t)q]) s[(size_t)q] = JPK_E_CORRUPT;
        settle();
    }
    if (!p.sizes && (m = (int32_t)live.size())) {
        std::vector<uint32_t> crc((size_t)m);
        for (int32_t q = 0; q < m; q++) src[(size_t)q] = p.dst[live[(size_t)q]];
        JPK_TRY(jam_crcs(ctx, m, src.data(), len.data(), p.d_crc, crc.data()));
        for (int32_t q = 0; q < m; q++) {
            s[(size_t)q] = crc[(size_t)q] != p.crc[live[(size_t)q]] ? JPK_E_CORRUPT : JPK_OK;     // "Detected corrupt block!", jampack.cpp:59
            got[(size_t)q] = len[(size_t)q];
        }
        settle();
    }
    for (size_t q = 0; q < live.size(); q++) raw[live[q]] = len[q];
    return JPK_OK;
}

// Where the chained frames of one pass work, in ctx->jam_scratch: the pass's crc words, a gather table of `pieces` entries, slot A and
// slot B of every frame, and `rest` bytes behind them that are the caller's.  A slot holds caps[q] bytes for the stages and is slot[q] long.
struct ChainSlots {
    uint32_t *d_crc = nullptr;
    JamGatherPiece *d_pieces = nullptr;
    uint8_t *rest = nullptr;
    std::vector<uint8_t *> a, b;
    std::vector<int32_t> caps;
    std::vector<size_t> slot;
    explicit ChainSlots(size_t n) : a(n), b(n), caps(n), slot(n) {}
};
int jam_chain_slots(jpk_ctx *ctx, const std::vector<int32_t> &block_size, size_t pieces, size_t rest, ChainSlots *s)
{
    const size_t n = block_size.size(), o_pieces = jpk_align((size_t)JPK_JAM_PASS_FRAMES * 4), o_slots = o_pieces + jpk_align(pieces * sizeof(JamGatherPiece));
    size_t need = o_slots;
    for (size_t q = 0; q < n; q++) {
        s->caps[q] = jam_cli_cap(block_size[q]);
        s->slot[q] = jpk_align((size_t)s->caps[q] + 64);         // (>= 16 bytes behind every frame: k_jam_gather's aligned loads)
        need += 2 * s->slot[q];
    }
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->jam_scratch, &ctx->jam_scratch_cap, need + rest));
    s->d_crc = reinterpret_cast<uint32_t *>(ctx->jam_scratch);
    s->d_pieces = reinterpret_cast<JamGatherPiece *>(ctx->jam_scratch + o_pieces);
    size_t off = o_slots;
    for (size_t q = 0; q < n; q++) { s->a[q] = ctx->jam_scratch + off; s->b[q] = s->a[q] + s->slot[q]; off += 2 * s->slot[q]; }
    s->rest = ctx->jam_scratch + off;
    return JPK_OK;
}

// the CliPass of the frames that work in the slots s, every flag off: a caller sets the ones it means by name
CliPass jam_chain_pass(const ChainSlots &s, const uint8_t *const *ins, const int32_t *lens, uint8_t *const *dst, const int32_t *dst_cap, const uint32_t *crc)
{
    CliPass p{};
    p.n = (int)s.a.size();
    p.ins = ins; p.lens = lens;
    p.a = s.a.data(); p.b = s.b.data(); p.caps = s.caps.data();
    p.dst = dst; p.dst_cap = dst_cap;
    p.crc = crc; p.d_crc = s.d_crc;
    return p;
}

// The plain frames of one pass: the batch decoder, ins[i] into the raws[i] bytes at outs[i] -- a frame that does not decode to exactly
// that is JPK_E_CORRUPT --, then one batched checksum of the frames that decoded against crc[i] (d_crc: n words of device memory).
// st[i] = JPK_OK for a verified frame, else its status.  prefix as in CliPass: only the frames in front of the first one that did not
// decode are checked, and every frame behind the first failing one has its status; otherwise every frame has its own.
int jam_plain_group(jpk_ctx *ctx, int n, const uint8_t *const *ins, const int32_t *lens, uint8_t *const *outs, const int32_t *raws, const uint32_t *crc,
                    uint32_t *d_crc, bool prefix, int32_t *st)
{
    std::vector<int32_t> outl((size_t)n), clen;
    std::vector<int> dec;
    std::vector<const uint8_t *> cin;
    JPK_TRY(jpk_dev_blocks_decompress(ctx, n, ins, lens, outs, raws, outl.data(), st));
    for (int i = 0; i < n; i++) {
        if (st[i] == JPK_OK && outl[i] != raws[i]) st[i] = JPK_E_CORRUPT;
        if (st[i] != JPK_OK) {
            if (prefix) break;
            continue;
        }
        dec.push_back(i); cin.push_back(outs[i]); clen.push_back(raws[i]);
    }
    if (!dec.empty()) {
        std::vector<uint32_t> got(dec.size());
        JPK_TRY(jam_crcs(ctx, (int)dec.size(), cin.data(), clen.data(), d_crc, got.data()));
        for (size_t q = 0; q < dec.size(); q++)
            if (got[q] != crc[dec[q]]) st[dec[q]] = JPK_E_CORRUPT;       // "Detected corrupt block!", jampack.cpp:59
    }
    if (prefix) {
        int fail = 0;
        while (fail < n && st[fail] == JPK_OK) fail++;
        for (int i = fail + 1; i < n; i++) st[i] = st[fail];
    }
    return JPK_OK;
}
}  // namespace

// ---- whole archives on the device: one pass loop for plain, stock-CLI and staged archives ("Staged frames") ------------------
// Per pass: the chained frames first -- every frame of a stock-CLI archive with the full stage list, the staged frames of a JAM_STAGED
// archive with the staged one, none of a plain archive -- through jam_cli_pass: every one ends verified in its slot A, and its raw size
// is known; then the capacity answer for the pass; then the plain frames in front of the first bad chained one decode in their places
// in d_out, which are known now, and meet their crcs; then one gather launch moves the chained frames to theirs.
namespace {
// jpk_dev_jam_decompress, jpk_dev_jam_cli_decompress(_ix), jpk_dev_jam_staged_decompress(_ix) and, with deliver == false,
// jpk_dev_jam_cli_index_create: the same passes without an output buffer, a capacity answer or a gather.  done (nullable) receives the
// frames that were verified, f.raw = their raw size, and *done_bad (nullable) the first bad frame (-1: none) -- what an index of the
// archive holds.
int jam_decode(jpk_ctx *ctx, int kind, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, const JamResult &res, bool deliver,
               std::vector<JamFrame> *done, int32_t *done_bad)
{
    const bool cli = kind == JAM_CLI;
    jam_result_zero(res);
    if (done_bad) *done_bad = -1;
    if (kind != JAM_PLAIN && in_len == 0) return JPK_OK;        // an empty archive: no frame, no device call
    std::vector<JamFrame> fr;
    int32_t bad = -1;
    JPK_TRY(jam_walk_dev(ctx, d_in, in_len, fr, &bad, kind));
    // plain: the raw bytes, known from the walk -- the capacity answer is exact, comes first and nothing is touched; otherwise the raw
    // bound (a chained frame at its BlockSize), and the answer comes per pass, behind the pass's chain
    const int64_t raw_bound = jam_sum(fr, 0, fr.size(), cli);
    if (kind == JAM_PLAIN && raw_bound > out_cap) { *res.out_len = raw_bound; return JPK_E_CAPACITY; }      // the size query (out_cap = 0) ends here
    auto chained = [cli](const JamFrame &f) { return cli || f.staged; };
    int64_t pos = 0;
    for (size_t k = 0; k < fr.size();) {
        const size_t e = jam_pass_end(fr, k, cli);
        const int n = (int)(e - k);
        // the chained frames of the pass: at[q] = its place in the pass
        std::vector<int> at;
        std::vector<const uint8_t *> cin;
        std::vector<int32_t> clens, bsz;
        std::vector<uint32_t> ccrc;
        for (int i = 0; i < n; i++) {
            const JamFrame &f = fr[k + i];
            if (!chained(f)) continue;
            at.push_back(i);
            cin.push_back(d_in + f.payload_off); clens.push_back(f.psize); bsz.push_back(f.block_size); ccrc.push_back(f.crc);
        }
        const int nc = (int)at.size();
        ChainSlots s(bsz.size());
        JPK_TRY(jam_chain_slots(ctx, bsz, (size_t)JPK_JAM_PASS_FRAMES, 0, &s));
        std::vector<int32_t> craw((size_t)nc), cst((size_t)nc);
        if (nc) {
            // every frame ends in its slot A; a frame that decodes to more than its BlockSize is a bad frame
            CliPass p = jam_chain_pass(s, cin.data(), clens.data(), s.a.data(), bsz.data(), ccrc.data());
            p.prefix = true;
            p.staged = !cli;
            JPK_TRY(jam_cli_pass(ctx, p, craw.data(), cst.data()));
        }
        // m = the frames in front of the first one that has failed so far, rc = its status; raw[i] of the frames in front of it
        std::vector<int64_t> raw((size_t)n);
        int m = n, rc = JPK_OK;
        for (int i = 0; i < n; i++) raw[i] = fr[k + i].raw;
        for (int q = 0; q < nc; q++) {
            if (cst[q] != JPK_OK) { m = at[q]; rc = cst[q]; break; }
            raw[at[q]] = craw[q];
        }
        int64_t sum = 0;
        for (int i = 0; i < m; i++) sum += raw[i];
        if (deliver && sum > out_cap - pos) {
            *res.out_len = raw_bound;
            if (res.frames) *res.frames = (int32_t)k;
            return JPK_E_CAPACITY;
        }
        // the plain frames in front of frame m, in place
        std::vector<int> pat;
        std::vector<const uint8_t *> pin;
        std::vector<uint8_t *> pout;
        std::vector<int32_t> plens, praw;
        std::vector<uint32_t> pcrc;
        {
            int64_t o = pos;
            for (int i = 0; i < m; i++) {
                const JamFrame &f = fr[k + i];
                if (!chained(f)) {
                    pat.push_back(i);
                    pin.push_back(d_in + f.payload_off); plens.push_back(f.psize); pout.push_back(d_out + o); praw.push_back((int32_t)f.raw); pcrc.push_back(f.crc);
                }
                o += raw[i];
            }
        }
        if (!pat.empty()) {
            const int np = (int)pat.size();
            std::vector<int32_t> pst((size_t)np);
            JPK_TRY(jam_plain_group(ctx, np, pin.data(), plens.data(), pout.data(), praw.data(), pcrc.data(), s.d_crc, true, pst.data()));
            for (int q = 0; q < np; q++)
                if (pst[q] != JPK_OK) { m = pat[q]; rc = pst[q]; break; }
        }
        // the chained frames in front of frame m, from their slots to their places
        std::vector<JamGatherPiece> pieces;
        uint64_t words = 0, gbytes = 0;
        sum = 0;
        for (int i = 0, q = 0; i < m; i++) {
            if (chained(fr[k + i])) {
                if (deliver && raw[i]) {
                    jam_piece_add(pieces, &words, s.a[q], d_out + pos + sum, (uint64_t)raw[i], s.a[q], s.a[q] + s.slot[q]);
                    gbytes += (uint64_t)raw[i];
                }
                q++;
            }
            sum += raw[i];
        }
        JPK_TRY(jam_gather(ctx, s.d_pieces, pieces, words, gbytes));
        if (!pieces.empty() && ctx->prof_on) jpk_prof_resolve(ctx);
        if (done)
            for (int i = 0; i < m; i++) {
                done->push_back(fr[k + i]);
                done->back().raw = raw[i];
            }
        pos += sum;
        if (m < n) {
            if (done_bad) *done_bad = (int32_t)k + m;
            return jam_result_stop(res, pos, (int32_t)k + m, rc);
        }
        k = e;
    }
    if (done_bad) *done_bad = bad;
    return jam_result_done(res, pos, fr.size(), bad);
}

// the _ix entries: the decode, and the index of what was delivered -- the whole archive, or the frames in front of the bad one
int jam_decode_ix(jpk_ctx *ctx, int kind, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, const JamResult &res, jpk_jam_index **index)
{
    // (JPK_ENTER taken apart: the argument checks come before the first device call)
    if (!ctx || !res.out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !d_in) || (out_cap > 0 && !d_out)) return JPK_E_ARG;
    if (index) *index = nullptr;
    JPK_HIP(hipSetDevice(ctx->device));
    std::vector<JamFrame> done;
    int32_t done_bad = -1;
    const int rc = jam_decode(ctx, kind, d_in, in_len, d_out, out_cap, res, true, index ? &done : nullptr, &done_bad);
    const int32_t ix_kind = kind == JAM_CLI ? JPK_JAM_INDEX_CLI : JPK_JAM_INDEX_STAGED;
    if (index && (rc == JPK_OK || rc == JPK_E_CORRUPT) && !(*index = jam_index_make(done, in_len, done_bad, ix_kind))) return JPK_E_ALLOC;
    return rc;
}
}  // namespace

extern "C" int jpk_dev_jam_decompress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len, int32_t *frames,
                                      int32_t *bad_frame)
{
    JPK_ENTER(ctx);
    if (!out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !d_in) || (out_cap > 0 && !d_out)) return JPK_E_ARG;
    return jam_decode(ctx, JAM_PLAIN, d_in, in_len, d_out, out_cap, JamResult{out_len, frames, bad_frame}, true, nullptr, nullptr);
}

extern "C" int jpk_dev_jam_cli_decompress_ix(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                             int32_t *frames, int32_t *bad_frame, jpk_jam_index **index)
{
    return jam_decode_ix(ctx, JAM_CLI, d_in, in_len, d_out, out_cap, JamResult{out_len, frames, bad_frame}, index);
}

extern "C" int jpk_dev_jam_cli_decompress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                          int32_t *frames, int32_t *bad_frame)
{
    return jam_decode_ix(ctx, JAM_CLI, d_in, in_len, d_out, out_cap, JamResult{out_len, frames, bad_frame}, nullptr);
}

extern "C" int jpk_dev_jam_staged_decompress_ix(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                                int32_t *frames, int32_t *bad_frame, jpk_jam_index **index)
{
    return jam_decode_ix(ctx, JAM_STAGED, d_in, in_len, d_out, out_cap, JamResult{out_len, frames, bad_frame}, index);
}

extern "C" int jpk_dev_jam_staged_decompress(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                             int32_t *frames, int32_t *bad_frame)
{
    return jam_decode_ix(ctx, JAM_STAGED, d_in, in_len, d_out, out_cap, JamResult{out_len, frames, bad_frame}, nullptr);
}

namespace {
// frames [k, e) of an archive in host memory as a device archive of their own: copied to ctx->stage_in in stream order, *len bytes long,
// and *a0 = the archive offset of its first byte, which a payload_off found in it lacks
int jam_stage_frames(jpk_ctx *ctx, const uint8_t *in, const std::vector<JamFrame> &fr, size_t k, size_t e, int64_t *len, int64_t *a0)
{
    *a0 = fr[k].payload_off - JPK_JAM_HEADER_BYTES;
    *len = fr[e - 1].payload_off + fr[e - 1].psize - *a0;
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_in, &ctx->stage_in_cap, (size_t)*len + 64));
    JPK_HIP(hipMemcpyAsync(ctx->stage_in, in + *a0, (size_t)*len, hipMemcpyHostToDevice, ctx->stream));
    return JPK_OK;
}

// jpk_jam_decompress / jpk_jam_cli_decompress / jpk_jam_staged_decompress: the archive staged one pass at a time -- the pass's frames are an archive of their own
// for the device call
int jam_decompress_host(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frames, int32_t *bad_frame, int kind)
{
    // (an archive that may hold staged frames is sized and reported like one of the stock CLI: a frame's raw size is known behind its last stage)
    const bool cli = kind != JAM_PLAIN;
    if (!out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !in) || (out_cap > 0 && !out)) return JPK_E_ARG;
    const JamResult res{out_len, frames, bad_frame};
    jam_result_zero(res);
    jpk_ctx *ctx;
    JPK_TRY(jpk_host_enter(&ctx, 0));
    std::vector<JamFrame> fr;
    int32_t bad = -1;
    jam_walk_host(in, in_len, fr, &bad, kind);
    // plain: the raw bytes, known from the walk -- the capacity answer comes first and nothing is touched; cli: the raw bound
    const int64_t total = jam_sum(fr, 0, fr.size(), kind == JAM_CLI);
    if (!cli && total > out_cap) { *out_len = total; return JPK_E_CAPACITY; }
    int64_t pos = 0;
    for (size_t k = 0; k < fr.size();) {
        const size_t e = jam_pass_end(fr, k, kind == JAM_CLI);
        // the pass decodes into its raw bytes; cli: into what is left of out_cap, at most the pass's BlockSize bytes
        int64_t room = jam_sum(fr, k, e, kind == JAM_CLI);
        if (cli) room = std::min(room, out_cap - pos);
        JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_res, &ctx->stage_res_cap, (size_t)room + 64));
        int64_t len = 0, a0 = 0, n = 0;
        JPK_TRY(jam_stage_frames(ctx, in, fr, k, e, &len, &a0));
        int32_t nf = 0, bf = -1;
        const int rc = jam_decode(ctx, kind, ctx->stage_in, len, ctx->stage_res, room, JamResult{&n, &nf, &bf}, true, nullptr, nullptr);
        if (cli && rc == JPK_E_CAPACITY) {
            JPK_HIP(hipStreamSynchronize(ctx->stream));
            *out_len = total;
            if (frames) *frames = (int32_t)k;
            return rc;
        }
        if (n > 0 && (rc == JPK_OK || rc == JPK_E_CORRUPT)) JPK_HIP(hipMemcpyAsync(out + pos, ctx->stage_res, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        JPK_HIP(hipStreamSynchronize(ctx->stream));
        if (rc != JPK_OK) {
            // the pass's own report, its frame numbers counted from the archive's start
            if (rc == JPK_E_CORRUPT) *out_len = pos + n;
            if (frames) *frames = (int32_t)k + nf;
            if (bad_frame && bf >= 0) *bad_frame = (int32_t)k + bf;
            return rc;
        }
        pos += n;
        k = e;
    }
    return jam_result_done(res, pos, fr.size(), bad);
}
}  // namespace

extern "C" int jpk_jam_decompress(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frames, int32_t *bad_frame)
{
    return jam_decompress_host(in, in_len, out, out_cap, out_len, frames, bad_frame, JAM_PLAIN);
}

extern "C" int jpk_jam_cli_decompress(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frames, int32_t *bad_frame)
{
    return jam_decompress_host(in, in_len, out, out_cap, out_len, frames, bad_frame, JAM_CLI);
}

extern "C" int jpk_jam_staged_decompress(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frames, int32_t *bad_frame)
{
    return jam_decompress_host(in, in_len, out, out_cap, out_len, frames, bad_frame, JAM_STAGED);
}

// ---- range reads of a .jam archive: jpk_jam_index + jpk_dev_jam_read / jpk_jam_read -----------------------------------------------
// The index is the frame table of the walks with the 64-bit prefix sum of the raw sizes.  A read maps every range to the frames it
// touches, decodes each touched frame ONCE -- in place in the first range that contains it whole, otherwise into a padded slot of
// ctx->jam_scratch -- in passes with the limits of the archive calls, checks every decoded frame against its header crc, and delivers
// the pieces of the verified frames with one k_jam_gather launch per pass.  A frame no range touches is neither decoded nor checked.
// An index of a stock-CLI archive (kind JPK_JAM_INDEX_CLI) can only come from a decode -- a frame's raw size is in no header -- and a
// read through it is the same plan with jam_cli_pass as the decoder: two slots of 1.05 x BlockSize + 4096 per touched frame, passes
// bounded by BlockSize, and the last stage writes a frame that a range holds whole straight into that range at exactly its indexed size.
// An index of plain and staged frames (kind JPK_JAM_INDEX_STAGED) takes a staged frame's raw size from the token walk of its S1
// (k_lz77_sizes: no expansion, no checksum) or from a decode; a pass of a read through it holds two groups behind the one plan, the
// plain frames for the batch decoder and the staged ones for jam_cli_pass with the staged stage list, and one gather for both.
namespace {
// the argument checks of both read entries: nothing is touched before they pass
int jam_read_check(const jpk_jam_index *ix, const void *in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len, uint8_t *const *out)
{
    if (!ix || n < 0 || in_len != ix->archive_len || (n > 0 && (!off || !len || !out))) return JPK_E_ARG;
    const int64_t raw_len = ix->raw_off.back();
    for (int32_t r = 0; r < n; r++) {
        if (off[r] < 0 || len[r] < 0 || off[r] > raw_len || len[r] > raw_len - off[r]) return JPK_E_ARG;
        if (len[r] > 0 && (!out[r] || !in)) return JPK_E_ARG;
    }
    return JPK_OK;
}

// The read itself.  The archive is d_in (HBM) or, when d_in is NULL, h_in (host memory: the payloads of a pass's frames are staged
// through ctx->stage_in); d_out[] are device buffers in both cases.  status has n entries.
int jam_read_pieces(jpk_ctx *ctx, const jpk_jam_index *ix, const uint8_t *d_in, const uint8_t *h_in, int32_t n, const int64_t *off, const int64_t *len,
                    uint8_t *const *d_out, int32_t *status, int32_t *bad_frame)
{
    const size_t F = ix->fr.size();
    const std::vector<int64_t> &ro = ix->raw_off;
    // frames [first[r], last[r]] of range r; pieces per frame (a piece = the part of one frame one range wants); the in-place home of
    // a frame: inside the first range that contains it whole
    std::vector<int32_t> first((size_t)n, -1), last((size_t)n, -1);
    std::vector<size_t> start(F + 1, 0);
    std::vector<uint8_t *> home(F, nullptr);
    for (int32_t r = 0; r < n; r++) {
        status[r] = JPK_OK;
        if (len[r] == 0) continue;
        const int64_t a = off[r], b = a + len[r];
        first[r] = (int32_t)(std::upper_bound(ro.begin(), ro.end(), a) - ro.begin()) - 1;
        last[r] = (int32_t)(std::lower_bound(ro.begin(), ro.end(), b) - ro.begin()) - 1;
        for (int32_t f = first[r]; f <= last[r]; f++) {
            if (ix->fr[(size_t)f].raw == 0) continue;
            start[(size_t)f + 1]++;
            if (!home[(size_t)f] && ro[(size_t)f] >= a && ro[(size_t)f + 1] <= b) home[(size_t)f] = d_out[r] + (ro[(size_t)f] - a);
        }
    }
    std::vector<size_t> touched;
    for (size_t f = 0; f < F; f++) {
        if (start[f + 1]) touched.push_back(f);
        start[f + 1] += start[f];
    }
    std::vector<int32_t> piece_range(start[F]);
    {
        std::vector<size_t> fill(start.begin(), start.end() - 1);
        for (int32_t r = 0; r < n; r++)
            for (int32_t f = first[r]; f >= 0 && f <= last[r]; f++)
                if (ix->fr[(size_t)f].raw) piece_range[fill[(size_t)f]++] = r;
    }
    std::vector<int32_t> fstat(F, JPK_OK);
    const bool cli = ix->kind == JPK_JAM_INDEX_CLI;
    // the frames that go through the stage chain (jam_cli_pass): all of a stock-CLI index, the staged ones of a JPK_JAM_INDEX_STAGED index
    // (no other index holds one); the other frames are plain ones for the batch decoder alone
    auto chained = [&](size_t f) { return cli || ix->fr[f].staged; };
    // the jobs of one decoder in a pass: at[q] = the frame's place in the pass, crcs[q] the crc to meet
    struct Group {
        std::vector<int> at;
        std::vector<const uint8_t *> ins;
        std::vector<uint8_t *> outs;
        std::vector<int32_t> lens, caps;
        std::vector<uint32_t> crcs;
    };
    for (size_t k = 0; k < touched.size();) {
        const size_t e = jam_pass_end(touched.size(), k, [&](size_t i) { return jam_weight(ix->fr[touched[i]], cli); });
        const int m = (int)(e - k);
        size_t npieces = 0, plain_bytes = 0, stage_bytes = 0;
        std::vector<int32_t> bsz;                                             // of the chain's frames: two slots each, whatever the frame's raw size
        for (int i = 0; i < m; i++) {
            const size_t f = touched[k + i];
            npieces += start[f + 1] - start[f];
            if (chained(f)) bsz.push_back(ix->fr[f].block_size);
            else if (!home[f]) plain_bytes += jpk_align((size_t)ix->fr[f].raw + 64);
            stage_bytes += jpk_align((size_t)ix->fr[f].psize + 64);
        }
        ChainSlots s(bsz.size());
        JPK_TRY(jam_chain_slots(ctx, bsz, npieces, plain_bytes, &s));
        if (!d_in) JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_in, &ctx->stage_in_cap, stage_bytes));
        std::vector<const uint8_t *> hi((size_t)m);                           // hi[i]: the end of what is readable around the decoded frame
        std::vector<uint8_t *> outs((size_t)m);
        Group chain, plain;
        chain.crcs.resize(bsz.size());                                        // (filled by copies in stream order: the words must stay where they are)
        uint8_t *slot = s.rest;
        size_t stage = 0;
        for (int i = 0; i < m; i++) {
            const size_t f = touched[k + i];
            const JamFrame &fr = ix->fr[f];
            Group &g = chained(f) ? chain : plain;
            if (d_in) g.ins.push_back(d_in + fr.payload_off);
            else {
                JPK_HIP(hipMemcpyAsync(ctx->stage_in + stage, h_in + fr.payload_off, (size_t)fr.psize, hipMemcpyHostToDevice, ctx->stream));
                g.ins.push_back(ctx->stage_in + stage);
                stage += jpk_align((size_t)fr.psize + 64);
            }
            g.at.push_back(i); g.lens.push_back(fr.psize); g.caps.push_back((int32_t)fr.raw);
            if (chained(f)) {
                const size_t q = g.at.size() - 1;
                // the crc to meet is the one in the header of the archive being read, which need not be the indexed one any more
                if (d_in) JPK_HIP(hipMemcpyAsync(&g.crcs[q], d_in + fr.payload_off - JPK_JAM_HEADER_BYTES + 3, 4, hipMemcpyDeviceToHost, ctx->stream));
                else memcpy(&g.crcs[q], h_in + fr.payload_off - JPK_JAM_HEADER_BYTES + 3, 4);
                outs[i] = home[f] ? home[f] : s.a[q];
                hi[i] = home[f] ? outs[i] + fr.raw : s.a[q] + s.slot[q];
            } else {
                g.crcs.push_back(fr.crc);
                if (home[f]) outs[i] = home[f];
                else { outs[i] = slot; slot += jpk_align((size_t)fr.raw + 64); }
                hi[i] = home[f] ? outs[i] + fr.raw : outs[i] + ((fr.raw + 15) & ~(int64_t)15) + 16;
            }
            g.outs.push_back(outs[i]);
        }
        if (!chain.at.empty()) {
            // the stage chain on the touched frames alone, the last stage at the indexed raw size; the checksum is the pass's
            const int nc = (int)chain.at.size();
            std::vector<int32_t> outl((size_t)nc), st((size_t)nc);
            CliPass p = jam_chain_pass(s, chain.ins.data(), chain.lens.data(), chain.outs.data(), chain.caps.data(), chain.crcs.data());
            p.exact = true;
            p.staged = !cli;
            JPK_TRY(jam_cli_pass(ctx, p, outl.data(), st.data()));
            for (int q = 0; q < nc; q++) fstat[touched[k + (size_t)chain.at[q]]] = st[q];
        }
        if (!plain.at.empty()) {
            // the batch decoder, then one batched checksum of the frames that decoded, against their indexed crcs
            const int np = (int)plain.at.size();
            std::vector<int32_t> st((size_t)np);
            JPK_TRY(jam_plain_group(ctx, np, plain.ins.data(), plain.lens.data(), plain.outs.data(), plain.caps.data(), plain.crcs.data(), s.d_crc, false, st.data()));
            for (int q = 0; q < np; q++) fstat[touched[k + (size_t)plain.at[q]]] = st[q];
        }
        // the pieces of the verified frames (the one a frame was decoded into in place is already where it belongs)
        std::vector<JamGatherPiece> tab;
        tab.reserve(npieces);
        uint64_t words = 0, bytes = 0;
        for (int i = 0; i < m; i++) {
            const size_t f = touched[k + i];
            if (fstat[f] != JPK_OK) continue;
            for (size_t q = start[f]; q < start[f + 1]; q++) {
                const int32_t r = piece_range[q];
                const int64_t a = std::max(ro[f], off[r]), b = std::min(ro[f + 1], off[r] + len[r]);
                const uint8_t *src = outs[i] + (a - ro[f]);
                uint8_t *dst = d_out[r] + (a - off[r]);
                if (src == dst) continue;
                jam_piece_add(tab, &words, src, dst, (uint64_t)(b - a), outs[i], hi[i]);
                bytes += (uint64_t)(b - a);
            }
        }
        JPK_TRY(jam_gather(ctx, s.d_pieces, tab, words, bytes));
        k = e;
    }
    int32_t bad = -1;
    for (size_t f : touched) if (fstat[f] != JPK_OK) { bad = (int32_t)f; break; }
    if (bad >= 0)
        for (int32_t r = 0; r < n; r++)
            for (int32_t f = first[r]; f >= 0 && f <= last[r]; f++)
                if (ix->fr[(size_t)f].raw && fstat[(size_t)f] != JPK_OK) { status[r] = fstat[(size_t)f]; break; }
    if (bad_frame) *bad_frame = bad;
    return JPK_OK;
}

// n and the number of pieces are the caller's: the host tables of a read that does not fit in memory end in JPK_E_ALLOC, not in an
// exception that leaves through the C ABI
int jam_read_run(jpk_ctx *ctx, const jpk_jam_index *ix, const uint8_t *d_in, const uint8_t *h_in, int32_t n, const int64_t *off, const int64_t *len,
                 uint8_t *const *d_out, int32_t *status, int32_t *bad_frame)
{
    try {
        return jam_read_pieces(ctx, ix, d_in, h_in, n, off, len, d_out, status, bad_frame);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(ctx->stream);             // nothing queued may outlive the tables it reads
        return JPK_E_ALLOC;
    }
}

// no range wants a byte: nothing to decode, every status JPK_OK
bool jam_read_empty(int32_t n, const int64_t *len, int32_t *status)
{
    for (int32_t r = 0; r < n; r++) if (len[r] > 0) return false;
    if (status) for (int32_t r = 0; r < n; r++) status[r] = JPK_OK;
    return true;
}

int jam_read_result(int32_t n, const int32_t *st, int32_t *status)
{
    if (status) { for (int32_t r = 0; r < n; r++) status[r] = st[r]; return JPK_OK; }
    for (int32_t r = 0; r < n; r++) if (st[r] != JPK_OK) return st[r];
    return JPK_OK;
}
}  // namespace

extern "C" int jpk_dev_jam_index_create(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame)
{
    JPK_ENTER(ctx);
    if (!index || in_len < 0 || (in_len > 0 && !d_in)) return JPK_E_ARG;
    *index = nullptr;
    std::vector<JamFrame> fr;
    int32_t bad = -1;
    JPK_TRY(jam_walk_dev(ctx, d_in, in_len, fr, &bad));
    return jam_index_finish(fr, in_len, bad, JPK_JAM_INDEX_PLAIN, index, bad_frame);
}

extern "C" int jpk_jam_index_create(const uint8_t *in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame)
{
    if (!index || in_len < 0 || (in_len > 0 && !in)) return JPK_E_ARG;
    *index = nullptr;
    std::vector<JamFrame> fr;
    int32_t bad = -1;
    jam_walk_host(in, in_len, fr, &bad);
    return jam_index_finish(fr, in_len, bad, JPK_JAM_INDEX_PLAIN, index, bad_frame);
}

extern "C" int jpk_dev_jam_cli_index_create(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame)
{
    // (JPK_ENTER taken apart: the argument checks come before the first device call, and an empty archive makes none)
    if (!ctx || !index || in_len < 0 || (in_len > 0 && !d_in)) return JPK_E_ARG;
    *index = nullptr;
    if (in_len > 0) JPK_HIP(hipSetDevice(ctx->device));
    std::vector<JamFrame> done;
    int64_t raw_len = 0;
    int32_t bad = -1;
    const int rc = jam_decode(ctx, JAM_CLI, d_in, in_len, nullptr, 0, JamResult{&raw_len, nullptr, nullptr}, false, &done, &bad);
    if (rc != JPK_OK && rc != JPK_E_CORRUPT) return rc;      // a bad frame ends the index, not the call
    return jam_index_finish(done, in_len, bad, JPK_JAM_INDEX_CLI, index, bad_frame);
}

extern "C" int jpk_jam_cli_index_create(const uint8_t *in, int64_t in_len, jpk_jam_index **index, int32_t *bad_frame)
{
    if (!index || in_len < 0 || (in_len > 0 && !in)) return JPK_E_ARG;
    *index = nullptr;
    std::vector<JamFrame> fr, done;
    int32_t bad = -1;
    if (in_len > 0) {
        jpk_ctx *ctx;
        JPK_TRY(jpk_host_enter(&ctx, 0));
        jam_walk_host(in, in_len, fr, &bad, JAM_CLI);
        // staged one pass at a time, jam_stage_frames: the pass is an archive of its own for the device decode
        for (size_t k = 0; k < fr.size();) {
            const size_t e = jam_pass_end(fr, k, true);
            int64_t len = 0, a0 = 0, raw_len = 0;
            JPK_TRY(jam_stage_frames(ctx, in, fr, k, e, &len, &a0));
            std::vector<JamFrame> got;
            int32_t pass_bad = -1;
            const int rc = jam_decode(ctx, JAM_CLI, ctx->stage_in, len, nullptr, 0, JamResult{&raw_len, nullptr, nullptr}, false, &got, &pass_bad);
            JPK_HIP(hipStreamSynchronize(ctx->stream));
            if (rc != JPK_OK && rc != JPK_E_CORRUPT) return rc;
            for (JamFrame &f : got) { f.payload_off += a0; done.push_back(f); }
            if (pass_bad >= 0) { bad = (int32_t)k + pass_bad; break; }
            k = e;
        }
    }
    return jam_index_finish(done, in_len, bad, JPK_JAM_INDEX_CLI, index, bad_frame);
}

namespace {
// The chained frames among fr[k, e) (one pass: the limits of the whole-archive decode of their kind) through jam_cli_pass without an output
// -- cli: every frame, with the stock-CLI stage list; otherwise the staged ones, with the staged list.  verify: the whole stage list and the
// header crcs; otherwise (staged frames only) its sizes form, which stops in front of the expansion.  The payload of a frame is at d_in +
// (payload_off - a0).  st[i - k] = JPK_OK and fr[i].raw = its raw size, or the status of the stage it failed (prefix: also of every chained
// frame behind the first failing one); a plain frame keeps the raw size of the walk, is not decoded and is JPK_OK.
int jam_chain_size_pass(jpk_ctx *ctx, const uint8_t *d_in, int64_t a0, std::vector<JamFrame> &fr, size_t k, size_t e, bool cli, bool verify, bool prefix, int32_t *st)
{
    std::vector<size_t> sidx;
    std::vector<const uint8_t *> sin;
    std::vector<int32_t> slens, bsz;
    std::vector<uint32_t> scrc;
    for (size_t i = k; i < e; i++) {
        const JamFrame &f = fr[i];
        st[i - k] = JPK_OK;
        if (!cli && !f.staged) continue;
        sidx.push_back(i);
        sin.push_back(d_in + (f.payload_off - a0)); slens.push_back(f.psize); bsz.push_back(f.block_size); scrc.push_back(f.crc);
    }
    const size_t ns = sidx.size();
    if (!ns) return JPK_OK;
    ChainSlots s(bsz.size());
    JPK_TRY(jam_chain_slots(ctx, bsz, 0, 0, &s));
    std::vector<int32_t> sraw(ns), sst(ns);
    // a frame that declares more than its BlockSize is a bad frame, expanded or not
    CliPass p = jam_chain_pass(s, sin.data(), slens.data(), s.a.data(), bsz.data(), scrc.data());
    p.prefix = prefix;
    p.staged = !cli;
    p.sizes = !verify;
    JPK_TRY(jam_cli_pass(ctx, p, sraw.data(), sst.data()));
    for (size_t q = 0; q < ns; q++) {
        st[sidx[q] - k] = sst[q];
        if (sst[q] == JPK_OK) fr[sidx[q]].raw = sraw[q];
    }
    return JPK_OK;
}
int jam_staged_size_pass(jpk_ctx *ctx, const uint8_t *d_in, int64_t a0, std::vector<JamFrame> &fr, size_t k, size_t e, bool verify, bool prefix, int32_t *st)
{
    return jam_chain_size_pass(ctx, d_in, a0, fr, k, e, false, verify, prefix, st);
}
// every frame of a stock-CLI pass decoded into its slot A and checked against its crc (the passes of jpk_dev_jam_cli_index_create)
int jam_cli_size_pass(jpk_ctx *ctx, const uint8_t *d_in, int64_t a0, std::vector<JamFrame> &fr, size_t k, size_t e, bool prefix, int32_t *st)
{
    return jam_chain_size_pass(ctx, d_in, a0, fr, k, e, true, true, prefix, st);
}

// The frames of an index of kind JPK_JAM_INDEX_STAGED for an archive in HBM: the walk, then jam_staged_size_pass per pass.
// done = the frames in front of the first bad one, *bad = its position (-1: none).
int jam_staged_sizes(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, bool verify, std::vector<JamFrame> &done, int32_t *bad)
{
    std::vector<JamFrame> fr;
    JPK_TRY(jam_walk_dev(ctx, d_in, in_len, fr, bad, JAM_STAGED));
    std::vector<int32_t> st;
    for (size_t k = 0; k < fr.size();) {
        const size_t e = jam_pass_end(fr, k, false);
        st.resize(e - k);
        JPK_TRY(jam_staged_size_pass(ctx, d_in, 0, fr, k, e, verify, true, st.data()));
        size_t stop = k;
        while (stop < e && st[stop - k] == JPK_OK) stop++;
        done.insert(done.end(), fr.begin() + (ptrdiff_t)k, fr.begin() + (ptrdiff_t)stop);
        if (stop < e) { *bad = (int32_t)stop; return JPK_OK; }
        k = e;
    }
    return JPK_OK;
}

bool jam_verify_ok(int32_t verify) { return verify == 0 || verify == 1; }
}  // namespace

extern "C" int jpk_dev_jam_staged_index_create(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t verify, jpk_jam_index **index, int32_t *bad_frame)
{
    // (the argument checks come before the first device call, and an empty archive makes none)
    if (!ctx || !index || in_len < 0 || (in_len > 0 && !d_in) || !jam_verify_ok(verify)) return JPK_E_ARG;
    *index = nullptr;
    std::vector<JamFrame> done;
    int32_t bad = -1;
    if (in_len > 0) {
        JPK_HIP(hipSetDevice(ctx->device));
        JPK_TRY(jam_staged_sizes(ctx, d_in, in_len, verify != 0, done, &bad));
    }
    return jam_index_finish(done, in_len, bad, JPK_JAM_INDEX_STAGED, index, bad_frame);
}

extern "C" int jpk_jam_staged_index_create(const uint8_t *in, int64_t in_len, int32_t verify, jpk_jam_index **index, int32_t *bad_frame)
{
    if (!index || in_len < 0 || (in_len > 0 && !in) || !jam_verify_ok(verify)) return JPK_E_ARG;
    *index = nullptr;
    std::vector<JamFrame> fr, done;
    int32_t bad = -1;
    jam_walk_host(in, in_len, fr, &bad, JAM_STAGED);
    auto staged_in = [&fr](size_t k, size_t e) { return std::any_of(fr.begin() + (ptrdiff_t)k, fr.begin() + (ptrdiff_t)e, [](const JamFrame &f) { return f.staged; }); };
    // an archive of plain frames is indexed by the walk alone: no device is looked for
    jpk_ctx *ctx = nullptr;
    if (staged_in(0, fr.size())) JPK_TRY(jpk_host_enter(&ctx, 0));
    for (size_t k = 0; k < fr.size();) {
        const size_t e = jam_pass_end(fr, k, false);
        if (!staged_in(k, e)) { done.insert(done.end(), fr.begin() + (ptrdiff_t)k, fr.begin() + (ptrdiff_t)e); k = e; continue; }
        // staged one pass at a time, jam_stage_frames: the pass is an archive of its own for the device
        int64_t len = 0, a0 = 0;
        JPK_TRY(jam_stage_frames(ctx, in, fr, k, e, &len, &a0));
        std::vector<JamFrame> got;
        int32_t pass_bad = -1;
        const int rc = jam_staged_sizes(ctx, ctx->stage_in, len, verify != 0, got, &pass_bad);
        JPK_HIP(hipStreamSynchronize(ctx->stream));
        JPK_TRY(rc);
        for (JamFrame &f : got) { f.payload_off += a0; done.push_back(f); }
        if (pass_bad >= 0) { bad = (int32_t)k + pass_bad; break; }
        k = e;
    }
    return jam_index_finish(done, in_len, bad, JPK_JAM_INDEX_STAGED, index, bad_frame);
}

extern "C" int jpk_jam_index_kind(const jpk_jam_index *index) { return index ? index->kind : JPK_E_ARG; }

extern "C" int jpk_jam_index_frame_kind(const jpk_jam_index *index, int32_t k)
{
    if (!index || k < 0 || (size_t)k >= index->fr.size()) return JPK_E_ARG;
    if (index->kind != JPK_JAM_INDEX_STAGED) return index->kind;
    return index->fr[(size_t)k].staged ? JPK_JAM_INDEX_STAGED : JPK_JAM_INDEX_PLAIN;
}

extern "C" int jpk_jam_index_info(const jpk_jam_index *index, int32_t *frames, int64_t *raw_len, int64_t *archive_len)
{
    if (!index) return JPK_E_ARG;
    if (frames) *frames = (int32_t)index->fr.size();
    if (raw_len) *raw_len = index->raw_off.back();
    if (archive_len) *archive_len = index->archive_len;
    return JPK_OK;
}

extern "C" int jpk_jam_index_frame(const jpk_jam_index *index, int32_t k, int64_t *raw_off, int64_t *raw, int64_t *payload_off, int32_t *psize)
{
    if (!index || k < 0 || (size_t)k >= index->fr.size()) return JPK_E_ARG;
    if (raw_off) *raw_off = index->raw_off[(size_t)k];
    if (raw) *raw = index->fr[(size_t)k].raw;
    if (payload_off) *payload_off = index->fr[(size_t)k].payload_off;
    if (psize) *psize = index->fr[(size_t)k].psize;
    return JPK_OK;
}

extern "C" void jpk_jam_index_destroy(jpk_jam_index *index) { delete index; }

extern "C" int jpk_dev_jam_read(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len,
                                uint8_t *const *d_out, int32_t *status, int32_t *bad_frame)
{
    // (JPK_ENTER taken apart: the argument checks come before the first device call)
    if (!ctx) return JPK_E_ARG;
    JPK_TRY(jam_read_check(index, d_in, in_len, n, off, len, d_out));
    JPK_HIP(hipSetDevice(ctx->device));
    if (bad_frame) *bad_frame = -1;
    if (jam_read_empty(n, len, status)) return JPK_OK;
    std::vector<int32_t> st;
    try { st.resize((size_t)n); } catch (const std::bad_alloc &) { return JPK_E_ALLOC; }
    JPK_TRY(jam_read_run(ctx, index, d_in, nullptr, n, off, len, d_out, st.data(), bad_frame));
    return jam_read_result(n, st.data(), status);
}

extern "C" int jpk_jam_read(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len, uint8_t *const *out,
                            int32_t *status, int32_t *bad_frame)
{
    JPK_TRY(jam_read_check(index, in, in_len, n, off, len, out));
    if (bad_frame) *bad_frame = -1;
    if (jam_read_empty(n, len, status)) return JPK_OK;
    jpk_ctx *ctx;
    JPK_TRY(jpk_host_enter(&ctx, 0));
    // the ranges side by side in ctx->stage_res (a range may start at any address); only they travel back
    std::vector<uint8_t *> d_out;
    std::vector<int32_t> st;
    try { d_out.resize((size_t)n); st.resize((size_t)n); } catch (const std::bad_alloc &) { return JPK_E_ALLOC; }
    int64_t total = 0;
    for (int32_t r = 0; r < n; r++) total += len[r];
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_res, &ctx->stage_res_cap, (size_t)total + 64));
    total = 0;
    for (int32_t r = 0; r < n; r++) { d_out[(size_t)r] = ctx->stage_res + total; total += len[r]; }
    JPK_TRY(jam_read_run(ctx, index, nullptr, in, n, off, len, d_out.data(), st.data(), bad_frame));
    // few ranges: one copy each; many small ones: one copy of all of them and the split on the host
    if (n <= 16 || total > (64ll << 20)) {
        for (int32_t r = 0; r < n; r++)
            if (len[r] > 0 && st[(size_t)r] == JPK_OK) JPK_HIP(hipMemcpyAsync(out[r], d_out[(size_t)r], (size_t)len[r], hipMemcpyDeviceToHost, ctx->stream));
        JPK_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<uint8_t> all;
        try { all.resize((size_t)total); } catch (const std::bad_alloc &) { return JPK_E_ALLOC; }
        JPK_HIP(hipMemcpyAsync(all.data(), ctx->stage_res, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
        JPK_HIP(hipStreamSynchronize(ctx->stream));
        for (int32_t r = 0; r < n; r++)
            if (len[r] > 0 && st[(size_t)r] == JPK_OK) memcpy(out[r], all.data() + (d_out[(size_t)r] - ctx->stage_res), (size_t)len[r]);
    }
    return jam_read_result(n, st.data(), status);
}

// ---- damaged archives: an index past the damage, and everything recoverable ("Damaged archives") ------------------------
// jpk_(dev_)jam_index_recover run the resync walk of jam_resync.hpp -- one loop for both forms, over JamDevSrc or jrs::HostSrc: where
// the frame walk stops, the first structurally valid frame behind it is searched (in HBM: k_jam_scan_* for the plausible headers of a
// window, jpk_ans_decoded_sizes for a batch of them), and what lies between becomes a gap of the index.  An undamaged archive is one run
// of the frame walk and launches no scan.  The frames of a stock-CLI archive (kind 1) then go through their stage chain and meet their
// crcs, pass by pass (jam_cli_size_pass, every frame with a status of its own): that is where their raw sizes come from, and a frame that
// fails is a gap over its own span.  jpk_(dev_)jam_salvage is one range per frame through the reader above; jpk_(dev_)jam_repair copies the
// spans of the kept frames back to back and decodes nothing.
namespace {
std::atomic<int64_t> g_recover_window{jrs::DEFAULT_WINDOW};
std::atomic<int32_t> g_recover_cands{jrs::DEFAULT_CANDS};
constexpr int64_t JAM_SCAN_MAX_WINDOW = 1ll << 30;      // tiles and their prefix sums stay 32-bit
constexpr int32_t JAM_SCAN_MAX_CANDS = 1 << 16;

// the first max_cands plausible headers that start in [start, end) of an archive in HBM, ascending: count, scan, emit, one read-back.
// Scratch: a word per tile and max_cands table entries in ctx->jam_scratch
int jam_scan_dev(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int64_t start, int64_t end, bool staged_ok, int32_t max_cands, std::vector<JamWalkFrame> &out)
{
    out.clear();
    if (start >= end) return JPK_OK;
    const uint32_t ntiles = jpk_jam_scan_tiles(d_in, start, end);
    const size_t o_cands = jpk_align(((size_t)ntiles + 1) * 4);
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->jam_scratch, &ctx->jam_scratch_cap, o_cands + (size_t)max_cands * sizeof(JamWalkFrame)));
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(ctx->jam_scratch);
    JamWalkFrame *d_cands = reinterpret_cast<JamWalkFrame *>(ctx->jam_scratch + o_cands);
    JPK_TRY(jpk_jam_scan_count_enqueue(ctx, d_in, in_len, start, end, staged_ok, d_counts));
    uint32_t total = 0;
    JPK_TRY(jpk_dev_exclusive_scan_u32(ctx, d_counts, (int32_t)ntiles + 1, &total));     // synchronises
    const size_t n = std::min<size_t>(total, (size_t)max_cands);
    if (n) {
        out.resize(n);
        JPK_TRY(jpk_jam_scan_emit_enqueue(ctx, d_in, in_len, start, end, staged_ok, d_counts, d_cands, (uint32_t)max_cands));
        JPK_HIP(hipMemcpyAsync(out.data(), d_cands, n * sizeof(JamWalkFrame), hipMemcpyDeviceToHost, ctx->stream));
        JPK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (ctx->prof_on) jpk_prof_resolve(ctx);
    return JPK_OK;
}

// jrs::walk's source for an archive in HBM
struct JamDevSrc {
    jpk_ctx *ctx;
    const uint8_t *d_in;
    int64_t in_len;
    int kind;                                         // JAM_PLAIN, JAM_CLI or JAM_STAGED
    std::vector<JamWalkFrame> c;                      // the candidates of the last cands()
    template <class OnFrame> int run(int64_t g, OnFrame on_frame, int64_t *stop)
    {
        std::vector<JamFrame> fr;
        int32_t bad = -1;
        JPK_TRY(jam_walk_dev(ctx, d_in, in_len, fr, &bad, kind, g, stop));
        for (const JamFrame &f : fr) on_frame(f);
        return JPK_OK;
    }
    int cands(int64_t from, int64_t to, int32_t K, int32_t *n)
    {
        JPK_TRY(jam_scan_dev(ctx, d_in, in_len, from, to, kind == JAM_STAGED, K, c));
        *n = (int32_t)c.size();
        return JPK_OK;
    }
    int64_t cand(int32_t i) const { return (int64_t)c[(size_t)i].payload_off - JPK_JAM_HEADER_BYTES; }
    int first_valid(int32_t n, int32_t *hit, JamFrame *f)
    {
        std::vector<const uint8_t *> ins((size_t)n);
        std::vector<int32_t> lens((size_t)n), st((size_t)n);
        std::vector<int64_t> dec((size_t)n);
        for (int32_t i = 0; i < n; i++) { ins[(size_t)i] = d_in + c[(size_t)i].payload_off; lens[(size_t)i] = c[(size_t)i].psize; }
        JPK_TRY(jpk_ans_decoded_sizes(ctx, n, ins.data(), lens.data(), dec.data(), st.data()));
        *hit = -1;
        for (int32_t i = 0; i < n && *hit < 0; i++)
            if (jam_frame_of(c[(size_t)i], st[(size_t)i], dec[(size_t)i], kind == JAM_CLI, f)) *hit = i;
        return JPK_OK;
    }
};

using JamGap = jpk_jam_index::Gap;

// the resync walk of either form: the frames it found and the gaps between them (why = JPK_JAM_GAP_NOFRAME)
template <class Src> int jam_recover_walk(Src &src, int64_t in_len, std::vector<JamFrame> &fr, std::vector<JamGap> &gaps)
{
    return jrs::walk(src, in_len, g_recover_window.load(), g_recover_cands.load(), [&](const JamFrame &f) { fr.push_back(f); },
                     [&](int64_t o, int64_t n) { gaps.push_back(JamGap{o, n, (int32_t)fr.size(), JPK_JAM_GAP_NOFRAME}); });
}

// frames [k, e) form the sizing pass that starts at frame k: the limits of jam_pass_end (cli: a frame weighs its BlockSize), and frames
// that lie back to back in the archive -- a pass never spans a gap, so the host form can stage it as one piece
size_t jam_recover_pass_end(const std::vector<JamFrame> &fr, size_t k, bool cli)
{
    const size_t lim = jam_pass_end(fr, k, cli);
    size_t e = k + 1;
    while (e < lim && fr[e].payload_off - JPK_JAM_HEADER_BYTES == fr[e - 1].payload_off + fr[e - 1].psize) e++;
    return e;
}

// what the index holds: frames whose status is JPK_OK, every other one a gap over its own span (why = JPK_JAM_GAP_STAGE) among the
// gaps of the walk, and `frame` of every gap counted in the frames that stay
jpk_jam_index *jam_recover_make(const std::vector<JamFrame> &fr, const std::vector<int32_t> &st, const std::vector<JamGap> &gaps, int64_t in_len, int32_t kind)
{
    std::vector<JamFrame> keep;
    std::vector<JamGap> all;
    size_t gi = 0;
    for (size_t i = 0; i <= fr.size(); i++) {
        for (; gi < gaps.size() && (size_t)gaps[gi].frame == i; gi++) all.push_back(JamGap{gaps[gi].archive_off, gaps[gi].archive_len, (int32_t)keep.size(), gaps[gi].why});
        if (i == fr.size()) break;
        if (st[i] == JPK_OK) keep.push_back(fr[i]);
        else all.push_back(JamGap{fr[i].payload_off - JPK_JAM_HEADER_BYTES, (int64_t)JPK_JAM_HEADER_BYTES + fr[i].psize, (int32_t)keep.size(), JPK_JAM_GAP_STAGE});
    }
    jpk_jam_index *ix = jam_index_make(keep, in_len, -1, kind);
    if (ix) ix->gaps = std::move(all);
    return ix;
}

bool jam_recover_args_ok(const void *in, int64_t in_len, int32_t kind, int32_t verify, jpk_jam_index **index)
{
    // (a plain index verifies nothing; every frame of a stock-CLI index has been decoded: its raw size is known only behind its last stage)
    return index && in_len >= 0 && (in_len == 0 || in) && (kind == JPK_JAM_INDEX_PLAIN || kind == JPK_JAM_INDEX_CLI || kind == JPK_JAM_INDEX_STAGED) &&
           jam_verify_ok(verify) && !(kind == JPK_JAM_INDEX_PLAIN && verify) && !(kind == JPK_JAM_INDEX_CLI && !verify);
}

// what the walks call the archive of an index kind
int jam_recover_walk_kind(int32_t kind) { return kind == JPK_JAM_INDEX_STAGED ? JAM_STAGED : kind == JPK_JAM_INDEX_CLI ? JAM_CLI : JAM_PLAIN; }

int jam_recover_dev(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t kind, int32_t verify, jpk_jam_index **index, int32_t *ngaps)
{
    std::vector<JamFrame> fr;
    std::vector<JamGap> gaps;
    std::vector<int32_t> st;
    const bool cli = kind == JPK_JAM_INDEX_CLI;
    if (in_len > 0) {
        JPK_HIP(hipSetDevice(ctx->device));
        JamDevSrc src{ctx, d_in, in_len, jam_recover_walk_kind(kind), {}};
        JPK_TRY(jam_recover_walk(src, in_len, fr, gaps));
        st.assign(fr.size(), JPK_OK);
        for (size_t k = 0; k < fr.size();) {
            const size_t e = jam_recover_pass_end(fr, k, cli);
            if (cli) JPK_TRY(jam_cli_size_pass(ctx, d_in, 0, fr, k, e, false, st.data() + k));
            else JPK_TRY(jam_staged_size_pass(ctx, d_in, 0, fr, k, e, verify != 0, false, st.data() + k));
            k = e;
        }
    }
    if (!(*index = jam_recover_make(fr, st, gaps, in_len, kind))) return JPK_E_ALLOC;
    if (ngaps) *ngaps = (int32_t)(*index)->gaps.size();
    return JPK_OK;
}

int jam_recover_host(const uint8_t *in, int64_t in_len, int32_t kind, int32_t verify, jpk_jam_index **index, int32_t *ngaps)
{
    std::vector<JamFrame> fr;
    std::vector<JamGap> gaps;
    const int32_t K = g_recover_cands.load();
    std::vector<int64_t> offs((size_t)(K < 1 ? jrs::DEFAULT_CANDS : K));
    const bool cli = kind == JPK_JAM_INDEX_CLI;
    jrs::HostSrc src{in, in_len, kind == JPK_JAM_INDEX_STAGED, offs.data(), cli};
    JPK_TRY(jam_recover_walk(src, in_len, fr, gaps));
    std::vector<int32_t> st(fr.size(), JPK_OK);
    // an archive without a chained frame (of a stock-CLI archive, every frame is one) is indexed by the walk alone: no device is looked for
    auto chained = [cli](const JamFrame &f) { return cli || f.staged; };
    jpk_ctx *ctx = nullptr;
    if (std::any_of(fr.begin(), fr.end(), chained)) JPK_TRY(jpk_host_enter(&ctx, 0));
    for (size_t k = 0; k < fr.size();) {
        const size_t e = jam_recover_pass_end(fr, k, cli);
        if (std::any_of(fr.begin() + (ptrdiff_t)k, fr.begin() + (ptrdiff_t)e, chained)) {
            // staged one pass at a time, jam_stage_frames: the frames of the pass lie back to back
            int64_t len = 0, a0 = 0;
            JPK_TRY(jam_stage_frames(ctx, in, fr, k, e, &len, &a0));
            const int rc = cli ? jam_cli_size_pass(ctx, ctx->stage_in, a0, fr, k, e, false, st.data() + k)
                               : jam_staged_size_pass(ctx, ctx->stage_in, a0, fr, k, e, verify != 0, false, st.data() + k);
            JPK_HIP(hipStreamSynchronize(ctx->stream));
            JPK_TRY(rc);
        }
        k = e;
    }
    if (!(*index = jam_recover_make(fr, st, gaps, in_len, kind))) return JPK_E_ALLOC;
    if (ngaps) *ngaps = (int32_t)(*index)->gaps.size();
    return JPK_OK;
}
}  // namespace

extern "C" int jpk_dev_jam_index_recover(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int32_t kind, int32_t verify, jpk_jam_index **index, int32_t *gaps)
{
    // (the argument checks come before the first device call, and an empty archive makes none)
    if (!ctx || !jam_recover_args_ok(d_in, in_len, kind, verify, index)) return JPK_E_ARG;
    *index = nullptr;
    try {
        return jam_recover_dev(ctx, d_in, in_len, kind, verify, index, gaps);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(ctx->stream);
        return JPK_E_ALLOC;
    }
}

extern "C" int jpk_jam_index_recover(const uint8_t *in, int64_t in_len, int32_t kind, int32_t verify, jpk_jam_index **index, int32_t *gaps)
{
    if (!jam_recover_args_ok(in, in_len, kind, verify, index)) return JPK_E_ARG;
    *index = nullptr;
    try {
        return jam_recover_host(in, in_len, kind, verify, index, gaps);
    } catch (const std::bad_alloc &) {
        return JPK_E_ALLOC;
    }
}

extern "C" int jpk_jam_index_gaps(const jpk_jam_index *index) { return index ? (int)index->gaps.size() : JPK_E_ARG; }

extern "C" int jpk_jam_index_gap(const jpk_jam_index *index, int32_t g, int64_t *archive_off, int64_t *archive_len, int32_t *frame, int32_t *why)
{
    if (!index || g < 0 || (size_t)g >= index->gaps.size()) return JPK_E_ARG;
    const JamGap &x = index->gaps[(size_t)g];
    if (archive_off) *archive_off = x.archive_off;
    if (archive_len) *archive_len = x.archive_len;
    if (frame) *frame = x.frame;
    if (why) *why = x.why;
    return JPK_OK;
}

extern "C" int jpk_debug_jam_scan(jpk_ctx *ctx, const uint8_t *d_in, int64_t in_len, int64_t start, int64_t window, int32_t staged_ok, int32_t max_cands,
                                  int64_t *offsets, int32_t *count)
{
    if (!ctx || !count || in_len < 0 || (in_len > 0 && !d_in) || start < 0 || start > in_len || window < 0 || window > JAM_SCAN_MAX_WINDOW || max_cands < 1 ||
        max_cands > JAM_SCAN_MAX_CANDS || !offsets)
        return JPK_E_ARG;
    JPK_HIP(hipSetDevice(ctx->device));
    *count = 0;
    try {
        std::vector<JamWalkFrame> c;
        JPK_TRY(jam_scan_dev(ctx, d_in, in_len, start, std::min(in_len, start + window), staged_ok != 0, max_cands, c));
        for (size_t i = 0; i < c.size(); i++) offsets[i] = (int64_t)c[i].payload_off - JPK_JAM_HEADER_BYTES;
        *count = (int32_t)c.size();
    } catch (const std::bad_alloc &) {
        return JPK_E_ALLOC;
    }
    return JPK_OK;
}

// test hook (JPK_DEBUG_HOOKS=1 only): the window and the candidates per round of the resync search of this process; 0, 0: the defaults
extern "C" int jpk_debug_jam_recover_limits(int64_t window, int32_t max_cands)
{
    if (jpk_env_long("JPK_DEBUG_HOOKS", 0) == 0) return JPK_E_ARG;
    if (window < 0 || window > JAM_SCAN_MAX_WINDOW || max_cands < 0 || max_cands > JAM_SCAN_MAX_CANDS) return JPK_E_ARG;
    g_recover_window.store(window ? window : jrs::DEFAULT_WINDOW);
    g_recover_cands.store(max_cands ? max_cands : jrs::DEFAULT_CANDS);
    return JPK_OK;
}

namespace {
// the checks of both salvage entries, and the capacity answer: nothing is touched before they pass
int jam_salvage_check(const jpk_jam_index *ix, const void *in, int64_t in_len, const void *out, int64_t out_cap, int64_t *out_len)
{
    if (!ix || !out_len || in_len != ix->archive_len || out_cap < 0 || (in_len > 0 && !in) || (out_cap > 0 && !out)) return JPK_E_ARG;
    *out_len = ix->raw_off.back();
    return *out_len > out_cap ? JPK_E_CAPACITY : JPK_OK;
}

// one range per frame that has bytes -- every frame whole inside its range, so it decodes in its place -- through the reader's passes, then
// zeros where a frame failed.  The archive is d_in or (NULL) h_in, as in jam_read_run; d_out holds raw_len bytes
int jam_salvage_run(jpk_ctx *ctx, const jpk_jam_index *ix, const uint8_t *d_in, const uint8_t *h_in, uint8_t *d_out, int32_t *frame_status, int32_t *failed)
{
    const size_t F = ix->fr.size();
    std::vector<int64_t> off, len;
    std::vector<uint8_t *> outs;
    std::vector<size_t> of;
    for (size_t k = 0; k < F; k++) {
        if (frame_status) frame_status[k] = JPK_OK;
        if (ix->fr[k].raw == 0) continue;                     // no range touches it: reported JPK_OK, not verified
        of.push_back(k); off.push_back(ix->raw_off[k]); len.push_back(ix->fr[k].raw); outs.push_back(d_out + ix->raw_off[k]);
    }
    int32_t nfail = 0;
    if (!of.empty()) {
        std::vector<int32_t> st(of.size());
        JPK_TRY(jam_read_run(ctx, ix, d_in, h_in, (int32_t)of.size(), off.data(), len.data(), outs.data(), st.data(), nullptr));
        for (size_t r = 0; r < of.size(); r++) {
            if (st[r] == JPK_OK) continue;
            nfail++;
            if (frame_status) frame_status[of[r]] = JPK_E_CORRUPT;
            JPK_HIP(hipMemsetAsync(outs[r], 0, (size_t)len[r], ctx->stream));
        }
        JPK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (failed) *failed = nfail;
    return JPK_OK;
}
}  // namespace

extern "C" int jpk_dev_jam_salvage(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, uint8_t *d_out, int64_t out_cap, int64_t *out_len,
                                   int32_t *frame_status, int32_t *failed)
{
    // (the argument checks and the capacity answer come before the first device call)
    if (!ctx) return JPK_E_ARG;
    JPK_TRY(jam_salvage_check(index, d_in, in_len, d_out, out_cap, out_len));
    JPK_HIP(hipSetDevice(ctx->device));
    try {
        return jam_salvage_run(ctx, index, d_in, nullptr, d_out, frame_status, failed);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(ctx->stream);
        return JPK_E_ALLOC;
    }
}

extern "C" int jpk_jam_salvage(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *frame_status,
                               int32_t *failed)
{
    JPK_TRY(jam_salvage_check(index, in, in_len, out, out_cap, out_len));
    const int64_t raw_len = *out_len;
    if (raw_len == 0) {                                       // nothing to decode: no device is looked for
        for (size_t k = 0; frame_status && k < index->fr.size(); k++) frame_status[k] = JPK_OK;
        if (failed) *failed = 0;
        return JPK_OK;
    }
    jpk_ctx *ctx;
    JPK_TRY(jpk_host_enter(&ctx, 0));
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_res, &ctx->stage_res_cap, (size_t)raw_len + 64));
    try {
        JPK_TRY(jam_salvage_run(ctx, index, nullptr, in, ctx->stage_res, frame_status, failed));
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(ctx->stream);
        return JPK_E_ALLOC;
    }
    JPK_HIP(hipMemcpyAsync(out, ctx->stage_res, (size_t)raw_len, hipMemcpyDeviceToHost, ctx->stream));
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    return JPK_OK;
}

// ---- repair: the kept frames of an index, their headers and payloads unchanged, back to back -- an archive every whole-archive decoder reads to its end
namespace {
struct JamSpan { int64_t off, len; };       // a frame in the archive: its header and its payload

// the checks of both repair entries, the spans of the frames that stay and the capacity answer: nothing is touched before they pass
int jam_repair_plan(const jpk_jam_index *ix, const void *in, int64_t in_len, const int32_t *frame_status, const void *out, int64_t out_cap, int64_t *out_len,
                    int32_t *frames, std::vector<JamSpan> &keep)
{
    if (!ix || !out_len || in_len != ix->archive_len || out_cap < 0 || (in_len > 0 && !in) || (out_cap > 0 && !out)) return JPK_E_ARG;
    int64_t total = 0;
    for (size_t k = 0; k < ix->fr.size(); k++) {
        if (frame_status && frame_status[k] != JPK_OK) continue;
        const JamFrame &f = ix->fr[k];
        keep.push_back(JamSpan{f.payload_off - JPK_JAM_HEADER_BYTES, (int64_t)JPK_JAM_HEADER_BYTES + f.psize});
        total += keep.back().len;
    }
    *out_len = total;
    if (frames) *frames = (int32_t)keep.size();
    return total > out_cap ? JPK_E_CAPACITY : JPK_OK;
}
}  // namespace

extern "C" int jpk_dev_jam_repair(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, const int32_t *frame_status, uint8_t *d_out,
                                  int64_t out_cap, int64_t *out_len, int32_t *frames)
{
    // (the argument checks and the capacity answer come before the first device call, and an index without a kept frame makes none)
    if (!ctx) return JPK_E_ARG;
    try {
        std::vector<JamSpan> keep;
        JPK_TRY(jam_repair_plan(index, d_in, in_len, frame_status, d_out, out_cap, out_len, frames, keep));
        if (keep.empty()) return JPK_OK;
        JPK_HIP(hipSetDevice(ctx->device));
        // one piece per kept frame; the table is as long as the index, not as a pass
        JPK_TRY(jpk_buf_ensure(ctx, &ctx->jam_scratch, &ctx->jam_scratch_cap, keep.size() * sizeof(JamGatherPiece)));
        std::vector<JamGatherPiece> tab;
        tab.reserve(keep.size());
        uint64_t words = 0, pos = 0;
        for (const JamSpan &s : keep) {
            jam_piece_add(tab, &words, d_in + s.off, d_out + pos, (uint64_t)s.len, d_in, d_in + in_len);
            pos += (uint64_t)s.len;
        }
        JPK_TRY(jam_gather(ctx, reinterpret_cast<JamGatherPiece *>(ctx->jam_scratch), tab, words, pos));
        if (ctx->prof_on) jpk_prof_resolve(ctx);
        return JPK_OK;
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(ctx->stream);
        return JPK_E_ALLOC;
    }
}

extern "C" int jpk_jam_repair(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, const int32_t *frame_status, uint8_t *out, int64_t out_cap,
                              int64_t *out_len, int32_t *frames)
{
    try {
        std::vector<JamSpan> keep;
        JPK_TRY(jam_repair_plan(index, in, in_len, frame_status, out, out_cap, out_len, frames, keep));
        int64_t pos = 0;
        for (const JamSpan &s : keep) { memcpy(out + pos, in + s.off, (size_t)s.len); pos += s.len; }
        return JPK_OK;
    } catch (const std::bad_alloc &) {
        return JPK_E_ALLOC;
    }
}

// ---- update: byte ranges of an archive replaced, only the touched frames encoded again ("Updating an archive") -----------------
// The plan is jam_update_plan.hpp's: which frame is kept, which is rewritten, the pieces of the sources, the passes.  Per pass: the partly
// covered frames through the reader (jam_read_run, one whole-frame range each: every one decodes, verified, in place in its slot of
// ctx->jam_update), one gather launch that lays the sources over the slots, the compress pass in its general form (jam_compress_frames:
// payload slots in ctx->jam_scratch, sizes and crcs to the host), and one k_jam_splice launch that writes the stretch of the output the
// pass ends -- the kept frames since the pass before, copied from the archive, and the pass's new ones.  Behind the last pass one more
// splice for the kept frames that are left, then the tail through the passes of the whole-archive writer of the index's kind.  The new
// index is made of what these steps know; the output is not walked.  The host-buffer form runs the same passes: the payloads of the
// partly covered frames, the pieces of the sources and the tail travel to the device, the new payloads travel back, and the kept frames
// are copied with memcpy.
namespace {
int jam_update_kind(const jpk_jam_index *ix, const JamFrame &f) { return ix->kind == JPK_JAM_INDEX_CLI ? JAM_CLI : f.staged ? JAM_STAGED : JAM_PLAIN; }
int jam_update_tail_kind(const jpk_jam_index *ix) { return ix->kind == JPK_JAM_INDEX_CLI ? JAM_CLI : ix->kind == JPK_JAM_INDEX_STAGED ? JAM_STAGED : JAM_PLAIN; }

// what the bound and both entries refuse alike, and the plan of what they take; *bound = jpk_jam_update_bound's answer, *least = what the
// output holds at least (the kept spans and a header per new frame)
int jam_update_plan(const jpk_jam_index *ix, int32_t n, const int64_t *off, const int64_t *len, int64_t tail_len, int32_t tail_block_size, jup::Plan *plan,
                    int64_t *bound, int64_t *least)
{
    if (!ix || tail_len < 0 || (tail_len > 0 && !jpk_jam_block_size_ok(tail_block_size))) return JPK_E_ARG;
    if (!jup::check(ix->raw_off, n, off, len)) return JPK_E_ARG;
    const bool cli = ix->kind == JPK_JAM_INDEX_CLI;
    std::vector<int64_t> weight(ix->fr.size());
    for (size_t k = 0; k < weight.size(); k++) weight[k] = jam_weight(ix->fr[k], cli);
    *plan = jup::make(ix->raw_off, weight, n, off, len, jup::Limits{(size_t)JPK_JAM_PASS_FRAMES, JAM_PASS_RAW});
    int64_t sum = 0, low = 0;
    for (size_t k = 0; k < ix->fr.size(); k++) {
        const JamFrame &f = ix->fr[k];
        if (plan->cls[k] == jup::KEPT) { sum += (int64_t)JPK_JAM_HEADER_BYTES + f.psize; low += (int64_t)JPK_JAM_HEADER_BYTES + f.psize; }
        else { sum += jam_frame_bound((int32_t)f.raw, jam_update_kind(ix, f) != JAM_PLAIN); low += JPK_JAM_HEADER_BYTES; }
    }
    if (tail_len > 0) {
        sum += jam_compress_bound(tail_len, tail_block_size, jam_update_tail_kind(ix) != JAM_PLAIN);
        low += (int64_t)JPK_JAM_HEADER_BYTES * ((tail_len + tail_block_size - 1) / tail_block_size);
    }
    *bound = sum;
    if (least) *least = low;
    return JPK_OK;
}

// the arguments of either entry: the archive, the sources, the tail and the output are device buffers, or (host) host buffers
struct JamUpdate {
    const jpk_jam_index *ix;
    const uint8_t *in; int64_t in_len;
    int32_t n; const int64_t *off, *len; const uint8_t *const *src;
    const uint8_t *tail; int64_t tail_len; int32_t tail_block_size;
    uint32_t flags; int32_t in_flight;
    uint8_t *out; int64_t out_cap; int64_t *out_len;
    jpk_jam_index **new_index; int32_t *rewritten, *bad_frame;
    bool host;
};

// the argument checks, the plan and the first capacity answer: no device is looked for, nothing is written before they pass
int jam_update_check(const JamUpdate &u, jup::Plan *plan, int64_t *bound)
{
    if (!u.ix || !u.out_len || !u.new_index || u.in_len != u.ix->archive_len || u.out_cap < 0 || (u.in_len > 0 && !u.in) || (u.out_cap > 0 && !u.out) ||
        !JPK_CLI_FLAGS_OK(u.flags) || u.n < 0 || (u.n > 0 && (!u.off || !u.len || !u.src)) || u.tail_len < 0 || (u.tail_len > 0 && !u.tail))
        return JPK_E_ARG;
    for (int32_t r = 0; r < u.n; r++) if (u.len[r] > 0 && !u.src[r]) return JPK_E_ARG;
    int64_t least = 0;
    JPK_TRY(jam_update_plan(u.ix, u.n, u.off, u.len, u.tail_len, u.tail_block_size, plan, bound, &least));
    *u.new_index = nullptr;
    if (u.bad_frame) *u.bad_frame = -1;
    if (u.rewritten) *u.rewritten = (int32_t)plan->rewritten.size();
    *u.out_len = *bound;
    return least > u.out_cap ? JPK_E_CAPACITY : JPK_OK;
}

// frames [f0, f1) of the index, every one kept, to out + *pos: one splice launch, or (host) a memcpy per frame
int jam_update_kept(jpk_ctx *ctx, const JamUpdate &u, int32_t f0, int32_t f1, int64_t *pos, std::vector<JamFrame> &done)
{
    if (f0 >= f1) return JPK_OK;
    std::vector<JamSpliceFrame> tab;
    uint64_t o = 0;
    for (int32_t f = f0; f < f1; f++) {
        const JamFrame &x = u.ix->fr[(size_t)f];
        tab.push_back(JamSpliceFrame{o, u.in + x.payload_off - JPK_JAM_HEADER_BYTES, x.psize, x.crc, 0, 1});
        o += (uint64_t)JPK_JAM_HEADER_BYTES + (uint64_t)x.psize;
    }
    if ((int64_t)o > u.out_cap - *pos) return JPK_E_CAPACITY;
    if (u.host) {
        for (const JamSpliceFrame &t : tab) memcpy(u.out + *pos + t.off, t.src, (size_t)JPK_JAM_HEADER_BYTES + (size_t)t.psize);
    } else {
        JPK_TRY(jpk_buf_ensure(ctx, &ctx->jam_update, &ctx->jam_update_cap, tab.size() * sizeof(JamSpliceFrame)));
        JamSpliceFrame *d_tab = reinterpret_cast<JamSpliceFrame *>(ctx->jam_update);
        JPK_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(JamSpliceFrame), hipMemcpyHostToDevice, ctx->stream));
        JPK_TRY(jpk_jam_splice_enqueue(ctx, d_tab, (uint32_t)tab.size(), u.out + *pos, o, u.in, u.in + u.in_len));
        JPK_HIP(hipStreamSynchronize(ctx->stream));
    }
    for (int32_t f = f0; f < f1; f++) {
        done.push_back(u.ix->fr[(size_t)f]);
        done.back().payload_off = *pos + (int64_t)tab[(size_t)(f - f0)].off + JPK_JAM_HEADER_BYTES;
    }
    *pos += (int64_t)o;
    return JPK_OK;
}

// one pass of the plan: its partly covered frames decoded, the sources laid over its slots, its frames compressed, its stretch written
int jam_update_pass(jpk_ctx *ctx, const JamUpdate &u, const jup::Plan &plan, const jup::Pass &ps, int64_t *pos, std::vector<JamFrame> &done)
{
    const jpk_jam_index *ix = u.ix;
    const size_t m = ps.q1 - ps.q0, p0 = plan.piece_at[ps.q0], p1 = plan.piece_at[ps.q1];
    // ctx->jam_update: the gather table | the splice table | (host) the pieces of the sources | a slot per rewritten frame, padded as the reader's are
    size_t src_bytes = 0, slot_bytes = 0;
    if (u.host) for (size_t i = p0; i < p1; i++) src_bytes += (size_t)plan.pieces[i].len;
    for (size_t q = ps.q0; q < ps.q1; q++) slot_bytes += jpk_align((size_t)ix->fr[(size_t)plan.rewritten[q]].raw + 64);
    const size_t o_splice = jpk_align((p1 - p0) * sizeof(JamGatherPiece)), o_src = o_splice + jpk_align((size_t)(ps.f1 - ps.f0) * sizeof(JamSpliceFrame)),
                 o_slots = o_src + jpk_align(src_bytes + 64);
    JPK_TRY(jpk_buf_ensure(ctx, &ctx->jam_update, &ctx->jam_update_cap, o_slots + slot_bytes));
    uint8_t *const d_srcs = ctx->jam_update + o_src;
    std::vector<uint8_t *> slot(m);
    {
        size_t o = o_slots;
        for (size_t q = 0; q < m; q++) { slot[q] = ctx->jam_update + o; o += jpk_align((size_t)ix->fr[(size_t)plan.rewritten[ps.q0 + q]].raw + 64); }
    }
    // 1. the partly covered frames: one whole-frame range each, so the reader decodes every one in place in its slot and verifies it
    {
        std::vector<int64_t> roff, rlen;
        std::vector<uint8_t *> rout;
        for (size_t q = 0; q < m; q++) {
            const size_t f = (size_t)plan.rewritten[ps.q0 + q];
            if (plan.cls[f] != jup::PART) continue;
            roff.push_back(ix->raw_off[f]); rlen.push_back(ix->fr[f].raw); rout.push_back(slot[q]);
        }
        if (!roff.empty()) {
            std::vector<int32_t> st(roff.size());
            int32_t bad = -1;
            JPK_TRY(jam_read_run(ctx, ix, u.host ? nullptr : u.in, u.host ? u.in : nullptr, (int32_t)roff.size(), roff.data(), rlen.data(), rout.data(), st.data(), &bad));
            if (bad >= 0) {
                JPK_HIP(hipStreamSynchronize(ctx->stream));
                if (u.bad_frame) *u.bad_frame = bad;
                for (int32_t s : st) if (s != JPK_OK) return s;
                return JPK_E_CORRUPT;
            }
        }
    }
    // 2. the sources over the slots, one gather launch
    {
        std::vector<JamGatherPiece> tab;
        tab.reserve(p1 - p0);
        uint64_t words = 0, bytes = 0;
        size_t at = 0;
        for (size_t q = 0; q < m; q++)
            for (size_t i = plan.piece_at[ps.q0 + q]; i < plan.piece_at[ps.q0 + q + 1]; i++) {
                const jup::Piece &pc = plan.pieces[i];
                const uint8_t *from = u.src[pc.write] + pc.write_off, *lo = u.src[pc.write], *hi = lo + u.len[pc.write];
                if (u.host) {
                    JPK_HIP(hipMemcpyAsync(d_srcs + at, from, (size_t)pc.len, hipMemcpyHostToDevice, ctx->stream));
                    from = d_srcs + at; lo = d_srcs; hi = d_srcs + src_bytes;
                    at += (size_t)pc.len;
                }
                jam_piece_add(tab, &words, from, slot[q] + pc.frame_off, (uint64_t)pc.len, lo, hi);
                bytes += (uint64_t)pc.len;
            }
        JPK_TRY(jam_gather(ctx, reinterpret_cast<JamGatherPiece *>(ctx->jam_update), tab, words, bytes));
    }
    // 3. the new frames: each keeps its raw size, its BlockSize and its kind
    std::vector<JamNewFrame> nf(m);
    for (size_t q = 0; q < m; q++) {
        const JamFrame &f = ix->fr[(size_t)plan.rewritten[ps.q0 + q]];
        nf[q] = JamNewFrame{slot[q], (int32_t)f.raw, f.block_size, jam_update_kind(ix, f)};
    }
    std::vector<JamPayload> made;
    uint8_t *unused = nullptr;
    JPK_TRY(jam_compress_frames(ctx, nf, u.flags, u.in_flight, made, &unused));
    // 4. the stretch: the kept frames since the pass before and between the new ones, and the new ones
    std::vector<JamSpliceFrame> tab;
    tab.reserve((size_t)(ps.f1 - ps.f0));
    uint64_t o = 0;
    size_t q = 0;
    for (int32_t f = ps.f0; f < ps.f1; f++) {
        const JamFrame &x = ix->fr[(size_t)f];
        if (plan.cls[(size_t)f] == jup::KEPT) tab.push_back(JamSpliceFrame{o, u.in + x.payload_off - JPK_JAM_HEADER_BYTES, x.psize, x.crc, 0, 1});
        else {
            tab.push_back(JamSpliceFrame{o, made[q].slot, made[q].psize, made[q].crc, x.staged ? (x.block_size | JPK_JAM_STAGED) : x.block_size, 0});
            q++;
        }
        o += (uint64_t)JPK_JAM_HEADER_BYTES + (uint64_t)tab.back().psize;
    }
    if ((int64_t)o > u.out_cap - *pos) return JPK_E_CAPACITY;
    if (u.host) {
        // only the new payloads travel back; the kept frames are the host's own bytes
        for (const JamSpliceFrame &t : tab) {
            uint8_t *at = u.out + *pos + t.off;
            if (t.kept) { memcpy(at, t.src, (size_t)JPK_JAM_HEADER_BYTES + (size_t)t.psize); continue; }
            jpk_jam_header_write(at, t.crc, t.psize, t.field);
            if (t.psize) JPK_HIP(hipMemcpyAsync(at + JPK_JAM_HEADER_BYTES, t.src, (size_t)t.psize, hipMemcpyDeviceToHost, ctx->stream));
        }
    } else {
        JamSpliceFrame *d_tab = reinterpret_cast<JamSpliceFrame *>(ctx->jam_update + o_splice);
        JPK_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(JamSpliceFrame), hipMemcpyHostToDevice, ctx->stream));
        JPK_TRY(jpk_jam_splice_enqueue(ctx, d_tab, (uint32_t)tab.size(), u.out + *pos, o, u.in, u.in + u.in_len));
    }
    JPK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof_on) jpk_prof_resolve(ctx);
    for (int32_t f = ps.f0; f < ps.f1; f++) {
        const JamSpliceFrame &t = tab[(size_t)(f - ps.f0)];
        done.push_back(ix->fr[(size_t)f]);
        JamFrame &d = done.back();
        d.payload_off = *pos + (int64_t)t.off + JPK_JAM_HEADER_BYTES;
        if (!t.kept) { d.psize = t.psize; d.crc = t.crc; }
    }
    *pos += (int64_t)o;
    return JPK_OK;
}

// the tail: new frames behind the last one, through the passes of the whole-archive writer of the index's kind (host: staged pass by pass)
int jam_update_tail(jpk_ctx *ctx, const JamUpdate &u, int64_t *pos, std::vector<JamFrame> &done)
{
    const int kind = jam_update_tail_kind(u.ix);
    const int32_t bs = u.tail_block_size;
    const int64_t step = (int64_t)jam_pass_frames(bs) * bs;
    for (int64_t o = 0; o < u.tail_len; o += step) {
        const int64_t len = std::min(step, u.tail_len - o);
        const size_t first = done.size();
        int64_t got = 0;
        if (u.host) {
            const int64_t room = jam_compress_bound(len, bs, kind != JAM_PLAIN);
            JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_in, &ctx->stage_in_cap, (size_t)len + 64));
            JPK_TRY(jpk_buf_ensure(ctx, &ctx->stage_res, &ctx->stage_res_cap, (size_t)room + 64));
            JPK_HIP(hipMemcpyAsync(ctx->stage_in, u.tail + o, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
            JPK_TRY(jam_compress_pass(ctx, ctx->stage_in, len, bs, ctx->stage_res, room, &got, u.in_flight, kind, u.flags, &done));
            if (got > u.out_cap - *pos) return JPK_E_CAPACITY;
            JPK_HIP(hipMemcpyAsync(u.out + *pos, ctx->stage_res, (size_t)got, hipMemcpyDeviceToHost, ctx->stream));
            JPK_HIP(hipStreamSynchronize(ctx->stream));
        } else {
            JPK_TRY(jam_compress_pass(ctx, u.tail + o, len, bs, u.out + *pos, u.out_cap - *pos, &got, u.in_flight, kind, u.flags, &done));
        }
        for (size_t i = first; i < done.size(); i++) done[i].payload_off += *pos;
        *pos += got;
    }
    return JPK_OK;
}

// the update behind its checks.  ctx may be NULL when the plan has no pass and there is no tail (the host form then makes no device call)
int jam_update_run(jpk_ctx *ctx, const JamUpdate &u, const jup::Plan &plan, int64_t bound)
{
    std::vector<JamFrame> done;
    done.reserve(u.ix->fr.size());
    int64_t pos = 0;
    int rc = JPK_OK;
    for (size_t p = 0; p < plan.passes.size() && rc == JPK_OK; p++) rc = jam_update_pass(ctx, u, plan, plan.passes[p], &pos, done);
    if (rc == JPK_OK) rc = jam_update_kept(ctx, u, plan.tail_f0, (int32_t)u.ix->fr.size(), &pos, done);
    if (rc == JPK_OK) rc = jam_update_tail(ctx, u, &pos, done);
    if (rc != JPK_OK) {
        if (rc == JPK_E_CAPACITY) *u.out_len = bound;
        return rc;
    }
    if (!(*u.new_index = jam_index_make(done, pos, -1, u.ix->kind))) return JPK_E_ALLOC;
    *u.out_len = pos;
    return JPK_OK;
}
}  // namespace

extern "C" int64_t jpk_jam_update_bound(const jpk_jam_index *index, int32_t n, const int64_t *off, const int64_t *len, int64_t tail_len, int32_t tail_block_size)
{
    try {
        jup::Plan plan;
        int64_t bound = 0;
        const int rc = jam_update_plan(index, n, off, len, tail_len, tail_block_size, &plan, &bound, nullptr);
        return rc != JPK_OK ? rc : bound;
    } catch (const std::bad_alloc &) {
        return JPK_E_ALLOC;
    }
}

extern "C" int jpk_dev_jam_update(jpk_ctx *ctx, const jpk_jam_index *index, const uint8_t *d_in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len,
                                  const uint8_t *const *d_src, const uint8_t *d_tail, int64_t tail_len, int32_t tail_block_size, uint32_t flags, int32_t in_flight,
                                  uint8_t *d_out, int64_t out_cap, int64_t *out_len, jpk_jam_index **new_index, int32_t *rewritten, int32_t *bad_frame)
{
    // (the argument checks and the first capacity answer come before the first device call)
    if (!ctx) return JPK_E_ARG;
    try {
        const JamUpdate u{index, d_in, in_len, n, off, len, d_src, d_tail, tail_len, tail_block_size, flags, in_flight, d_out, out_cap, out_len, new_index, rewritten,
                          bad_frame, false};
        jup::Plan plan;
        int64_t bound = 0;
        JPK_TRY(jam_update_check(u, &plan, &bound));
        JPK_HIP(hipSetDevice(ctx->device));
        return jam_update_run(ctx, u, plan, bound);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(ctx->stream);
        return JPK_E_ALLOC;
    }
}

extern "C" int jpk_jam_update(const jpk_jam_index *index, const uint8_t *in, int64_t in_len, int32_t n, const int64_t *off, const int64_t *len,
                              const uint8_t *const *src, const uint8_t *tail, int64_t tail_len, int32_t tail_block_size, uint32_t flags, int32_t in_flight, uint8_t *out,
                              int64_t out_cap, int64_t *out_len, jpk_jam_index **new_index, int32_t *rewritten, int32_t *bad_frame)
{
    jpk_ctx *ctx = nullptr;
    try {
        const JamUpdate u{index, in, in_len, n, off, len, src, tail, tail_len, tail_block_size, flags, in_flight, out, out_cap, out_len, new_index, rewritten, bad_frame,
                          true};
        jup::Plan plan;
        int64_t bound = 0;
        JPK_TRY(jam_update_check(u, &plan, &bound));
        // no frame to rewrite and no tail: jpk_jam_repair's copies, and no device is looked for
        if (!plan.passes.empty() || tail_len > 0) JPK_TRY(jpk_host_enter(&ctx, 0));
        return jam_update_run(ctx, u, plan, bound);
    } catch (const std::bad_alloc &) {
        if (ctx) (void)hipStreamSynchronize(ctx->stream);
        return JPK_E_ALLOC;
    }
}
