// lz_expand.hpp -- the rule of the parallel LZ77 expanders (jpk_dev_blocks_lz77_expand and, with the deep rule at the end of this file,
// jpk_dev_blocks_lz77_expand_deep; DESIGN 4.6, "Staged frames"), shared by its host form (the stand-alone rule tests) and the k_lzx_* and
// k_lzd_* kernels (prestage_dev.hip): the plan, which turns the token stream into one segment
// record per literal run and per match with the checks of Lz77::Decompress in their order, and the chase, which finds the input byte
// behind any output position from the records alone.  Pure functions of the stream, so the result depends on no launch order.
#pragma once
#include <stdint.h>

#include "../../include/jampack_abi.h"
#include "prestage_rules.hpp"

namespace lzx {

constexpr uint32_t MAX_CHASE = 8;           // match hops from an output byte to its literal; a block that needs more is decoded serially

// `len` output bytes from `out`: input bytes from src (match == 0), or the bytes `src` in front of them, repeated with period src (match == 1)
struct Seg { uint32_t out, len, src, match; };

// records a block may use: the dedupe writes at most n / 256 + 2 tokens of two records each
JPK_HD uint32_t seg_cap(int64_t in_len) { return (uint32_t)(in_len / 64 + 4); }

// the walk over the tokens: pos / op as in jpk_lz77_decompress; serial = the block fails a check or needs more than `cap` records and
// goes to the serial decoder, which gives it its status
struct Plan { int64_t pos = 0, op = 0; uint32_t nseg = 0; bool done = false, serial = false; };

JPK_HD bool more(const Plan &p, int64_t in_len) { return !p.done && p.pos < in_len; }

// One token: t was parsed at p.pos (parsed == false: pre::parse_token refused it).  put(i, seg) stores record i.  No record is empty, the
// records are in output order and the first one starts at 0.
template <class Put> JPK_HD void step(Plan &p, bool parsed, const pre::Token &t, int64_t in_len, int64_t out_cap, uint32_t cap, Put put)
{
    auto fail = [&p]() { p.serial = true; p.done = true; };
    auto add = [&](int64_t len, int64_t src, uint32_t match) {
        if (len == 0) return true;
        if (p.nseg >= cap) { fail(); return false; }
        Seg s;
        s.out = (uint32_t)p.op; s.len = (uint32_t)len; s.src = (uint32_t)src; s.match = match;     // all below 2^31: checked against in_len / out_cap
        put(p.nseg++, s);
        p.op += len;
        return true;
    };
    if (!parsed) return fail();
    p.pos += t.used;
    if (t.off == 0) {                                                  // end marker: raw remainder
        const int64_t rest = in_len - p.pos;
        if (p.op + rest > out_cap) return fail();
        add(rest, p.pos, 0u);
        p.done = true;
        return;
    }
    if (t.off < 0 || t.lit > in_len - p.pos) return fail();
    if (t.lit + t.len > out_cap - p.op) return fail();
    if (!add(t.lit, p.pos, 0u)) return;
    p.pos += t.lit;
    if ((int64_t)t.off > p.op) return fail();
    add(t.len, t.off, 1u);
}

// ---- the size rule: the same walk for the raw size alone (jpk_lz77_size, k_lz77_sizes) ---------------------------------------------------
// What jpk_lz77_decompress / k_pre_lz77 answer for a stream without its bytes: the status by their checks in their order -- the two
// failures apart, and no record cap, which is why this is not lzx::step -- and op, the sum of the literal and match lengths.
struct Size { int64_t pos = 0, op = 0; int32_t status = JPK_OK; bool done = false; };

JPK_HD bool more(const Size &s, int64_t in_len) { return !s.done && s.pos < in_len; }

// One token: t was parsed at s.pos (parsed == false: pre::parse_token refused it).  s.pos grows by the token's bytes at least.
JPK_HD void step(Size &s, bool parsed, const pre::Token &t, int64_t in_len, int64_t out_cap)
{
    auto fail = [&s](int32_t status) { s.status = status; s.done = true; };
    if (!parsed) return fail(JPK_E_CORRUPT);
    s.pos += t.used;
    if (t.off == 0) {                                                  // end marker: raw remainder
        const int64_t rest = in_len - s.pos;
        if (s.op + rest > out_cap) return fail(JPK_E_CAPACITY);
        s.op += rest;
        s.done = true;
        return;
    }
    if (t.off < 0 || t.lit > in_len - s.pos) return fail(JPK_E_CORRUPT);
    if (t.lit + t.len > out_cap - s.op) return fail(JPK_E_CAPACITY);
    s.op += t.lit;
    s.pos += t.lit;
    if ((int64_t)t.off > s.op) return fail(JPK_E_CORRUPT);
    s.op += t.len;
}

// the out_len of both decoders: 0 unless the stream is good (op <= out_cap < 2^31)
JPK_HD int32_t out_len(const Size &s) { return s.status == JPK_OK ? (int32_t)s.op : 0; }

// the record of output position pos among s[0..n): the last one with out <= pos (n >= 1)
JPK_HD uint32_t find(const Seg *s, uint32_t n, uint32_t pos)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s[mid].out <= pos) lo = mid; else hi = mid; }
    return lo;
}

// where a position of match sg reads: in front of the match in one step, however long an overlapping match is
JPK_HD uint32_t back(const Seg &sg, uint32_t pos) { return sg.out - sg.src + (pos - sg.out) % sg.src; }

// The input byte behind output position pos, which lies in record idx = sg: *in_off.  Every hop lands in an earlier record (a match is
// never record 0: its offset would exceed the output so far), so the chase ends; false: it needs more than `hops` hops.
JPK_HD bool source(const Seg *s, uint32_t idx, Seg sg, uint32_t pos, uint32_t hops, uint32_t *in_off)
{
    for (uint32_t k = 0;; k++) {
        if (!sg.match) { *in_off = sg.src + (pos - sg.out); return true; }
        if (k == hops) return false;
        pos = back(sg, pos);
        idx = find(s, idx, pos);
        sg = s[idx];
    }
}

// the expander's chase: MAX_CHASE hops
JPK_HD bool source(const Seg *s, uint32_t idx, Seg sg, uint32_t pos, uint32_t *in_off) { return source(s, idx, sg, pos, MAX_CHASE, in_off); }

// ---- the deep rule: the same plan and chase with a record budget in output terms and a larger hop cap (jpk_dev_blocks_lz77_expand_deep,
// k_lzd_plan / k_lzd_copy; DESIGN 4.6, "The deep expander") ----------------------------------------------------------------------------
// The dedupe writes matches of at least dd::MIN_MATCH = 256 bytes and at most two records per token, so behind every token of a stream
// it wrote records <= op / 128 + 2.  The deep plan gives a block up as soon as records > op / DEEP_BYTES + DEEP_SLACK behind a token: a
// dense stream is left within its first tokens, and a stream inside the budget has at most out_cap / 128 + 4 records behind a token and
// two more inside one -- deep_seg_cap, which the host knows without reading the stream.
constexpr uint32_t DEEP_CHASE = 32;         // hops: twice the deepest dedupe stream measured (15 at 64 MiB of real sources), as a power of two
constexpr uint32_t DEEP_BYTES = 128;        // output bytes that pay for one record
constexpr uint32_t DEEP_SLACK = 4;          // records a stream may be ahead of its output

JPK_HD uint32_t deep_seg_cap(int64_t out_cap) { return (uint32_t)(out_cap / DEEP_BYTES + DEEP_SLACK + 4); }

JPK_HD bool deep_over(const Plan &p) { return (int64_t)p.nseg > p.op / (int64_t)DEEP_BYTES + (int64_t)DEEP_SLACK; }

// One token of the deep plan: lzx::step with the array's size as its cap (never reached inside the budget), then the budget
template <class Put> JPK_HD void deep_step(Plan &p, bool parsed, const pre::Token &t, int64_t in_len, int64_t out_cap, uint32_t cap, Put put)
{
    step(p, parsed, t, in_len, out_cap, cap, put);
    if (!p.serial && deep_over(p)) { p.serial = true; p.done = true; }
}

}  // namespace lzx
