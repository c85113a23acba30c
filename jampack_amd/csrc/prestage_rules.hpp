// prestage_rules.hpp -- the rules of the stock CLI's pre-stages that the host forms (prestage.cpp) and the kernels
// (prestage_dev.hip) share, so that both compute the same bytes and the same statuses by construction: the LEB128 code, the LZ77 token,
// the LPX model with its part cut and its one step, the sizes and the LPC recurrence of the filter stage, and the writer's choice among the
// delta filters (its integer cost, the order of its walk, the transformed bytes).  Pure functions, no HIP
// header: the file compiles with a plain C++17 compiler, where the serial walk of the LPX kernels runs under a sanitizer.  The copy
// loops, scans and word assembly are shapes of their own and stay with their forms; the rule of the dedupe is dedupe.hpp.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define JPK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define JPK_HD inline
#endif

namespace pre {

// ---- LEB128 "with carry" (Utils::EncodeLeb128 / DecodeLeb128, utils.cpp:22-90) ------------------------------------------------------
// Big-endian 7-bit groups, the last byte has bit 7 set; a code of d + 1 bytes starts at LEB_OFF[d - 1], where the shorter ones end.
constexpr uint32_t LEB_OFF[4] = {127u, 16510u, 2113661u, 270549116u};

// the value whose bytes are get(0), get(1), ... with `avail` of them in the stream; returns bytes consumed or -1
template <class Get> JPK_HD int leb_read(Get get, int64_t avail, uint32_t *v)
{
    int d = 0;
    uint32_t x = 0, b;
    for (;;) {
        if (d >= avail) return -1;
        b = get(d);
        if (b & 0x80u) break;
        if (d >= 4) return -1;
        x = (x << 7) | b;
        d++;
    }
    x = (x << 7) | (b & 0x7fu);
    if (d > 0) x += d == 1 ? LEB_OFF[0] : (d == 2 ? LEB_OFF[1] : (d == 3 ? LEB_OFF[2] : LEB_OFF[3]));   // selects: no table load in a kernel
    *v = x;
    return d + 1;
}
// the same for bytes in memory (pass a pointer to const: any other argument is taken for a getter)
JPK_HD int leb_read(const uint8_t *b, int64_t avail, uint32_t *v)
{
    return leb_read([b](int j) { return (uint32_t)b[j]; }, avail, v);
}

// returns bytes written, at most 5
JPK_HD uint32_t leb_write(uint32_t v, uint8_t *b)
{
    if (v < LEB_OFF[0]) { b[0] = (uint8_t)(v | 0x80u); return 1; }
    if (v < LEB_OFF[1]) { v -= LEB_OFF[0]; b[0] = (uint8_t)((v >> 7) & 0x7fu); b[1] = (uint8_t)((v & 0x7fu) | 0x80u); return 2; }
    if (v < LEB_OFF[2]) {
        v -= LEB_OFF[1];
        b[0] = (uint8_t)((v >> 14) & 0x7fu); b[1] = (uint8_t)((v >> 7) & 0x7fu); b[2] = (uint8_t)((v & 0x7fu) | 0x80u);
        return 3;
    }
    if (v < LEB_OFF[3]) {
        v -= LEB_OFF[2];
        b[0] = (uint8_t)((v >> 21) & 0x7fu); b[1] = (uint8_t)((v >> 14) & 0x7fu); b[2] = (uint8_t)((v >> 7) & 0x7fu);
        b[3] = (uint8_t)((v & 0x7fu) | 0x80u);
        return 4;
    }
    v -= LEB_OFF[3];
    b[0] = (uint8_t)((v >> 28) & 0x7fu); b[1] = (uint8_t)((v >> 21) & 0x7fu); b[2] = (uint8_t)((v >> 14) & 0x7fu);
    b[3] = (uint8_t)((v >> 7) & 0x7fu); b[4] = (uint8_t)((v & 0x7fu) | 0x80u);
    return 5;
}

// ---- LZ77 token (lz77.cpp:75-98) ----------------------------------------------------------------------------------------------------
// One byte = match length class (5 bits) | literal count class (3 bits), then the offset, then the extensions of a saturated class; match
// lengths are stored minus 4 (MIN_MATCH, lz77.hpp:33).  At most 16 bytes.  len and lit are 64-bit: the extensions are attacker-controlled.
constexpr uint8_t END_TOKEN[2] = {0x04, 0x80};    // WriteToken(MIN_MATCH, MIN_MATCH, 0) (lz77.cpp:620): offset 0, the rest is copied through
struct Token { int32_t off; int64_t len, lit; int used; };

// the token whose bytes are get(0), ... with avail >= 1 of them in the stream; false: corrupt
template <class Get> JPK_HD bool parse_token(Get get, int64_t avail, Token *t)
{
    const uint32_t token = get(0);
    int at = 1;
    auto leb = [&](int32_t *v) {
        uint32_t x = 0;
        const int n = leb_read([&](int j) { return get(at + j); }, avail - at, &x);
        *v = (int32_t)x;
        at += n;
        return n >= 0;
    };
    int32_t e = 0;
    t->len = (int64_t)(token >> 3);
    t->lit = (int64_t)(token & 7u);
    if (!leb(&t->off)) return false;
    if (t->len == 31) { if (!leb(&e) || e < 0) return false; t->len += e; }
    t->len += 4;
    if (t->lit == 7) { if (!leb(&e) || e < 0) return false; t->lit += e; }
    t->used = at;
    return true;
}

// ---- LPX: localized prefix model (lpx.hpp:12-24) ------------------------------------------------------------------------------------
// Three tables (context orders 1..3) of 256 records keyed by the leading prefix byte; the decoder mirrors the encoder's table walk.
struct Record { uint32_t cxt, pos, hits, miss; int32_t threshold; };
constexpr int LPX_MAX_THRESHOLD = 128, LPX_MIN_THRESHOLD = 4;
constexpr uint32_t LPX_MAX_RECORD = 64u << 10;
constexpr uint32_t LPX_TILE = 16u << 10;                         // the kernels' tile
constexpr uint32_t LPX_RING = LPX_MAX_RECORD + LPX_TILE;         // their ring: position p lives at p mod LPX_RING until p + LPX_RING is written

JPK_HD Record fresh_record()
{
    Record r;
    r.cxt = 0; r.pos = 0; r.hits = 0; r.miss = 0; r.threshold = LPX_MAX_THRESHOLD >> 1;
    return r;
}

// lpx.cpp:11-52.  Note the reference re-indexes the table with the *updated* order for the threshold adjustments.
JPK_HD void update(Record (*table)[256], uint32_t cxt, int &order, uint32_t pos)
{
    const uint32_t lp = (cxt >> (order * 8)) & 0xffu;
    const uint32_t ls = cxt & ((1u << (order * 8)) - 1u);
    Record *r = &table[order - 1][lp];
    const int32_t distance = (int32_t)(pos - r->pos);
    const int32_t lower = LPX_MIN_THRESHOLD;
    int32_t upper;
    if (r->hits < (uint32_t)LPX_MAX_THRESHOLD) upper = distance > LPX_MIN_THRESHOLD ? distance : LPX_MIN_THRESHOLD;
    else { const int32_t a = distance >> order, b = LPX_MAX_THRESHOLD >> order; upper = a < b ? a : b; }
    const int32_t bound = (distance <= lower) ? lower : (distance > upper ? upper : distance);
    if (pos <= (uint32_t)order) return;
    if (r->cxt == ls) {
        r->pos = pos - (uint32_t)order;
        r->hits++;
        r->miss = 0;
        if (r->hits > (uint32_t)((r->threshold << order) << 3) && order > 1 && order <= 3) order--;
        r = &table[order - 1][lp];
        if (r->hits > (uint32_t)(r->threshold << 1) && r->miss == 0) r->threshold += (bound - r->threshold) >> order;
    } else {
        r->hits >>= 2;
        r->miss++;
        r->cxt = ls;
        if (r->miss > (uint32_t)(r->threshold * r->threshold * order) && order >= 1 && order < 3) order++;
        r = &table[order - 1][lp];
        if (r->miss > (uint32_t)r->threshold) r->threshold += (LPX_MAX_THRESHOLD - r->threshold) >> (4 - order);
    }
}

// Lpx::Encode / Lpx::Decode (lpx.cpp:148-169) cut a block by `for (i = 0; i < len; i += len / 4)`, each part with a fresh model: four
// parts, more when len is not a multiple of 4 (a fifth, short one; up to seven for len < 8).  The reference loops forever for 0 < len < 4
// (part size 0); no encoder output can be that short, so such a block is one part.
JPK_HD uint32_t parts(uint32_t len)
{
    const uint32_t part = len / 4u;
    return part ? (len + part - 1) / part : (len ? 1u : 0u);
}
// part pi of the block; false: there is no such part
JPK_HD bool part_of(uint32_t len, uint32_t pi, uint32_t *start, uint32_t *plen)
{
    const uint32_t part = len / 4u;
    *start = part ? pi * part : (pi ? len : 0u);
    if (*start >= len) return false;
    *plen = (part && part < len - *start) ? part : len - *start;
    return true;
}

// the state of a part's walk besides its tables; run: inside a predicted stretch, which goes on at distance dist while the error byte is 0
struct Walk { uint32_t cxt = 0, dist = 0; int order = 3; bool run = false; };

// Position i of a part (Lpx::EncodeBlock lpx.cpp:56-99, DecodeBlock lpx.cpp:101-144): takes the input byte and returns the byte to emit.
// back(dist) is the plain byte dist positions behind i: an input byte in encode, an output byte in decode.  Inside a stretch the stream
// holds prediction XOR byte.  r.pos <= i always holds (update stores pos - order); `d <= i` keeps the read inside the part all the same.
template <bool ENC, class Back> JPK_HD uint8_t step(Record (*table)[256], Walk &w, uint32_t i, uint8_t byte_in, Back back)
{
    if (!w.run) {
        const Record *r = &table[w.order - 1][w.cxt & 0xffu];
        const uint32_t d = i - r->pos;
        if (r->hits > (uint32_t)r->threshold && d < LPX_MAX_RECORD && d <= i) { w.run = true; w.dist = d; }
    }
    uint8_t o = byte_in;
    if (w.run) {
        o = (uint8_t)(back(w.dist) ^ byte_in);
        if ((ENC ? o : byte_in) != 0) w.run = false;               // the error byte
    }
    update(table, w.cxt, w.order, i);
    w.cxt = (w.cxt << 8) | (ENC ? byte_in : o);                    // the context is made of plain bytes
    return o;
}

// ring index of the byte dist <= LPX_MAX_RECORD positions behind the one at ring index wi
JPK_HD uint32_t ring_back(uint32_t wi, uint32_t dist) { return wi >= dist ? wi - dist : wi + LPX_RING - dist; }

// ---- filters and the stage chain (filters.cpp:245, 421-490) -------------------------------------------------------------------------
constexpr uint32_t FBS = 64u << 10;              // filter block: FBS bytes behind two header bytes (filter type, channel width)

// filter blocks of a stream of in_len bytes: all but the last are full
JPK_HD uint32_t filter_blocks(int64_t in_len) { return (uint32_t)((in_len + FBS + 1) / (FBS + 2)); }

// |S4| from |S1| in the writer's stage chain (prestage.cpp): a 00 00 header per filter piece of S1 and the second end token
JPK_HD int64_t s4_of_s1(int64_t s1) { return s1 + 2 + 2 * ((s1 + FBS - 1) / FBS); }

// LpcDecode: x = w + 2 p1 - p2 - err, w += (err - w) >> 6; dst may be src
JPK_HD void lpc_decode(const uint8_t *src, uint8_t *dst, uint32_t len)
{
    int32_t weight = 0;
    uint8_t p1 = 0, p2 = 0;
    for (uint32_t k = 0; k < len; k++) {
        const uint8_t err = src[k];
        const uint8_t cur = (uint8_t)(weight + (((int32_t)p1 - (int32_t)p2) + (int32_t)p1) - (int32_t)err);
        dst[k] = cur;
        weight += ((int32_t)err - weight) >> 6;
        p2 = p1;
        p1 = cur;
    }
}

// ---- filter choice of the writer ("Filters"): a rule of this library's own, not the reference's float heuristic ----------
// Per piece x[0..len) of S1 the candidates are raw, type 0 (Reorder + DeltaEncode, filters.cpp:21-30, 85-91: the delta runs over the whole
// reordered buffer, across channel borders) at widths 1..32 and type 2 (InlineDelta, filters.cpp:101-120) at widths 1..32; type 1 is never
// written.  A candidate costs the order-0 code length of its len output bytes in units of 1/4096 bit, in integer arithmetic, so that host
// and device choose alike; any choice decodes.
constexpr uint32_t FILTER_WIDTHS = 32;                     // MAX_CHANNEL_WIDTH
constexpr uint32_t FILTER_CANDS = 2 * FILTER_WIDTHS;       // candidate (type, width) has number (type / 2) * FILTER_WIDTHS + width - 1

// 4096 log2 v for 1 <= v <= 65536, off by at most 1, exact at powers of two.  The fraction comes bit by bit from sixteen squarings of the
// mantissa in Q31 (x < 2^32, so x * x fits 64 bits): floor(2^16 frac) up to the truncations, which weigh 2^-30 in all, rounded to 12 bits.
JPK_HD uint32_t lg12(uint32_t v)
{
    const uint32_t k = 31u - (uint32_t)__builtin_clz(v);
    uint64_t x = (uint64_t)v << (31u - k);
    uint32_t f = 0;
    for (int i = 0; i < 16; i++) {
        x = (x * x) >> 31;
        f <<= 1;
        if (x >> 32) { x >>= 1; f |= 1u; }
    }
    return (k << 12) + ((f + 8u) >> 4);
}

// what a byte value that occurs h times among len output bytes adds to the cost, lg_len = lg12(len): h (lg12(len) - lg12(h))
JPK_HD int64_t cost_term(uint32_t h, uint32_t lg_len) { return h ? (int64_t)h * ((int64_t)lg_len - (int64_t)lg12(h)) : 0; }

// the cost of len output bytes with byte histogram h
JPK_HD int64_t filter_cost(const uint32_t *h, uint32_t len)
{
    const uint32_t lg_len = lg12(len);
    int64_t c = 0;
    for (int s = 0; s < 256; s++) c += cost_term(h[s], lg_len);
    return c;
}

// The choice: raw keeps a margin of 1/16 of its cost; type 0 at widths 1..32, then type 2 at widths 1..32, a candidate wins only strictly
// below the best so far.  cost(type, width) is asked once per candidate, in that order.  width 0: the piece stays raw (00 00).
struct FilterChoice { uint32_t type, width; };
template <class Cost> JPK_HD FilterChoice filter_choose(int64_t raw_cost, Cost cost)
{
    FilterChoice ch = {0u, 0u};
    int64_t best = raw_cost - (raw_cost >> 4);
    for (uint32_t type = 0; type <= 2u; type += 2u)
        for (uint32_t w = 1; w <= FILTER_WIDTHS; w++) {
            const int64_t c = cost(type, w);
            if (c < best) { best = c; ch.type = type; ch.width = w; }
        }
    return ch;
}

// Reorder: the piece index of position pos of its output.  Channel c holds x[c], x[c + width], ...: q = len / width elements, one more when
// c < r = len mod width, so it starts at c q + min(c, r) -- the formula k_pre_filters reads by, inverted.
JPK_HD uint32_t reorder_src(uint32_t len, uint32_t width, uint32_t pos)
{
    const uint32_t q = len / width, r = len % width, big = r * (q + 1u);
    if (pos < big) return pos / (q + 1u) + (pos % (q + 1u)) * width;
    const uint32_t p = pos - big;                                      // q >= 1 here: q == 0 means big == len
    return r + p / q + (p % q) * width;
}

// byte pos of the candidate's output; x(i) = byte i of the piece.  width 0: raw.
template <class Get> JPK_HD uint8_t filter_byte(Get x, uint32_t len, uint32_t type, uint32_t width, uint32_t pos)
{
    if (width == 0u) return (uint8_t)x(pos);
    if (type == 2u) return pos < len % width + width ? (uint8_t)x(pos) : (uint8_t)(x(pos) - x(pos - width));   // raw head, first group against zeros
    const uint32_t cur = x(reorder_src(len, width, pos));
    return pos ? (uint8_t)(cur - x(reorder_src(len, width, pos - 1u))) : (uint8_t)cur;
}

// Both types at one width share the differences D = { x[i] - x[i - width] : width <= i < len }.  What a candidate's output differs from D
// by, as add(byte, +1 or -1) calls, fewer than 3 width of them:
//   type 0  every i >= width is an element k >= 1 of channel i mod width, so D is all of it but the channel starts: x[0] against zero, and
//           x[c] against the last element of channel c - 1
//   type 2  the first min(len, len mod width + width) bytes go out as they are; those of them at i >= width leave D
template <class Get, class Add> JPK_HD void filter_fixups(Get x, uint32_t len, uint32_t type, uint32_t width, Add add)
{
    if (type == 2u) {
        const uint32_t head = len % width + width < len ? len % width + width : len;
        for (uint32_t i = 0; i < head; i++) {
            add((uint8_t)x(i), 1);
            if (i >= width) add((uint8_t)(x(i) - x(i - width)), -1);
        }
        return;
    }
    if (len) add((uint8_t)x(0u), 1);
    for (uint32_t c = 1; c < width && c < len; c++) add((uint8_t)(x(c) - x(c - 1u + (len - c) / width * width)), 1);
}

}  // namespace pre
