// dedupe.hpp -- the rule of jpk_lz77_dedupe ("Dedupe"), shared by its host form (prestage.cpp) and the k_dd_* kernels
// (prestage_dev.hip) so that both compute the same bytes: the window fingerprint, the slot of the anchor table, the offset a position is
// a candidate for, the extension of a run from its head, the greedy selection and the token header.  Every function is a pure function of
// the block and of the finished anchor table (the smallest aligned position per slot), so the result depends on no launch order.
#pragma once
#include <stdint.h>

#include "prestage_rules.hpp"

namespace dd {

constexpr uint32_t W = 64;                  // window: anchors are the windows at multiples of W
constexpr uint32_t MIN_MATCH = 256;         // DUPE_MATCH, lz77.cpp:544
constexpr uint32_t TILE = 1024;             // positions per tile of the candidate pass
constexpr uint32_t TILE_HEADS = 32;         // heads kept per tile, the first ones in position order
constexpr uint32_t GAP = 8;                 // windows in a row that are no candidate for the run's offset and that it crosses by byte equality
constexpr uint32_t RUN_W = 64;              // windows a run looks at going forward: four tiles, each of which starts a piece of its own
constexpr uint32_t BACK_W = 8;              // windows a run grows backward from its head by byte equality
constexpr uint32_t BACK = 63, FWD = 63;     // bytes a run then grows at its two ends by byte equality
constexpr uint32_t MUL = 0x01000193u;       // polynomial base (odd)
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr int MIN_BITS = 10;

struct Run { uint32_t s, e, d; };           // [s, e) equals [s - d, e - d)
// one token as the emit pass sees it: `hlen` header bytes at out_off, then `lit` literals from in[lit_src ..]
struct Tok { uint32_t out_off, lit_src, lit, hlen; uint8_t hdr[16]; };

// anchors of an n-byte block and the bits of its slot table: a power of two of at least four slots per anchor
JPK_HD uint32_t anchors(uint32_t n) { return n / W; }
JPK_HD int table_bits(uint32_t n)
{
    int b = MIN_BITS;
    while (((uint64_t)1 << b) < 4ull * anchors(n)) b++;
    return b;
}
JPK_HD uint32_t tiles(uint32_t n) { return (n + TILE - 1) / TILE; }
JPK_HD uint32_t max_toks(uint32_t n) { return n / MIN_MATCH + 2; }

JPK_HD uint32_t slot(uint32_t fp, int bits) { return (fp * 0x9E3779B1u) >> (32 - bits); }

// fp(p) = sum (in[p + i] + 1) MUL^(63 - i) mod 2^32: what six doubling steps h2k(p) = hk(p) MUL^k + hk(p + k) give from h1(p) = in[p] + 1
JPK_HD uint32_t fp_at(const uint8_t *in, uint32_t p)
{
    uint32_t h = 0;
    for (uint32_t i = 0; i < W; i++) h = h * MUL + in[p + i] + 1u;
    return h;
}

JPK_HD bool equal_w(const uint8_t *a, const uint8_t *b)
{
    for (uint32_t i = 0; i < W; i++) if (a[i] != b[i]) return false;
    return true;
}

// the offset position p is a candidate for, from its fingerprint: the anchor q in its slot lies a whole window in front and holds the
// same 64 bytes (d = p - q >= 64); 0: none
JPK_HD uint32_t cand_fp(const uint8_t *in, uint32_t /* n */, const uint32_t *table, int bits, uint32_t p, uint32_t fp)
{
    const uint32_t q = table[slot(fp, bits)];
    if (q == EMPTY || q + W > p) return 0u;
    return equal_w(in + p, in + q) ? p - q : 0u;
}
JPK_HD uint32_t cand(const uint8_t *in, uint32_t n, const uint32_t *table, int bits, uint32_t p)
{
    if (p < W || (uint64_t)p + W > n) return 0u;
    return cand_fp(in, n, table, bits, p, fp_at(in, p));
}

// p with d = cand(p) != 0 and cand(p + 64) == d (two windows in a row at one offset) is a HEAD when cand(p - 64) != d -- the first of them --
// or when p lies in the first 64 positions of its tile: a long copy is reported in pieces of at most one tile, each by a head of its own.
JPK_HD bool is_head(uint32_t p, uint32_t dprev, uint32_t d, uint32_t dnext) { return d != 0u && dnext == d && (dprev != d || p % TILE < W); }

// The run of a head: forward window by window while the window is a candidate for d, or is none but equal byte for byte at d -- its anchor
// was lost to a collision in the slot table, or its slot names an earlier copy of the same 64 bytes, which data that repeats itself at short
// range (text) does to several windows in a hundred.  At most GAP such windows follow each other, so a run ends GAP windows behind the last
// candidate for d: that bounds the work on periodic data, where every window equals its predecessor at every period.  It also ends in front
// of a window that differs or that is a head for d itself (that head reports the rest, the selection joins the two), and behind RUN_W
// windows whatever it meets (it passes a tile's start only where that window is no head, so this is rare).  Then FWD bytes forward
// by byte equality; backward from the head at most BACK_W windows by byte equality -- a head needs two candidates in a row, so behind a
// changed byte the first one can lie some windows into the copy -- and then BACK bytes.
JPK_HD Run extend(const uint8_t *in, uint32_t n, const uint32_t *table, int bits, uint32_t p, uint32_t d)
{
    uint32_t e = p + W, cur = p + W, gap = 0, dprev = d;
    uint32_t dcur = cand(in, n, table, bits, cur);
    for (uint32_t w = 1; w < RUN_W && (uint64_t)cur + W <= n; w++) {
        const uint32_t dnext = cand(in, n, table, bits, cur + W);
        if (dcur == d) {
            if (is_head(cur, dprev, d, dnext)) break;
            gap = 0;
        } else {
            if (gap == GAP || !equal_w(in + cur, in + cur - d)) break;
            gap++;
        }
        e = cur + W;
        dprev = dcur;
        dcur = dnext;
        cur += W;
    }
    for (uint32_t k = 0; k < FWD && e < n && in[e] == in[e - d]; k++) e++;
    uint32_t s = p;
    for (uint32_t k = 0; k < BACK_W && s >= d + W && equal_w(in + s - W, in + s - W - d); k++) s -= W;
    for (uint32_t k = 0; k < BACK && s > d && in[s - 1] == in[s - 1 - d]; k++) s--;
    Run r;
    r.s = s; r.e = e; r.d = d;
    return r;
}

// Lz77::WriteToken (lz77.cpp:53-70): token byte, offset, the extension of a saturated match class, of a saturated literal class; <= 16 bytes
JPK_HD uint32_t token_write(uint32_t match, uint32_t lit, uint32_t off, uint8_t *b)
{
    match -= 4u;                                                       // MIN_MATCH, lz77.hpp:33
    uint32_t pos = 0;
    b[pos++] = (uint8_t)(((match < 31u ? match : 31u) << 3) | (lit < 7u ? lit : 7u));
    pos += pre::leb_write(off, b + pos);
    if (match >= 31u) pos += pre::leb_write(match - 31u, b + pos);
    if (lit >= 7u) pos += pre::leb_write(lit - 7u, b + pos);
    return pos;
}

// The greedy selection of one block, in the order of the run list (tile by tile, slot by slot).  One run is pending: a run that starts
// inside or at the end of it at the same offset makes it longer (the pieces of one copy); any other run settles it -- it becomes a token when
// it is at least 256 bytes long and moves the cursor to its end, else it is dropped -- and is itself cut to the cursor and made pending.
// finish() adds the end token 04 80 in front of the rest.  toks[] holds max_toks(n) records; store = false only counts.
struct Select {
    Tok *toks;
    bool store;
    uint32_t ntok = 0, out = 0, cursor = 0;          // tokens so far, bytes of S1' they and their literals take, end of the last token's match
    Run pend;                                        // e == 0: none
    JPK_HD Select(Tok *t, bool st) : toks(t), store(st) { pend.s = 0; pend.e = 0; pend.d = 0; }
    JPK_HD void flush()
    {
        if (pend.e != 0u && pend.e - pend.s >= MIN_MATCH) {
            Tok t;
            t.out_off = out; t.lit_src = cursor; t.lit = pend.s - cursor;
            for (int i = 0; i < 16; i++) t.hdr[i] = 0;
            t.hlen = token_write(pend.e - pend.s, t.lit, pend.d, t.hdr);
            if (store) toks[ntok] = t;
            ntok++;
            out += t.hlen + t.lit;
            cursor = pend.e;
        }
        pend.e = 0;
    }
    JPK_HD void add(const Run &r)
    {
        if (pend.e != 0u && r.d == pend.d && r.s <= pend.e) { if (r.e > pend.e) pend.e = r.e; return; }
        flush();
        const uint32_t s = r.s > cursor ? r.s : cursor;
        if (r.e > s) { pend.s = s; pend.e = r.e; pend.d = r.d; }
    }
    // returns |S1'|
    JPK_HD uint32_t finish(uint32_t n)
    {
        flush();
        Tok t;
        t.out_off = out; t.lit_src = cursor; t.lit = n - cursor; t.hlen = 2;
        for (int i = 0; i < 16; i++) t.hdr[i] = 0;
        t.hdr[0] = pre::END_TOKEN[0]; t.hdr[1] = pre::END_TOKEN[1];
        if (store) toks[ntok] = t;
        ntok++;
        return out + 2u + t.lit;
    }
};

}  // namespace dd
