// prestage.cpp -- host-side decoders of the three stages the stock CLI runs in front of the BWT
// (Jampack::Decomp, jampack.cpp:47-60: Lz77::Decompress, Lpx::Decode, Filters::Decode, Lz77::Decompress), so that
// frames written by an unmodified `jampack c` decode end to end: rANS decode + inverse BWT on the GPU, these on the
// host where SURVEY.md section 8f (row 4) puts them -- byte-serial state machines with no data parallelism.
// The encoder side is the part of the reference's encoders that a VALID stream needs and no more (writing): the stored forms
// of LZ77 and Filters, and Lpx::Encode, which has no stored form and is deterministic integer code; and, as options of the writer, a dedupe of
// long repeats in the token format of the first LZ77 stage (jpk_lz77_dedupe; the rule is dedupe.hpp's, not the reference's hash walk) and a
// choice among the delta filters per 64 KiB piece (jpk_filters_encode; an integer order-0 cost of this library's own, prestage_rules.hpp).
// The match finders and the reference's filter selection with their float heuristics stay with the reference.
//
// Unlike the reference (which trusts its input outside NDEBUG builds, lz77.cpp:697-701) every read and write is
// bounds checked and a bad stream gives JPK_E_CORRUPT / JPK_E_CAPACITY.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/jampack_abi.h"
#include "dedupe.hpp"
#include "lz_expand.hpp"

// Lz77::Decompress (lz77.cpp:678-714); the token is pre::parse_token.  Offset 0 ends the LZ code: the rest of the input is copied through.
extern "C" int jpk_lz77_decompress(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    if (!out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !in) || (out_cap > 0 && !out)) return JPK_E_ARG;
    int64_t pos = 0, op = 0;
    while (pos < in_len) {
        pre::Token t;
        if (!pre::parse_token([&](int j) { return (uint32_t)in[pos + j]; }, in_len - pos, &t)) return JPK_E_CORRUPT;
        const int32_t off = t.off;
        const int64_t len = t.len, lit = t.lit;
        pos += t.used;
        if (off == 0) {                                                // end marker: raw remainder
            const int64_t rest = in_len - pos;
            if (op + rest > out_cap) return JPK_E_CAPACITY;
            memcpy(out + op, in + pos, (size_t)rest);
            op += rest;
            break;
        }
        if (off < 0 || lit > in_len - pos) return JPK_E_CORRUPT;
        if (lit + len > (int64_t)out_cap - op) return JPK_E_CAPACITY;
        memcpy(out + op, in + pos, (size_t)lit);
        op += lit;
        pos += lit;
        if (off > op) return JPK_E_CORRUPT;
        const uint8_t *src = out + op - off;                           // may overlap the destination: byte order matters
        for (int64_t k = 0; k < len; k++) out[op + k] = src[k];
        op += len;
    }
    *out_len = (int32_t)op;
    return JPK_OK;
}

// The raw size of a stream without its bytes: the status jpk_lz77_decompress gives it at this out_cap and, when that is JPK_OK, its
// *out_len (0 otherwise).  The rule is lzx::step(lzx::Size) of lz_expand.hpp, which k_lz77_sizes compiles too.  No device call.
extern "C" int jpk_lz77_size(const uint8_t *in, int32_t in_len, int32_t out_cap, int32_t *out_len)
{
    if (!out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !in)) return JPK_E_ARG;
    lzx::Size s;
    while (lzx::more(s, in_len)) {
        pre::Token t;
        const uint8_t *at = in + s.pos;
        const bool parsed = pre::parse_token([at](int j) { return (uint32_t)at[j]; }, in_len - s.pos, &t);
        lzx::step(s, parsed, t, in_len, out_cap);
    }
    *out_len = lzx::out_len(s);
    return s.status;
}

namespace {

// Lpx::Encode (lpx.cpp:56-99, 148-158) / Lpx::Decode (lpx.cpp:101-169): every part (pre::part_of) with a fresh model, pre::step byte by
// byte.  The plain bytes behind position i are input bytes in encode and output bytes in decode.
template <bool ENC> int lpx_code(const uint8_t *in, int32_t len, uint8_t *out)
{
    if (len < 0 || (len > 0 && (!in || !out))) return JPK_E_ARG;
    pre::Record table[3][256];
    uint32_t start = 0, plen = 0;
    for (uint32_t pi = 0; pre::part_of((uint32_t)len, pi, &start, &plen); pi++) {
        const uint8_t *src = in + start, *plain = ENC ? src : out + start;
        uint8_t *dst = out + start;
        for (auto &t : table)
            for (auto &r : t) r = pre::fresh_record();
        pre::Walk w;
        for (uint32_t i = 0; i < plen; i++) dst[i] = pre::step<ENC>(table, w, i, src[i], [&](uint32_t d) { return plain[i - d]; });
    }
    return JPK_OK;
}

}  // namespace

extern "C" int jpk_lpx_decode(const uint8_t *in, int32_t len, uint8_t *out) { return lpx_code<false>(in, len, out); }
extern "C" int jpk_lpx_encode(const uint8_t *in, int32_t len, uint8_t *out) { return lpx_code<true>(in, len, out); }

// Filters::Decode (filters.cpp:442-490): per 64 KiB block two header bytes (filter type, channel width), width 0 =
// raw.  Types: 0 delta and 1 adaptive linear prediction on de-interleaved channels, 2 in-place delta per channel.
extern "C" int jpk_filters_decode(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    if (!out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !in) || (out_cap > 0 && !out)) return JPK_E_ARG;
    constexpr int64_t FBS = pre::FBS;
    std::vector<uint8_t> dbuf((size_t)FBS);
    int64_t i = 0, op = 0;
    while (i < in_len) {
        if (i + 2 > in_len) return JPK_E_CORRUPT;
        const int type = in[i], width = in[i + 1];
        i += 2;
        if (type >= 3 || width > 32) return JPK_E_CORRUPT;            // "unsupported configuration", filters.cpp:455
        const int64_t len = (i + FBS < in_len) ? FBS : in_len - i;
        if (op + len > out_cap) return JPK_E_CAPACITY;
        const uint8_t *src = in + i;
        uint8_t *dst = out + op;
        if (width == 0) {
            memcpy(dst, src, (size_t)len);
        } else if (type == 2) {                                         // InlineUndelta, filters.cpp: running sum per channel in place
            uint8_t prev[32] = {0};
            int64_t k = len % width;
            memcpy(dst, src, (size_t)k);
            for (; k < len; k += width)
                for (int j = 0; j < width; j++) { dst[k + j] = (uint8_t)(src[k + j] + prev[j]); prev[j] = dst[k + j]; }
        } else {
            if (type == 0) {                                            // DeltaDecode: running sum over the whole block
                uint8_t prev = 0;
                for (int64_t k = 0; k < len; k++) { prev = (uint8_t)(src[k] + prev); dbuf[(size_t)k] = prev; }
            } else {
                pre::lpc_decode(src, dbuf.data(), (uint32_t)len);
            }
            int64_t p = 0;                                              // Unreorder: channel c holds bytes c, c + width, ...
            for (int c = 0; c < width; c++)
                for (int64_t j = c; j < len; j += width) dst[j] = dbuf[(size_t)p++];
        }
        op += len;
        i += len;
    }
    *out_len = (int32_t)op;
    return JPK_OK;
}

// ---- Filters::Encode with this library's own choice ("Filters"; the rule is prestage_rules.hpp) ----------------------------
namespace {

// The choice for the piece x[0..len): the differences at distance w are counted once per width, and the histograms of both types' outputs
// come from them by pre::filter_fixups -- the shape k_enc_filters has; jpk_filters_cost counts a candidate's output bytes themselves.
pre::FilterChoice filters_choose(const uint8_t *x, uint32_t len)
{
    uint32_t raw[256] = {0}, d[256], h[256];
    int64_t cost[pre::FILTER_CANDS];
    for (uint32_t i = 0; i < len; i++) raw[x[i]]++;
    const auto get = [x](uint32_t i) { return (uint32_t)x[i]; };
    for (uint32_t w = 1; w <= pre::FILTER_WIDTHS; w++) {
        memset(d, 0, sizeof d);
        for (uint32_t i = w; i < len; i++) d[(uint8_t)(x[i] - x[i - w])]++;
        for (uint32_t type = 0; type <= 2u; type += 2u) {
            memcpy(h, d, sizeof h);
            pre::filter_fixups(get, len, type, w, [&h](uint8_t b, int s) { h[b] += (uint32_t)s; });
            cost[(type / 2u) * pre::FILTER_WIDTHS + w - 1u] = pre::filter_cost(h, len);
        }
    }
    return pre::filter_choose(pre::filter_cost(raw, len), [&cost](uint32_t type, uint32_t w) { return cost[(type / 2u) * pre::FILTER_WIDTHS + w - 1u]; });
}

// one piece of S2: two header bytes and len bytes into dst, which does not overlap x
void filters_encode_piece(const uint8_t *x, uint32_t len, uint8_t *dst)
{
    const pre::FilterChoice ch = filters_choose(x, len);
    dst[0] = (uint8_t)ch.type; dst[1] = (uint8_t)ch.width;
    if (ch.width == 0) { memcpy(dst + 2, x, len); return; }
    const auto get = [x](uint32_t i) { return (uint32_t)x[i]; };
    for (uint32_t pos = 0; pos < len; pos++) dst[2 + pos] = pre::filter_byte(get, len, ch.type, ch.width, pos);
}

}  // namespace

extern "C" int jpk_filters_encode(const uint8_t *in, int32_t in_len, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    if (!out_len || in_len < 0 || out_cap < 0 || (in_len > 0 && !in) || (out_cap > 0 && !out)) return JPK_E_ARG;
    constexpr int64_t FBS = pre::FBS;
    const int64_t total = (int64_t)in_len + 2 * (((int64_t)in_len + FBS - 1) / FBS);
    if (total > 0x7fffffff) return JPK_E_ARG;
    if (total > out_cap) return JPK_E_CAPACITY;
    int64_t op = 0;
    for (int64_t i = 0; i < in_len;) {
        const int64_t len = (i + FBS < in_len) ? FBS : in_len - i;
        filters_encode_piece(in + i, (uint32_t)len, out + op);
        op += 2 + len;
        i += len;
    }
    *out_len = (int32_t)op;
    return JPK_OK;
}

extern "C" int jpk_filters_cost(const uint8_t *piece, int32_t len, int32_t type, int32_t width, int64_t *cost)
{
    if (!piece || !cost || len < 1 || len > (int32_t)pre::FBS || width < 0 || width > (int32_t)pre::FILTER_WIDTHS) return JPK_E_ARG;
    if (width > 0 && type != 0 && type != 2) return JPK_E_ARG;
    uint32_t h[256] = {0};
    const auto get = [piece](uint32_t i) { return (uint32_t)piece[i]; };
    for (uint32_t pos = 0; pos < (uint32_t)len; pos++) h[pre::filter_byte(get, (uint32_t)len, (uint32_t)type, (uint32_t)width, pos)]++;
    *cost = pre::filter_cost(h, (uint32_t)len);
    return JPK_OK;
}

// ---- the stage chain of a frame the stock CLI decodes, written without match finding (writing) -----------------------------
//   S1 = end token | R          the token is what the reference's own flush writes, WriteToken(MIN_MATCH, MIN_MATCH, 0) (lz77.cpp:620,
//                               53-70): token byte (4 - 4) << 3 | 4 = 0x04, then EncodeLeb128(0) = 0x80 (utils.cpp:28-31).  Offset 0 makes
//                               Lz77::Decompress copy the rest through (lz77.cpp:705-711).
//   S2 = every 64 KiB piece of S1 behind a 00 00 header (type 0, width 0 = raw, filters.cpp:421-426, 480-483); the split is the
//                               encoder's own (filters.cpp:245): all pieces but the last are full, an exactly full last piece stays one
//                               (JPK_CLI_FILTERS: behind `type, width` and transformed where the choice above finds a filter; same length)
//   S3 = Lpx::Encode(S2)        same length
//   S4 = end token | S3
// |S2| = n + 2 + 2 P with P = ceil((n + 2) / 65536) pieces (n + 2 >= 2: at least one), |S4| = n + 4 + 2 P.
// The two bounds a frame must keep, for n <= BlockSize = B, B >= JPK_MIN_BLOCKSIZE = 2^20:
//   P <= (B + 2 + 65535) / 65536 <= B / 65536 + 1, so |S4| + 480 (the BWT trailer) <= B + B / 32768 + 486;
//   the reference's stage buffers hold (int)(B * 1.05) >= B + B / 20 - 1 bytes (jampack.cpp:157), and B / 20 - B / 32768 >= 52396 at
//   B = 2^20 and grows with B, which is above 487: the frame fits them, and with them this library's own 1.05 B + 4096 on the
//   entropy-decoded size.  At B = JPK_MAX_BLOCKSIZE |S4| = 1048576000 + 4 + 2 * 16001 stays below 2^31 and below JPK_FWD_BWT_LIMIT.
extern "C" int64_t jpk_cli_stages_bound(int64_t n)
{
    if (n < 0) return JPK_E_ARG;
    return pre::s4_of_s1(n + 2);
}

// S2 of S1 = head | body into buf[0..s2): the filter pieces, stored or chosen
static int cli_s2_from(const uint8_t *head, int64_t nhead, const uint8_t *body, int64_t nbody, uint8_t *buf, int64_t s2, bool filters)
{
    constexpr int64_t FBS = pre::FBS;
    const int64_t s1 = nhead + nbody;
    std::vector<uint8_t> piece;
    try { if (filters) piece.resize((size_t)FBS); } catch (...) { return JPK_E_ALLOC; }
    int64_t op = 0;
    for (int64_t i = 0; i < s1;) {                                     // byte i of S1: head[i], then body[i - nhead]
        const int64_t len = (i + FBS < s1) ? FBS : s1 - i;
        if (op + 2 + len > s2) return JPK_E_CAPACITY;                  // cannot happen: s2 counts exactly these bytes
        buf[op] = 0; buf[op + 1] = 0;
        op += 2;
        int64_t k = 0;
        for (; i + k < nhead && k < len; k++) buf[op + k] = head[i + k];
        if (len > k) memcpy(buf + op + k, body + (i + k - nhead), (size_t)(len - k));
        if (filters) {
            memcpy(piece.data(), buf + op, (size_t)len);
            filters_encode_piece(piece.data(), (uint32_t)len, buf + op - 2);
        }
        op += len;
        i += len;
    }
    return JPK_OK;
}

// S4 of S1 = head | body: the filter pieces, Lpx::Encode, the second end token
static int cli_stages_from(const uint8_t *head, int64_t nhead, const uint8_t *body, int64_t nbody, uint8_t *out, int32_t out_cap, int32_t *out_len,
                           bool filters)
{
    const int64_t s1 = nhead + nbody, total = pre::s4_of_s1(s1), s2 = total - 2;
    if (total > 0x7fffffff) return JPK_E_ARG;
    if (total > out_cap) return JPK_E_CAPACITY;
    std::vector<uint8_t> buf;
    try { buf.resize((size_t)s2); } catch (...) { return JPK_E_ALLOC; }
    int rc = cli_s2_from(head, nhead, body, nbody, buf.data(), s2, filters);
    if (rc != JPK_OK) return rc;
    out[0] = pre::END_TOKEN[0]; out[1] = pre::END_TOKEN[1];
    rc = jpk_lpx_encode(buf.data(), (int32_t)s2, out + 2);
    if (rc != JPK_OK) return rc;
    *out_len = (int32_t)total;
    return JPK_OK;
}

// ---- the dedupe: long repeats inside the block as tokens of the first LZ77 stage ("Dedupe"; the rule is dedupe.hpp) ----------
//   1 anchors     every aligned window q = 0, 64, ... goes into its slot of the table; a slot keeps the smallest q
//   2 candidates  every position is looked up by its fingerprint (rolled here, doubled in LDS on the device); heads are kept per tile of
//                 1024 positions, the first dd::TILE_HEADS of a tile
//   3 runs        dd::extend from every head
//   4 selection   dd::Select over the runs in position order
//   5 emit        token headers and literal runs, then 04 80 and the rest
// Work: steps 1, 2 and 5 touch every byte a constant number of times; a run of step 3 looks at no more than TILE / W + GAP windows and there
// are at most n / 32 heads (DESIGN has the arithmetic).
extern "C" int jpk_lz77_dedupe(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    if (!out_len || n < 0 || out_cap < 0 || (n > 0 && !in) || (out_cap > 0 && !out)) return JPK_E_ARG;
    *out_len = 0;
    const uint32_t N = (uint32_t)n;
    const int bits = dd::table_bits(N);
    std::vector<uint32_t> table;
    std::vector<dd::Tok> toks;
    try { table.assign((size_t)1 << bits, dd::EMPTY); toks.resize(dd::max_toks(N)); } catch (...) { return JPK_E_ALLOC; }
    for (uint32_t q = 0; (uint64_t)q + dd::W <= N; q += dd::W) {
        uint32_t &t = table[dd::slot(dd::fp_at(in, q), bits)];
        if (q < t) t = q;
    }
    dd::Select sel(toks.data(), true);
    if (N >= 2 * dd::W) {
        uint32_t top = 1;                                              // MUL^63: what the byte that leaves the window carries
        for (uint32_t i = 0; i + 1 < dd::W; i++) top *= dd::MUL;
        uint32_t ring[256] = {0};                                      // cand() of the last positions (0 in front of position 64)
        uint32_t fp = dd::fp_at(in, dd::W), tile = 0, kept = 0;
        for (uint32_t x = dd::W;; x++) {                               // x runs one window ahead of the position p it decides
            const uint32_t dx = dd::cand_fp(in, N, table.data(), bits, x, fp);
            ring[x & 255u] = dx;
            const uint32_t p = x - dd::W, d = ring[p & 255u];
            if (p >= dd::W && dd::is_head(p, ring[(p - dd::W) & 255u], d, dx)) {
                if (p / dd::TILE != tile) { tile = p / dd::TILE; kept = 0; }
                if (kept < dd::TILE_HEADS) { kept++; sel.add(dd::extend(in, N, table.data(), bits, p, d)); }
            }
            if ((uint64_t)x + dd::W >= N) break;                       // x was the last whole window
            fp = (fp - (in[x] + 1u) * top) * dd::MUL + in[x + dd::W] + 1u;
        }
    }
    const uint32_t total = sel.finish(N);
    if ((int64_t)total > out_cap) return JPK_E_CAPACITY;
    for (uint32_t i = 0; i < sel.ntok; i++) {
        const dd::Tok &t = toks[i];
        memcpy(out + t.out_off, t.hdr, t.hlen);
        if (t.lit) memcpy(out + t.out_off + t.hlen, in + t.lit_src, t.lit);
    }
    *out_len = (int32_t)total;
    return JPK_OK;
}

extern "C" int jpk_cli_stages_encode_ex(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags)
{
    if (!out_len || n < 0 || out_cap < 0 || (n > 0 && !in) || (out_cap > 0 && !out) || !JPK_CLI_FLAGS_OK(flags)) return JPK_E_ARG;
    if (jpk_cli_stages_bound(n) > 0x7fffffff) return JPK_E_ARG;
    const bool filters = (flags & JPK_CLI_FILTERS) != 0;
    if (!(flags & JPK_CLI_DEDUPE)) return cli_stages_from(pre::END_TOKEN, 2, in, n, out, out_cap, out_len, filters);
    std::vector<uint8_t> s1;
    try { s1.resize((size_t)n + 2); } catch (...) { return JPK_E_ALLOC; }
    int32_t m = 0;
    const int rc = jpk_lz77_dedupe(in, n, s1.data(), n + 2, &m);       // |S1'| <= n + 2: every token pays for itself
    if (rc != JPK_OK) return rc;
    return cli_stages_from(nullptr, 0, s1.data(), m, out, out_cap, out_len, filters);
}

// The same chain stopped at S2, which is what a staged frame hands to the BWT ("Staged frames"); |S2| = jpk_cli_stages_bound - 2
// at most.  Declared in common.hpp for abi_host.hip.
int jpk_staged_s2_host(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags);
int jpk_staged_s2_host(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len, uint32_t flags)
{
    if (!out_len || n < 0 || out_cap < 0 || (n > 0 && !in) || (out_cap > 0 && !out) || !JPK_CLI_FLAGS_OK(flags)) return JPK_E_ARG;
    if (jpk_cli_stages_bound(n) > 0x7fffffff) return JPK_E_ARG;
    const bool filters = (flags & JPK_CLI_FILTERS) != 0;
    std::vector<uint8_t> s1;
    int32_t m = 0;
    if (flags & JPK_CLI_DEDUPE) {
        try { s1.resize((size_t)n + 2); } catch (...) { return JPK_E_ALLOC; }
        const int rc = jpk_lz77_dedupe(in, n, s1.data(), n + 2, &m);
        if (rc != JPK_OK) return rc;
    }
    const int64_t s2 = pre::s4_of_s1((flags & JPK_CLI_DEDUPE) ? m : (int64_t)n + 2) - 2;
    if (s2 > out_cap) return JPK_E_CAPACITY;
    const int rc = (flags & JPK_CLI_DEDUPE) ? cli_s2_from(nullptr, 0, s1.data(), m, out, s2, filters) : cli_s2_from(pre::END_TOKEN, 2, in, n, out, s2, filters);
    if (rc != JPK_OK) return rc;
    *out_len = (int32_t)s2;
    return JPK_OK;
}

extern "C" int jpk_cli_stages_encode(const uint8_t *in, int32_t n, uint8_t *out, int32_t out_cap, int32_t *out_len)
{
    return jpk_cli_stages_encode_ex(in, n, out, out_cap, out_len, 0u);
}

// Checksum::IntegrityCheck on the host (checksum.cpp:12-36), for buffers that are already there
extern "C" uint32_t jpk_checksum_host(const uint8_t *p, int32_t size)
{
    const uint32_t prime = 0x9E3779B1u;
    uint32_t S[4] = {3u, 0u, 0u, 0u};
    uint32_t j = 0;
    const uint32_t n = size > 0 ? (uint32_t)size : 0u;
    while ((uint64_t)j + 16 < n) {
        for (int k = 0; k < 4; k++) {
            const uint8_t *q = p + j + 4 * k;
            const uint32_t w = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
            S[k] ^= (w + (1u << (S[k] & 7))) * prime;
        }
        j += 16;
    }
    for (; j < n; j++) S[0] ^= ((uint32_t)p[j] + (1u << (S[0] & 7))) * prime;
    return S[0] ^ S[1] ^ S[2] ^ S[3];
}
