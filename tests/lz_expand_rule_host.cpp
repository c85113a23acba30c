// The rule of the parallel LZ77 expander (jampack_amd/csrc/lz_expand.hpp) on the CPU: the host form of plan and chase -- the same
// lzx::step, lzx::find and lzx::source the kernels compile -- against jpk_lz77_decompress (prestage.cpp) on the crafted streams of
// tests/lz_expand_cases.py (argv[1]) and on 2000 random token streams of at most 4 KiB of output.  A block the rule decodes must have the
// serial decoder's status JPK_OK, its length and its bytes; a block the rule hands over must be one the serial decoder refuses, one
// with more records than lzx::seg_cap, or one with a byte more than lzx::MAX_CHASE matches from its literal -- all three recomputed here
// without the rule.  Built with -fsanitize=address,undefined by tests/test_lz_expand_rule_host.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../include/jampack_abi.h"
#include "../jampack_amd/csrc/lz_expand.hpp"

namespace {

int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL " __VA_ARGS__); printf("\n"); } } while (0)

// the rule: true = decoded from the records (out, *out_len), false = handed to the serial decoder
bool rule_expand(const std::vector<uint8_t> &in, std::vector<uint8_t> &out, int32_t out_cap, int32_t *out_len)
{
    const int64_t in_len = (int64_t)in.size();
    const uint32_t cap = lzx::seg_cap(in_len);
    std::vector<lzx::Seg> segs(cap);                                    // exactly the cap: a record too many is a heap overflow
    lzx::Plan p;
    while (lzx::more(p, in_len)) {
        pre::Token t;
        const uint8_t *at = in.data() + p.pos;
        const bool parsed = pre::parse_token([at](int j) { return (uint32_t)at[j]; }, in_len - p.pos, &t);
        lzx::step(p, parsed, t, in_len, (int64_t)out_cap, cap, [&segs](uint32_t i, const lzx::Seg &s) { segs.at(i) = s; });
    }
    if (p.serial) return false;
    for (uint32_t i = 0; i < p.nseg; i++) {
        CHECK(segs[i].len > 0 && segs[i].out == (i ? segs[i - 1].out + segs[i - 1].len : 0u), "records out of order at %u", i);
        CHECK(!segs[i].match || (i > 0 && segs[i].src >= 1 && segs[i].src <= segs[i].out), "match record %u", i);
        CHECK(segs[i].match || (uint64_t)segs[i].src + segs[i].len <= (uint64_t)in_len, "literal record %u", i);
    }
    for (int64_t pos = 0; pos < p.op; pos++) {
        const uint32_t idx = lzx::find(segs.data(), p.nseg, (uint32_t)pos);
        uint32_t io = 0;
        if (!lzx::source(segs.data(), idx, segs[idx], (uint32_t)pos, &io)) return false;
        out.at((size_t)pos) = in.at(io);
    }
    *out_len = (int32_t)p.op;
    return true;
}

// without the rule: the records a valid stream needs and the deepest byte, from a walk of its own over the tokens
void stream_shape(const std::vector<uint8_t> &in, uint32_t *nrec, uint32_t *depth)
{
    std::vector<uint32_t> d;
    int64_t pos = 0;
    *nrec = 0; *depth = 0;
    while (pos < (int64_t)in.size()) {
        pre::Token t;
        const uint8_t *at = in.data() + pos;
        if (!pre::parse_token([at](int j) { return (uint32_t)at[j]; }, (int64_t)in.size() - pos, &t)) return;
        pos += t.used;
        if (t.off == 0) { if (pos < (int64_t)in.size()) (*nrec)++; return; }
        if (t.lit) (*nrec)++;
        d.insert(d.end(), (size_t)t.lit, 0u);
        pos += t.lit;
        (*nrec)++;
        // one hop lands in front of the match however long it overlaps itself: byte k has the depth of source byte k mod off, plus one
        const size_t from = d.size() - (size_t)t.off;
        for (int64_t k = 0; k < t.len; k++) {
            const uint32_t v = d[from + (size_t)(k % (int64_t)t.off)] + 1;
            d.push_back(v);
            if (v > *depth) *depth = v;
        }
    }
}

struct Tally { int parallel = 0, refused = 0, over_cap = 0, deep = 0; };

void run_case(const char *name, const std::vector<uint8_t> &in, int32_t out_cap, int want_serial, Tally &tl)
{
    std::vector<uint8_t> ref((size_t)out_cap + 1, 0xA5), got((size_t)out_cap + 1, 0xA5);
    int32_t ref_len = 0, got_len = 0;
    const int rc = jpk_lz77_decompress(in.data(), (int32_t)in.size(), ref.data(), out_cap, &ref_len);
    const bool par = rule_expand(in, got, out_cap, &got_len);
    if (want_serial >= 0) CHECK(par == !want_serial, "%s: path %s, wanted %s", name, par ? "parallel" : "serial", want_serial ? "serial" : "parallel");
    if (par) {
        tl.parallel++;
        CHECK(rc == JPK_OK, "%s: the rule decoded what the serial decoder refuses (%d)", name, rc);
        CHECK(got_len == ref_len && memcmp(got.data(), ref.data(), (size_t)ref_len) == 0, "%s: bytes or length differ (%d vs %d)", name, got_len, ref_len);
        CHECK(got[(size_t)out_cap] == 0xA5, "%s: wrote behind out_cap", name);
        return;
    }
    if (rc != JPK_OK) { tl.refused++; return; }
    uint32_t nrec = 0, depth = 0;
    stream_shape(in, &nrec, &depth);
    if (nrec > lzx::seg_cap((int64_t)in.size())) tl.over_cap++;
    else if (depth > lzx::MAX_CHASE) tl.deep++;
    else CHECK(false, "%s: handed over without a reason (%u records, cap %u, depth %u)", name, nrec, lzx::seg_cap((int64_t)in.size()), depth);
}

void put_leb(std::vector<uint8_t> &s, uint32_t v)
{
    uint8_t b[5];
    const uint32_t n = pre::leb_write(v, b);
    s.insert(s.end(), b, b + n);
}

// a random stream: sparse ones (long literal runs) stay under the record cap, dense ones go over it, chains go deep; some are damaged on purpose
std::vector<uint8_t> random_stream(std::mt19937 &g, int32_t *out_cap)
{
    auto pick = [&g](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(g() % (hi - lo + 1)); };
    std::vector<uint8_t> s;
    const bool sparse = g() % 4 != 0, small_alphabet = g() % 2 == 0;
    const uint32_t target = pick(1, 4096);
    uint32_t op = 0;
    if (g() % 8 == 0) {                                                  // a chain: one long literal run, then matches that copy one another
        const uint32_t lit = pick(700, 1200), links = pick(2, 14);
        uint32_t prev = lit;
        for (uint32_t k = 0; k < links; k++) {
            const uint32_t len = pick(4, 34), off = pick(1, prev < 30 ? prev : 30), nl = k == 0 ? 7u : 0u;
            s.push_back((uint8_t)(((len - 4) << 3) | nl));
            put_leb(s, off);
            if (k == 0) {
                put_leb(s, lit - 7);
                for (uint32_t q = 0; q < lit; q++) s.push_back((uint8_t)g());
                op += lit;
            }
            op += len;
            prev = len;
        }
    }
    while (op < target) {
        const uint32_t lit = sparse ? pick(100, 400) : pick(0, 12), len = pick(4, g() % 3 ? 40 : 600);
        if (op + lit + len > 4096) break;
        uint32_t off = pick(1, op + lit > 0 ? op + lit : 1);
        if (g() % 8 == 0) off = pick(1, off < 4 ? off : 4);               // short periods
        if (g() % 200 == 0) off = op + lit + pick(1, 5);                  // beyond the output
        const uint32_t lc = len - 4 < 31 ? len - 4 : 31, nl = lit < 7 ? lit : 7;
        s.push_back((uint8_t)((lc << 3) | nl));
        put_leb(s, off);
        if (lc == 31) put_leb(s, len - 4 - 31);
        if (nl == 7) put_leb(s, lit - 7);
        for (uint32_t k = 0; k < lit; k++) s.push_back((uint8_t)(small_alphabet ? 'a' + g() % 3 : g()));
        op += lit + len;
    }
    if (g() % 3) {
        s.push_back(pre::END_TOKEN[0]); s.push_back(pre::END_TOKEN[1]);
        const uint32_t rest = pick(0, 4096 - op < 300 ? 4096 - op : 300);
        for (uint32_t k = 0; k < rest; k++) s.push_back((uint8_t)g());
        op += rest;
    }
    if (g() % 50 == 0 && !s.empty()) s.resize(s.size() - 1 - g() % (s.size() < 8 ? s.size() : 8));      // truncated
    *out_cap = g() % 20 == 0 ? (int32_t)pick(0, op) : (int32_t)op;                                          // sometimes short
    return s;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    Tally crafted, rnd;
    for (int32_t c = 0; c < count; c++) {
        int32_t h[3];
        if (fread(h, 4, 3, f) != 3) return 2;
        std::vector<uint8_t> in((size_t)h[0]);
        if (h[0] && fread(in.data(), 1, in.size(), f) != in.size()) return 2;
        int32_t cap = h[1];
        if (cap < 0) {                                                 // exact: what the serial decoder makes of it
            std::vector<uint8_t> big(1 << 20);
            if (jpk_lz77_decompress(in.data(), (int32_t)in.size(), big.data(), (int32_t)big.size(), &cap) != JPK_OK) return 2;
        }
        char name[32];
        snprintf(name, sizeof name, "crafted %d", c);
        run_case(name, in, cap, h[2], crafted);
    }
    fclose(f);
    std::mt19937 g(20240607u);
    for (int i = 0; i < 2000; i++) {
        int32_t cap = 0;
        const std::vector<uint8_t> s = random_stream(g, &cap);
        char name[32];
        snprintf(name, sizeof name, "random %d", i);
        run_case(name, s, cap, -1, rnd);
    }
    printf("crafted %d parallel %d refused %d over_cap %d deep %d\n", count, crafted.parallel, crafted.refused, crafted.over_cap, crafted.deep);
    printf("random 2000 parallel %d refused %d over_cap %d deep %d\n", rnd.parallel, rnd.refused, rnd.over_cap, rnd.deep);
    printf("all-ok %d\n", fails);
    return fails ? 1 : 0;
}
