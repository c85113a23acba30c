// The deep rule of the parallel LZ77 expander (jampack_amd/csrc/lz_expand.hpp: lzx::deep_step, lzx::deep_seg_cap, lzx::source with
// lzx::DEEP_CHASE hops -- what k_lzd_plan and k_lzd_copy compile) on the CPU against jpk_lz77_decompress (prestage.cpp): the crafted
// streams of tests/lz_deep_cases.py and the hostile ones of tests/lz_expand_cases.py (argv[1], packed by lz_expand_cases.pack) and 2000
// random token streams of at most 16 KiB of output.  A block the rule decodes must have the serial decoder's status JPK_OK, its length and
// its bytes; a block the rule hands over must be one the serial decoder refuses, one over the record budget behind some token, or one
// with a byte more than lzx::DEEP_CHASE matches from its literal -- all three recomputed here without the rule.  At most a quarter of the
// random streams may go the serial way.  Built with -fsanitize=address,undefined by tests/test_lz_deep_rule_host.py.
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

// the rule as the kernels run it: true = decoded from the records (out, *out_len), false = handed to the serial decoder.  Nothing is
// written to `out` before the plan has passed, and nothing at or behind out_cap.
bool rule_expand(const std::vector<uint8_t> &in, std::vector<uint8_t> &out, int32_t out_cap, int32_t *out_len)
{
    const int64_t in_len = (int64_t)in.size();
    const uint32_t cap = lzx::deep_seg_cap(out_cap);
    std::vector<lzx::Seg> segs(cap);                                    // exactly the cap: a record too many is a heap overflow
    lzx::Plan p;
    while (lzx::more(p, in_len)) {
        pre::Token t;
        const uint8_t *at = in.data() + p.pos;
        const bool parsed = pre::parse_token([at](int j) { return (uint32_t)at[j]; }, in_len - p.pos, &t);
        lzx::deep_step(p, parsed, t, in_len, (int64_t)out_cap, cap, [&segs](uint32_t i, const lzx::Seg &s) { segs.at(i) = s; });
    }
    if (p.serial) return false;
    CHECK(p.op <= out_cap, "the plan passed %lld bytes into %d", (long long)p.op, out_cap);
    for (uint32_t i = 0; i < p.nseg; i++) {
        CHECK(segs[i].len > 0 && segs[i].out == (i ? segs[i - 1].out + segs[i - 1].len : 0u), "records out of order at %u", i);
        CHECK(!segs[i].match || (i > 0 && segs[i].src >= 1 && segs[i].src <= segs[i].out), "match record %u", i);
        CHECK(segs[i].match || (uint64_t)segs[i].src + segs[i].len <= (uint64_t)in_len, "literal record %u", i);
    }
    for (int64_t pos = 0; pos < p.op; pos++) {
        const uint32_t idx = lzx::find(segs.data(), p.nseg, (uint32_t)pos);
        uint32_t io = 0;
        if (!lzx::source(segs.data(), idx, segs[idx], (uint32_t)pos, lzx::DEEP_CHASE, &io)) return false;
        out.at((size_t)pos) = in.at(io);
    }
    *out_len = (int32_t)p.op;
    return true;
}

// without the rule, for a stream the serial decoder accepts: is it over the budget behind some token, and its deepest byte
void stream_shape(const std::vector<uint8_t> &in, bool *over, uint32_t *depth)
{
    std::vector<uint32_t> d;
    int64_t pos = 0, nrec = 0;
    *over = false; *depth = 0;
    while (pos < (int64_t)in.size()) {
        pre::Token t;
        const uint8_t *at = in.data() + pos;
        if (!pre::parse_token([at](int j) { return (uint32_t)at[j]; }, (int64_t)in.size() - pos, &t)) return;
        pos += t.used;
        if (t.off == 0) {
            const int64_t rest = (int64_t)in.size() - pos;
            if (rest) nrec++;
            if (nrec > ((int64_t)d.size() + rest) / 128 + 4) *over = true;
            return;
        }
        if (t.lit) nrec++;
        d.insert(d.end(), (size_t)t.lit, 0u);
        pos += t.lit;
        nrec++;
        // one hop lands in front of the match however long it overlaps itself: byte k has the depth of source byte k mod off, plus one
        const size_t from = d.size() - (size_t)t.off;
        for (int64_t k = 0; k < t.len; k++) {
            const uint32_t v = d[from + (size_t)(k % (int64_t)t.off)] + 1;
            d.push_back(v);
            if (v > *depth) *depth = v;
        }
        if (nrec > (int64_t)d.size() / 128 + 4) *over = true;
    }
}

struct Tally { int parallel = 0, refused = 0, over = 0, deep = 0, model_serial = 0; };

void run_case(const char *name, const std::vector<uint8_t> &in, int32_t out_cap, int want_serial, Tally &tl)
{
    std::vector<uint8_t> ref((size_t)out_cap + 1, 0xA5), got((size_t)out_cap + 1, 0xA5);
    int32_t ref_len = 0, got_len = 0;
    const int rc = jpk_lz77_decompress(in.data(), (int32_t)in.size(), ref.data(), out_cap, &ref_len);
    // the model alone: the serial decoder's verdict and this file's own walk
    bool over = false;
    uint32_t depth = 0;
    if (rc == JPK_OK) stream_shape(in, &over, &depth);
    const bool model_serial = rc != JPK_OK || over || depth > lzx::DEEP_CHASE;
    if (model_serial) tl.model_serial++;
    const bool par = rule_expand(in, got, out_cap, &got_len);
    if (want_serial >= 0) CHECK(par == !want_serial, "%s: path %s, wanted %s", name, par ? "parallel" : "serial", want_serial ? "serial" : "parallel");
    CHECK(par == !model_serial, "%s: path %s, the model says %s (status %d, over the budget %d, depth %u)", name, par ? "parallel" : "serial",
          model_serial ? "serial" : "parallel", rc, (int)over, depth);
    if (par) {
        tl.parallel++;
        CHECK(rc == JPK_OK, "%s: the rule decoded what the serial decoder refuses (%d)", name, rc);
        CHECK(got_len == ref_len && memcmp(got.data(), ref.data(), (size_t)ref_len) == 0, "%s: bytes or length differ (%d vs %d)", name, got_len, ref_len);
        CHECK(got[(size_t)out_cap] == 0xA5, "%s: wrote behind out_cap", name);
        return;
    }
    if (rc != JPK_OK) tl.refused++;
    else if (over) tl.over++;
    else tl.deep++;
}

void put_leb(std::vector<uint8_t> &s, uint32_t v)
{
    uint8_t b[5];
    const uint32_t n = pre::leb_write(v, b);
    s.insert(s.end(), b, b + n);
}

void put_tok(std::vector<uint8_t> &s, uint32_t len, uint32_t off, uint32_t lit, std::mt19937 &g, bool small_alphabet)
{
    const uint32_t lc = len - 4 < 31 ? len - 4 : 31, nl = lit < 7 ? lit : 7;
    s.push_back((uint8_t)((lc << 3) | nl));
    put_leb(s, off);
    if (lc == 31) put_leb(s, len - 4 - 31);
    if (nl == 7) put_leb(s, lit - 7);
    for (uint32_t k = 0; k < lit; k++) s.push_back((uint8_t)(small_alphabet ? 'a' + g() % 3 : g()));
}

// A random stream of at most MAX_OUT bytes of output.  Most are what the dedupe writes -- matches of 256 bytes and more, any distance,
// short periods among them -- and stay inside the budget; one in ten is dense (short matches: over the budget within its first tokens),
// one in twelve a chain of matches that copy one another 20 to 45 deep; some are damaged on purpose.
constexpr uint32_t MAX_OUT = 16384;
std::vector<uint8_t> random_stream(std::mt19937 &g, int32_t *out_cap)
{
    auto pick = [&g](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(g() % (hi - lo + 1)); };
    std::vector<uint8_t> s;
    const bool dense = g() % 10 == 0, small_alphabet = g() % 2 == 0;
    const uint32_t target = pick(1, MAX_OUT);
    uint32_t op = 0;
    if (g() % 12 == 0) {                                                 // a chain: literals, then matches that each copy the one in front
        const uint32_t lit = pick(300, 700), links = pick(20, 45), len = pick(256, 300), off = g() % 2 ? len : pick(1, 20);
        for (uint32_t k = 0; k < links; k++) put_tok(s, len, off, k == 0 ? lit : 0u, g, small_alphabet);
        op = lit + links * len;
    }
    while (op < target) {
        uint32_t lit = dense ? pick(0, 12) : (g() % 3 ? 0u : pick(1, 500));
        const uint32_t len = dense ? pick(4, 40) : pick(256, 1500);
        if (op + lit == 0) lit = dense ? pick(1, 12) : pick(256, 500);     // a match needs something in front of it
        if (op + lit + len > MAX_OUT) break;
        uint32_t off = pick(1, op + lit > 0 ? op + lit : 1);
        if (g() % 6 == 0) off = pick(1, off < 20 ? off : 20);              // short periods
        if (g() % 300 == 0) off = op + lit + pick(1, 5);                   // beyond the output
        put_tok(s, len, off, lit, g, small_alphabet);
        op += lit + len;
    }
    if (g() % 3) {
        s.push_back(pre::END_TOKEN[0]); s.push_back(pre::END_TOKEN[1]);
        const uint32_t rest = pick(0, MAX_OUT - op < 300 ? MAX_OUT - op : 300);
        for (uint32_t k = 0; k < rest; k++) s.push_back((uint8_t)g());
        op += rest;
    }
    if (g() % 60 == 0 && !s.empty()) s.resize(s.size() - 1 - g() % (s.size() < 8 ? s.size() : 8));      // truncated
    *out_cap = g() % 25 == 0 ? (int32_t)pick(0, op) : (int32_t)op;                                          // sometimes short
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
    std::mt19937 g(20241020u);
    for (int i = 0; i < 2000; i++) {
        int32_t cap = 0;
        const std::vector<uint8_t> s = random_stream(g, &cap);
        char name[32];
        snprintf(name, sizeof name, "random %d", i);
        run_case(name, s, cap, -1, rnd);
    }
    CHECK(4 * rnd.model_serial <= 2000, "the generator sends %d of 2000 random streams the serial way by the model: more than a quarter", rnd.model_serial);
    printf("limits %u %u %u\n", lzx::DEEP_CHASE, lzx::DEEP_BYTES, lzx::DEEP_SLACK);
    printf("crafted %d parallel %d refused %d over %d deep %d\n", count, crafted.parallel, crafted.refused, crafted.over, crafted.deep);
    printf("random 2000 parallel %d refused %d over %d deep %d\n", rnd.parallel, rnd.refused, rnd.over, rnd.deep);
    printf("all-ok %d\n", fails);
    return fails ? 1 : 0;
}
