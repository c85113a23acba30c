// The size rule of the first LZ77 stage (lzx::Size / lzx::step of jampack_amd/csrc/lz_expand.hpp -- what k_lz77_sizes compiles) on the
// CPU: the host form of the walk and jpk_lz77_size against jpk_lz77_decompress (prestage.cpp), status and out_len, on the crafted
// streams of tests/lz_expand_cases.py (argv[1]) and on 2000 random token streams of at most 4 KiB of output, some of them damaged.
// Every stream is checked at out_cap = its exact size, its size - 1, 0 and a large cap; the size of a stream the decoder refuses at
// any cap is the one its case names (crafted) or its generator aimed at (random).  Built with -fsanitize=address,undefined by
// tests/test_lz_sizes_rule_host.py.
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

constexpr int32_t LARGE = 1 << 20;

// the rule as a kernel runs it: one parse and one step per token
int rule_size(const std::vector<uint8_t> &in, int32_t out_cap, int32_t *out_len)
{
    const int64_t in_len = (int64_t)in.size();
    lzx::Size s;
    int64_t steps = 0;
    while (lzx::more(s, in_len)) {
        pre::Token t;
        const int64_t before = s.pos;
        const bool parsed = pre::parse_token([&](int j) { return (uint32_t)in.at((size_t)(before + j)); }, in_len - s.pos, &t);
        lzx::step(s, parsed, t, in_len, (int64_t)out_cap);
        CHECK(s.done || s.pos >= before + 2, "the walk did not move at %lld", (long long)before);
        CHECK(s.pos <= in_len, "the walk left the input at %lld", (long long)before);
        if (++steps > in_len) { CHECK(false, "more steps than bytes"); break; }
    }
    *out_len = lzx::out_len(s);
    return s.status;
}

struct Tally { int ok = 0, corrupt = 0, capacity = 0; };

// one stream at one capacity; what the decoder said goes into *seen (bit 0 OK, 1 corrupt, 2 capacity)
void run_at(const char *name, const std::vector<uint8_t> &in, int32_t cap, int *seen)
{
    std::vector<uint8_t> out((size_t)cap + 1, 0xA5);
    int32_t ref_len = 0, rule_len = -1, lib_len = -1;
    const int rc = jpk_lz77_decompress(in.data(), (int32_t)in.size(), out.data(), cap, &ref_len);
    if (rc != JPK_OK) ref_len = 0;                                     // (the decoder leaves *out_len alone when it fails; the device form gives 0)
    const int rr = rule_size(in, cap, &rule_len);
    const int rl = jpk_lz77_size(in.data(), (int32_t)in.size(), cap, &lib_len);
    CHECK(rr == rc && rule_len == ref_len, "%s cap %d: rule %d / %d, decoder %d / %d", name, cap, rr, rule_len, rc, ref_len);
    CHECK(rl == rr && lib_len == rule_len, "%s cap %d: jpk_lz77_size %d / %d, rule %d / %d", name, cap, rl, lib_len, rr, rule_len);
    CHECK(rc == JPK_OK || rc == JPK_E_CORRUPT || rc == JPK_E_CAPACITY, "%s cap %d: status %d", name, cap, rc);
    *seen |= rc == JPK_OK ? 1 : rc == JPK_E_CORRUPT ? 2 : 4;
}

void run_stream(const char *name, const std::vector<uint8_t> &in, int32_t size_hint, Tally &tl)
{
    int32_t size = size_hint;
    {
        std::vector<uint8_t> big((size_t)LARGE);
        int32_t n = 0;
        if (jpk_lz77_decompress(in.data(), (int32_t)in.size(), big.data(), LARGE, &n) == JPK_OK) size = n;
    }
    int seen = 0;
    run_at(name, in, size, &seen);
    if (size > 0) run_at(name, in, size - 1, &seen);
    run_at(name, in, 0, &seen);
    run_at(name, in, LARGE, &seen);
    tl.ok += seen & 1; tl.corrupt += (seen >> 1) & 1; tl.capacity += (seen >> 2) & 1;
}

void put_leb(std::vector<uint8_t> &s, uint32_t v)
{
    uint8_t b[5];
    const uint32_t n = pre::leb_write(v, b);
    s.insert(s.end(), b, b + n);
}

// a random stream of *aim output bytes: short and long literal runs, short and long matches, now and then an offset beyond the output;
// some are cut short and some have a byte replaced, which makes tokens of any shape (lengths and literal counts near 2^31 included)
std::vector<uint8_t> random_stream(std::mt19937 &g, int32_t *aim)
{
    auto pick = [&g](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(g() % (hi - lo + 1)); };
    std::vector<uint8_t> s;
    const uint32_t target = pick(0, 4096);
    uint32_t op = 0;
    while (op < target) {
        const uint32_t lit = g() % 4 ? pick(0, 12) : pick(7, 300), len = pick(4, g() % 3 ? 40 : 600);
        if (op + lit + len > 4096) break;
        uint32_t off = pick(1, op + lit > 0 ? op + lit : 1);
        if (g() % 150 == 0) off = op + lit + pick(1, 5);                  // beyond the output
        const uint32_t lc = len - 4 < 31 ? len - 4 : 31, nl = lit < 7 ? lit : 7;
        s.push_back((uint8_t)((lc << 3) | nl));
        put_leb(s, off);
        if (lc == 31) put_leb(s, len - 4 - 31);
        if (nl == 7) put_leb(s, lit - 7);
        for (uint32_t k = 0; k < lit; k++) s.push_back((uint8_t)g());
        op += lit + len;
    }
    if (g() % 3) {
        s.push_back(pre::END_TOKEN[0]); s.push_back(pre::END_TOKEN[1]);
        const uint32_t rest = pick(0, 4096 - op < 300 ? 4096 - op : 300);
        for (uint32_t k = 0; k < rest; k++) s.push_back((uint8_t)g());
        op += rest;
    }
    if (g() % 25 == 0 && !s.empty()) s.resize(s.size() - 1 - g() % (s.size() < 8 ? s.size() : 8));      // cut short
    if (g() % 20 == 0 && !s.empty()) s[g() % s.size()] = (uint8_t)g();                                    // a byte replaced
    *aim = (int32_t)op;
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
        char name[32];
        snprintf(name, sizeof name, "crafted %d", c);
        run_stream(name, in, h[1] < 0 ? 0 : h[1], crafted);
    }
    fclose(f);
    // the arguments, as jpk_lz77_decompress checks them
    {
        const uint8_t two[2] = {0x04, 0x80};
        int32_t n = -1;
        CHECK(jpk_lz77_size(two, 2, 0, nullptr) == JPK_E_ARG && jpk_lz77_size(two, -1, 0, &n) == JPK_E_ARG && jpk_lz77_size(two, 2, -1, &n) == JPK_E_ARG &&
                  jpk_lz77_size(nullptr, 2, 0, &n) == JPK_E_ARG,
              "argument checks");
        CHECK(jpk_lz77_size(nullptr, 0, 0, &n) == JPK_OK && n == 0, "the empty stream");
    }
    std::mt19937 g(20250912u);
    for (int i = 0; i < 2000; i++) {
        int32_t aim = 0;
        const std::vector<uint8_t> s = random_stream(g, &aim);
        char name[32];
        snprintf(name, sizeof name, "random %d", i);
        run_stream(name, s, aim, rnd);
    }
    printf("crafted %d ok %d corrupt %d capacity %d\n", count, crafted.ok, crafted.corrupt, crafted.capacity);
    printf("random 2000 ok %d corrupt %d capacity %d\n", rnd.ok, rnd.corrupt, rnd.capacity);
    printf("all-ok %d\n", fails);
    return fails ? 1 : 0;
}
