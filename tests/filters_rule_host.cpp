// The filter choice of prestage_rules.hpp and its host encoder on the CPU, for tests/test_filters_rule_host.py (built with
// -fsanitize=address,undefined; prestage.cpp is compiled into this program, no library is loaded):
//   lg12     against log2 for all 65 536 arguments: off by at most 1, exact at the powers of two, never decreasing
//   reorder  reorder_src(len, width, .) is the order Filters::Reorder reads in, for every width at lengths around the channel edges
//   trip     jpk_filters_decode(jpk_filters_encode(x)) == x in heap buffers of exactly the sizes the entries name, at the lengths where a
//            piece is empty, short, exactly full or one byte more, on records of several widths, skewed bytes and random bytes; and every
//            piece's header is the argmin of jpk_filters_cost (the candidate's own output bytes) in the rule's order
// Prints one line per check; exit status 0 when all hold.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../jampack_amd/csrc/prestage.cpp"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL " __VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// kind 0: random bytes; 1: skewed bytes (no filter helps); w >= 2: records of w bytes, every column a slow walk
static std::vector<uint8_t> make(uint32_t n, uint32_t kind)
{
    std::vector<uint8_t> x(n);
    uint8_t col[32];
    for (auto &c : col) c = (uint8_t)rnd();
    for (uint32_t i = 0; i < n; i++) {
        if (kind == 0) x[i] = (uint8_t)rnd();
        else if (kind == 1) x[i] = (uint8_t)(rnd() % 7u * (rnd() % 5u));
        else { uint8_t &c = col[i % kind]; c = (uint8_t)(c + rnd() % 5u - 2u); x[i] = c; }
    }
    return x;
}

int main()
{
    uint32_t prev = 0, worst = 0;
    for (uint32_t v = 1; v <= 65536u; v++) {
        const uint32_t got = pre::lg12(v);
        const double exact = 4096.0 * log2((double)v), err = fabs((double)got - exact);
        CHECK(err <= 1.0, "lg12(%u) = %u, 4096 log2 = %.3f", v, got, exact);
        CHECK(got >= prev, "lg12(%u) = %u below lg12(%u) = %u", v, got, v - 1, prev);
        if ((v & (v - 1)) == 0) CHECK(got == 4096u * (uint32_t)lround(log2((double)v)), "lg12(%u) = %u is not exact", v, got);
        if ((uint32_t)(err * 1000.0) > worst) worst = (uint32_t)(err * 1000.0);
        prev = got;
    }
    printf("lg12 checked 65536 worst_milli %u\n", worst);

    uint32_t orders = 0;
    for (uint32_t width = 1; width <= pre::FILTER_WIDTHS; width++)
        for (uint32_t len : {1u, 2u, 31u, 32u, 33u, 63u, 64u, 65u, 1000u, 65535u, 65536u}) {
            uint32_t pos = 0;
            bool ok = true;
            for (uint32_t c = 0; c < width; c++)
                for (uint32_t j = c; j < len; j += width) ok = ok && pre::reorder_src(len, width, pos++) == j;
            CHECK(ok && pos == len, "reorder_src len %u width %u", len, width);
            orders++;
        }
    printf("reorder checked %u\n", orders);

    uint32_t trips = 0, filtered = 0, stored = 0;
    for (uint32_t n : {0u, 1u, 2u, 31u, 32u, 33u, 65535u, 65536u, 65537u, 131072u, 131073u, 196613u})
        for (uint32_t kind : {0u, 1u, 2u, 3u, 7u, 29u, 31u, 32u}) {
            const std::vector<uint8_t> x = make(n, kind);
            const uint32_t total = n + 2u * ((n + pre::FBS - 1u) / pre::FBS);
            std::vector<uint8_t> s2(total), back(n);
            int32_t m = -1, k = -1;
            if (total) CHECK(jpk_filters_encode(x.data(), (int32_t)n, s2.data(), (int32_t)total - 1, &m) == JPK_E_CAPACITY, "capacity %u", n);
            CHECK(jpk_filters_encode(x.data(), (int32_t)n, s2.data(), (int32_t)total, &m) == JPK_OK && m == (int32_t)total, "encode %u kind %u", n, kind);
            CHECK(jpk_filters_decode(s2.data(), m, back.data(), (int32_t)n, &k) == JPK_OK && k == (int32_t)n && back == x, "decode %u kind %u", n, kind);
            for (uint32_t i = 0, op = 0; i < n; i += pre::FBS, op += pre::FBS + 2u) {
                const uint32_t len = n - i < pre::FBS ? n - i : pre::FBS;
                int64_t raw = 0, c = 0;
                CHECK(jpk_filters_cost(x.data() + i, (int32_t)len, 0, 0, &raw) == JPK_OK, "raw cost");
                int64_t best = raw - (raw >> 4);
                uint32_t bt = 0, bw = 0;
                for (uint32_t t = 0; t <= 2u; t += 2u)
                    for (uint32_t w = 1; w <= 32u; w++) {
                        CHECK(jpk_filters_cost(x.data() + i, (int32_t)len, (int32_t)t, (int32_t)w, &c) == JPK_OK, "cost");
                        if (c < best) { best = c; bt = t; bw = w; }
                    }
                CHECK(s2[op] == bt && s2[op + 1] == bw, "choice n %u kind %u piece %u: header %u %u, argmin %u %u", n, kind, i / pre::FBS, s2[op], s2[op + 1], bt, bw);
                (s2[op + 1] ? filtered : stored)++;
            }
            trips++;
        }
    printf("trip checked %u filtered %u stored %u\n", trips, filtered, stored);
    printf("all-ok %d\n", failures);
    return failures ? 1 : 0;
}
