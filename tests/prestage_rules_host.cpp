// The rules of prestage_rules.hpp on the CPU, for tests/test_prestage_rules_host.py (built with -fsanitize=address,undefined):
//   lpx    the serial walk of k_lpx exactly as its lane 0 runs it -- tiles of LPX_TILE bytes, the ring of LPX_RING plain bytes, ring_back,
//          step<ENC> -- against the direct-indexed host form, both directions, at the lengths where a part meets a tile edge or the ring wrap
//   parts  parts() / part_of() against the reference's loop `for (i = 0; i < len; i += len / 4)`
//   leb    leb_read(leb_write(v)) == v at the class edges, -1 for every truncated prefix
//   golden every pair of files on the command line (a stream the REFERENCE's Lpx::Encode wrote, its plain bytes): the only check here of
//          the model itself -- both forms of the lpx check call the same step and update, so that check sees the tile and ring indexing only
// Prints one line per check; exit status 0 when all hold.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../jampack_amd/csrc/prestage_rules.hpp"

using namespace pre;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL " __VA_ARGS__); printf("\n"); } } while (0)

struct Stats { uint64_t stretch = 0, tile_cross = 0, ring_cross = 0; };   // bytes coded inside stretches; stretches that go on over an edge

static void fresh(Record (*table)[256])
{
    for (int k = 0; k < 3 * 256; k++) table[k >> 8][k & 255] = fresh_record();
}

// prestage.cpp's form: the plain bytes behind position i by direct index
template <bool ENC> static void direct_part(const uint8_t *in, uint8_t *out, uint32_t plen)
{
    Record table[3][256];
    fresh(table);
    const uint8_t *plain = ENC ? in : out;
    Walk w;
    for (uint32_t i = 0; i < plen; i++) out[i] = step<ENC>(table, w, i, in[i], [&](uint32_t d) { return plain[i - d]; });
}

// k_lpx's form: heap buffers of exactly the kernel's LDS sizes, so that the sanitizer sees every index the kernel would use
template <bool ENC> static void lane0_part(const uint8_t *in, uint8_t *out, uint32_t plen, Stats *st)
{
    std::vector<Record> recs(3 * 256);
    std::vector<uint8_t> tile(LPX_TILE), ring(LPX_RING);
    Record(*table)[256] = reinterpret_cast<Record(*)[256]>(recs.data());
    fresh(table);
    Walk w;
    for (uint32_t base = 0; base < plen; base += LPX_TILE) {
        const uint32_t cnt = plen - base < LPX_TILE ? plen - base : LPX_TILE;
        const uint32_t rb = base % LPX_RING;
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t q = rb + k;
            if (ENC) ring.at(q >= LPX_RING ? q - LPX_RING : q) = in[base + k];
            else tile.at(k) = in[base + k];
        }
        uint32_t wi = rb;
        for (uint32_t k = 0; k < cnt; k++) {
            if (w.run && k == 0) st->tile_cross++;
            if (w.run && wi == 0 && base + k > 0) st->ring_cross++;
            const uint8_t o = step<ENC>(table, w, base + k, ENC ? ring.at(wi) : tile.at(k), [&](uint32_t d) {
                st->stretch++;
                return ring.at(ring_back(wi, d));
            });
            if (ENC) tile.at(k) = o;
            else ring.at(wi) = o;
            wi = wi + 1 == LPX_RING ? 0u : wi + 1;
        }
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t q = rb + k;
            out[base + k] = ENC ? tile.at(k) : ring.at(q >= LPX_RING ? q - LPX_RING : q);
        }
    }
}

template <bool ENC> static void code(bool lane0, const std::vector<uint8_t> &in, std::vector<uint8_t> &out, Stats *st)
{
    uint32_t start = 0, plen = 0;
    for (uint32_t pi = 0; part_of((uint32_t)in.size(), pi, &start, &plen); pi++) {
        if (lane0) lane0_part<ENC>(in.data() + start, out.data() + start, plen, st);
        else direct_part<ENC>(in.data() + start, out.data() + start, plen);
    }
}

static uint32_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static std::vector<uint8_t> content(int kind, uint32_t len)
{
    std::vector<uint8_t> v(len, 0);
    rng_state = 12345u + (uint32_t)kind;
    if (kind == 1) {                                                   // a 4 KiB repeat
        for (uint32_t i = 0; i < len; i++) v[i] = i < 4096u ? (uint8_t)rnd() : v[i - 4096u];
    } else if (kind == 2) {                                            // corpus-like text: words of a small vocabulary
        static const char *words[] = {"the ", "block ", "of ", "sorted ", "suffix ", "array ", "and ", "a ", "model ", "predicts ", "every ", "byte.\n",
                                      "context ", "table ", "record ", "stream "};
        for (uint32_t i = 0; i < len;) {
            const char *wd = words[rnd() & 15u];
            for (; *wd && i < len; wd++) v[i++] = (uint8_t)*wd;
        }
    } else if (kind == 3) {
        for (uint32_t i = 0; i < len; i++) v[i] = (uint8_t)rnd();
    }
    return v;
}

static void check_lpx()
{
    static const char *names[] = {"zeros", "rep4k", "text", "random"};
    static const uint32_t lens[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 65536, 65540, 327680, 327684, 360001};
    for (int kind = 0; kind < 4; kind++)
        for (uint32_t len : lens) {
            const std::vector<uint8_t> plain = content(kind, len);
            std::vector<uint8_t> enc_d(len), enc_l(len), dec_d(len), dec_l(len);
            Stats se, sd, none;
            code<true>(false, plain, enc_d, &none);
            code<true>(true, plain, enc_l, &se);
            code<false>(false, enc_d, dec_d, &none);
            code<false>(true, enc_d, dec_l, &sd);
            CHECK(enc_l == enc_d, "lpx %s %u: the lane-0 encoder differs from the direct form", names[kind], len);
            CHECK(dec_l == dec_d, "lpx %s %u: the lane-0 decoder differs from the direct form", names[kind], len);
            CHECK(dec_d == plain, "lpx %s %u: decode(encode(x)) != x", names[kind], len);
            code<false>(false, plain, dec_d, &none);                   // any byte string is a stream: stretches that end on a wrong guess
            code<false>(true, plain, dec_l, &none);
            CHECK(dec_l == dec_d, "lpx %s %u: the lane-0 decoder differs from the direct form on the plain bytes as a stream", names[kind], len);
            CHECK(se.stretch == sd.stretch, "lpx %s %u: encoder and decoder disagree on the stretches", names[kind], len);
            printf("lpx %s %u enc_stretch %llu enc_tile_cross %llu enc_ring_cross %llu dec_stretch %llu dec_tile_cross %llu dec_ring_cross %llu\n", names[kind], len,
                   (unsigned long long)se.stretch, (unsigned long long)se.tile_cross, (unsigned long long)se.ring_cross, (unsigned long long)sd.stretch,
                   (unsigned long long)sd.tile_cross, (unsigned long long)sd.ring_cross);
        }
}

static void check_parts()
{
    uint32_t checked = 0;
    for (uint32_t len = 0; len <= 4100; len++) {
        std::vector<uint32_t> starts, lens;                            // Lpx::Decode's loop (lpx.cpp:158-169); one part below 4 bytes
        const uint32_t part = len / 4;
        if (part == 0) { if (len) { starts.push_back(0); lens.push_back(len); } }
        else for (uint32_t i = 0; i < len; i += part) { starts.push_back(i); lens.push_back(i + part < len ? part : len - i); }
        CHECK(parts(len) == starts.size(), "parts(%u) = %u, the loop makes %zu", len, parts(len), starts.size());
        uint32_t s = 0, l = 0;
        for (uint32_t pi = 0; pi < starts.size(); pi++) {
            const bool ok = part_of(len, pi, &s, &l);
            CHECK(ok && s == starts[pi] && l == lens[pi], "part_of(%u, %u) = %d %u %u, the loop has %u %u", len, pi, (int)ok, s, l, starts[pi], lens[pi]);
        }
        CHECK(!part_of(len, (uint32_t)starts.size(), &s, &l), "part_of(%u, %zu) finds a part behind the last one", len, starts.size());
        checked++;
    }
    printf("parts checked %u\n", checked);
}

static void check_leb()
{
    static const uint32_t edges[] = {0u, 126u, 127u, 16509u, 16510u, 2113660u, 2113661u, 270549115u, 270549116u, 0x7fffffffu};
    static const uint32_t sizes[] = {1, 1, 2, 2, 3, 3, 4, 4, 5, 5};
    uint32_t checked = 0;
    for (int e = 0; e < 10; e++) {
        std::vector<uint8_t> buf(5);
        const uint32_t n = leb_write(edges[e], buf.data());
        CHECK(n == sizes[e], "leb_write(%u) takes %u bytes", edges[e], n);
        buf.resize(n);                                                 // exact size: a read past the code is a sanitizer error
        uint32_t v = 0xdeadbeefu;
        const uint8_t *code = buf.data();
        CHECK(leb_read(code, n, &v) == (int)n && v == edges[e], "leb_read(leb_write(%u)) = %u", edges[e], v);
        for (uint32_t cut = 0; cut < n; cut++) {
            const std::vector<uint8_t> head(buf.begin(), buf.begin() + cut);
            CHECK(leb_read(head.data(), cut, &v) == -1, "leb_read of %u of the %u bytes of %u is not -1", cut, n, edges[e]);
        }
        checked++;
    }
    const uint8_t five[6] = {0, 0, 0, 0, 0, 0x80};                      // a fifth byte without bit 7: no code is that long
    uint32_t v = 0;
    CHECK(leb_read(five, 6, &v) == -1, "leb_read accepts a six-byte code");
    printf("leb checked %u\n", checked);
}

static std::vector<uint8_t> read_file(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static void check_golden(const char *stream_path, const char *plain_path)
{
    const std::vector<uint8_t> stream = read_file(stream_path), plain = read_file(plain_path);
    CHECK(!stream.empty() && stream.size() == plain.size(), "golden %s: %zu stream bytes, %zu plain bytes", stream_path, stream.size(), plain.size());
    std::vector<uint8_t> out(stream.size());
    Stats st, none;
    for (int lane0 = 0; lane0 < 2; lane0++) {
        code<false>(lane0 != 0, stream, out, &st);
        CHECK(out == plain, "golden %s: the %s decoder does not give the plain bytes", stream_path, lane0 ? "lane-0" : "direct");
        code<true>(lane0 != 0, plain, out, &none);
        CHECK(out == stream, "golden %s: the %s encoder does not give the reference's stream", stream_path, lane0 ? "lane-0" : "direct");
    }
    size_t changed = 0;
    for (size_t i = 0; i < stream.size(); i++) changed += stream[i] != plain[i];
    printf("golden %zu bytes changed %zu stretch %llu\n", stream.size(), changed, (unsigned long long)st.stretch);
}

int main(int argc, char **argv)
{
    check_leb();
    check_parts();
    check_lpx();
    for (int i = 1; i + 1 < argc; i += 2) check_golden(argv[i], argv[i + 1]);
    printf(failures ? "FAILED %d\n" : "all-ok %d\n", failures);
    return failures ? 1 : 0;
}
