// The resync rule of damaged .jam archives (jampack_amd/csrc/jam_resync.hpp -- what jpk_jam_index_recover runs, and with another source of
// candidates jpk_dev_jam_index_recover) on the CPU: jrs::walk over jrs::HostSrc under several windows and candidate caps against a
// brute-force walk of this file's own, which tries every offset with header checks written out here.  Archives are made of synthetic
// frames whose payloads are chunk headers the chunk walk accepts.  Crafted damage (the cases of tests/jam_resync_model.py) and 2000 random
// archives: "JAM"-dense junk, header fields around every bound, truncations at every offset of a header.  Built with
// -fsanitize=address,undefined by tests/test_jam_resync_rule_host.py; every archive lives in a heap block of exactly its size.
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../jampack_amd/csrc/jam_resync.hpp"

namespace {

int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL " __VA_ARGS__); printf("\n"); } } while (0)

typedef std::vector<uint8_t> Bytes;
struct Span { int64_t off, len; int32_t frame; bool gap; };
bool operator==(const Span &a, const Span &b) { return a.off == b.off && a.len == b.len && a.frame == b.frame && a.gap == b.gap; }

void put_u32(Bytes &b, size_t at, uint32_t v) { memcpy(b.data() + at, &v, 4); }
void leb(Bytes &b, uint32_t v) { uint8_t t[5]; const uint32_t n = pre::leb_write(v, t); b.insert(b.end(), t, t + n); }

// a payload of `chunks` chunks that declare `olen` bytes each: 256 frequencies, olen, clen, rlen, clen bytes (fill)
Bytes payload(int chunks, uint32_t olen, uint8_t fill)
{
    Bytes p;
    for (int c = 0; c < chunks; c++) {
        for (int s = 0; s < 256; s++) leb(p, s == 7 ? olen : 0u);
        leb(p, olen); leb(p, 16u + (uint32_t)c); leb(p, olen / 2);
        p.insert(p.end(), 16 + (size_t)c, fill);
    }
    return p;
}

Bytes frame(const Bytes &p, int32_t field, int32_t psize_delta = 0)
{
    Bytes f = {'J', 'A', 'M', 1, 2, 3, 4};
    f.resize(15);
    put_u32(f, 7, (uint32_t)((int32_t)p.size() + psize_delta));
    put_u32(f, 11, (uint32_t)field);
    f.insert(f.end(), p.begin(), p.end());
    return f;
}

// the rule, written out: every check of a plausible header, the chunk walk, the declared size
bool valid_ref(const uint8_t *in, int64_t n, int64_t o, bool staged_ok, int64_t *span)
{
    if (o + 15 > n) return false;
    if (in[o] != 'J' || in[o + 1] != 'A' || in[o + 2] != 'M') return false;
    int32_t psize, field;
    memcpy(&psize, in + o + 7, 4);
    memcpy(&field, in + o + 11, 4);
    bool staged = false;
    if (staged_ok && (field & (1 << 30)) && field > 0) { staged = true; field &= ~(1 << 30); }
    if (field < (1 << 20) || field > (1000 << 20)) return false;
    if (psize < 0 || psize > (1000 << 20) || o + 15 + (int64_t)psize > n) return false;
    int64_t dec = 0;
    if (jrs::ans_decoded_size(in + o + 15, psize, &dec, nullptr) != JPK_OK) return false;
    const int64_t cap = staged ? (int64_t)((double)field * 1.05) + 4096 : field;
    if (dec < JPK_TRAILER_BYTES || dec - JPK_TRAILER_BYTES > cap) return false;
    *span = 15 + (int64_t)psize;
    return true;
}

std::vector<Span> brute(const uint8_t *in, int64_t n, bool staged_ok)
{
    std::vector<Span> out;
    int64_t g = 0;
    int32_t frames = 0;
    while (g < n) {
        int64_t o = g, span = 0;
        while (o < n && !valid_ref(in, n, o, staged_ok, &span)) o++;
        if (o > g) out.push_back(Span{g, o - g, frames, true});
        if (o == n) break;
        out.push_back(Span{o, span, frames++, false});
        g = o + span;
    }
    return out;
}

std::vector<Span> rule(const uint8_t *in, int64_t n, bool staged_ok, int64_t W, int32_t K)
{
    std::vector<Span> out;
    std::vector<int64_t> offs((size_t)(K < 1 ? jrs::DEFAULT_CANDS : K));
    jrs::HostSrc src{in, n, staged_ok, offs.data()};
    int32_t frames = 0;
    const int rc = jrs::walk(src, n, W, K, [&](const JamFrame &f) { out.push_back(Span{f.payload_off - 15, 15 + (int64_t)f.psize, frames++, false}); },
                             [&](int64_t o, int64_t len) { out.push_back(Span{o, len, frames, true}); });
    CHECK(rc == JPK_OK, "walk status %d", rc);
    return out;
}

struct Tally { int archives = 0, frames = 0, gaps = 0, clean = 0; };

void check(const char *name, const Bytes &a, bool staged_ok, Tally *t)
{
    // a heap block of exactly the archive's size: one byte read past it is the sanitizer's
    uint8_t *in = new uint8_t[a.size() ? a.size() : 1];
    if (!a.empty()) memcpy(in, a.data(), a.size());
    const int64_t n = (int64_t)a.size();
    const std::vector<Span> want = brute(in, n, staged_ok);
    int64_t at = 0;
    for (const Span &s : want) { CHECK(s.off == at && s.len > 0, "%s: the model does not tile at %lld", name, (long long)at); at += s.len; }
    CHECK(at == n, "%s: the model ends at %lld of %lld", name, (long long)at, (long long)n);
    const int64_t Ws[] = {0, 1, 15, 16, 64, 4096};
    const int32_t Ks[] = {0, 1, 2, 4};
    for (int64_t W : Ws)
        for (int32_t K : Ks) {
            const std::vector<Span> got = rule(in, n, staged_ok, W, K);
            CHECK(got == want, "%s: W %lld K %d: %zu spans, the model has %zu", name, (long long)W, K, got.size(), want.size());
        }
    t->archives++;
    bool gap = false;
    for (const Span &s : want) { if (s.gap) { t->gaps++; gap = true; } else t->frames++; }
    if (!gap) t->clean++;
    delete[] in;
}

Bytes cat(const std::vector<Bytes> &parts)
{
    Bytes a;
    for (const Bytes &p : parts) a.insert(a.end(), p.begin(), p.end());
    return a;
}

void crafted(Tally *t)
{
    const int32_t MiB = 1 << 20;
    std::vector<Bytes> f;
    for (int k = 0; k < 5; k++) f.push_back(frame(payload(1 + k % 2, 600u + 100u * (uint32_t)k, (uint8_t)('J' + k)), MiB));
    std::vector<size_t> s(6, 0);
    for (int k = 0; k < 5; k++) s[(size_t)k + 1] = s[(size_t)k] + f[(size_t)k].size();
    const Bytes a = cat(f);
    Bytes b;
    check("undamaged", a, false, t);
    check("empty", Bytes(), false, t);
    b = a; b[s[2]] ^= 1; check("magic", b, false, t);
    b = a; put_u32(b, s[2] + 11, (uint32_t)(MiB - 1)); check("blocksize_low", b, false, t);
    b = a; put_u32(b, s[2] + 11, (uint32_t)((1000 << 20) + 1)); check("blocksize_high", b, false, t);
    b = a; put_u32(b, s[2] + 7, (uint32_t)-5); check("negative_payload", b, false, t);
    b = a; put_u32(b, s[2] + 7, (uint32_t)((1000 << 20) + 1)); check("payload_above_max", b, false, t);
    b = a; put_u32(b, s[4] + 7, (uint32_t)(a.size() - s[4])); check("payload_past_end", b, false, t);
    // truncations at every offset of a header: behind the last frame, and inside the archive
    for (size_t extra = 1; extra <= 15; extra++) { b = a; b.insert(b.end(), a.begin(), a.begin() + (ptrdiff_t)extra); check("trailing", b, false, t); }
    for (size_t cut = 0; cut <= 15; cut++) { b.assign(a.begin(), a.begin() + (ptrdiff_t)(s[2] + cut)); check("truncated_header", b, false, t); }
    b = a; put_u32(b, s[2] + 7, (uint32_t)(s[3] - s[2] - 16)); check("psize_minus_1", b, false, t);
    b = a; put_u32(b, s[1] + 7, (uint32_t)(s[3] - s[1] - 15)); check("psize_swallows_next", b, false, t);
    b = a; b[s[2] + 15] ^= 1; check("first_payload_byte", b, false, t);
    b = a; b.insert(b.begin() + (ptrdiff_t)s[2], 37, (uint8_t)0x5A); check("inserted_37", b, false, t);
    b = a; b[s[1]] ^= 1; b[s[2] + 1] ^= 1; check("two_lost", b, false, t);
    b = a; b[2] ^= 1; check("first_lost", b, false, t);
    b.assign(a.begin(), a.begin() + 14); check("fourteen_bytes", b, false, t);
    const Bytes decoy = frame(Bytes(), MiB, 100);
    b = a; b[s[2]] ^= 1; memcpy(b.data() + s[2] + 15, decoy.data(), 15); check("decoy_in_lost_payload", b, false, t);
    { std::vector<Bytes> p = {f[0], f[1]}; for (int i = 0; i < 40; i++) p.push_back(decoy); p.push_back(f[2]); p.push_back(f[3]); check("decoy_flood", cat(p), false, t); }
    // a decoy whose payload passes the chunk walk is a frame of the rule: the accepted risk
    b = a; b[s[2]] ^= 1;
    { const Bytes d = frame(payload(1, 700u, 0), MiB); if (d.size() + 15 < f[2].size()) memcpy(b.data() + s[2] + 15, d.data(), d.size()); }
    check("decoy_that_walks", b, false, t);
    // staged frames: bit 30 of the field, with and without staged_ok; bit 31 never
    b = cat({f[0], frame(payload(1, 900u, 1), MiB | (1 << 30)), f[3]});
    check("staged_refused", b, false, t);
    check("staged_ok", b, true, t);
    b = cat({f[0], frame(payload(1, 900u, 1), (int32_t)(0x80000000u | (uint32_t)MiB | (1u << 30))), f[3]});
    check("bit_31", b, true, t);
    // a frame that declares more than its BlockSize allows (2 chunks of 1 MiB at BlockSize 1 MiB; staged: within 1.05 x + 4096)
    b = cat({f[0], frame(payload(2, 1u << 20, 2), MiB), f[1]});
    check("declares_too_much", b, false, t);
    b = cat({f[0], frame(payload(2, (1u << 19) + 20000u, 2), MiB | (1 << 30)), f[1]});
    check("staged_declares_within_cap", b, true, t);
}

void random_archives(Tally *t)
{
    std::mt19937 rng(20260419u);
    auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const int32_t bounds[] = {0, 1, -1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1000 << 20) - 1, 1000 << 20, (1000 << 20) + 1, (1 << 30) | (1 << 20), (1 << 30) | ((1 << 20) - 1),
                              (int32_t)0x80100000u, (int32_t)0xC0100000u, 0x7FFFFFFF};
    for (int it = 0; it < 2000; it++) {
        Bytes a;
        const int parts = 1 + (int)pick(6);
        for (int p = 0; p < parts; p++) {
            switch (pick(6)) {
            case 0: case 1: {          // a good frame, sometimes staged
                a = cat({a, frame(payload(1 + (int)pick(2), 480u + pick(3000), (uint8_t)pick(256)), (1 << 20) | (pick(4) == 0 ? (1 << 30) : 0))});
                break;
            }
            case 2: {                  // "JAM"-dense junk
                const int n = (int)pick(60);
                for (int i = 0; i < n; i++) a.push_back((uint8_t)"JAMJA"[pick(5)]);
                break;
            }
            case 3: {                  // a header with fields around the bounds, then some bytes
                Bytes h = frame(Bytes(), bounds[pick(14)]);
                put_u32(h, 7, pick(3) ? (uint32_t)pick(40) : (uint32_t)bounds[pick(14)]);
                a = cat({a, h, Bytes(pick(40), (uint8_t)0x80)});
                break;
            }
            case 4: {                  // a good frame with a damaged byte
                Bytes f = frame(payload(1, 480u + pick(2000), 3), 1 << 20);
                f[pick((uint32_t)f.size())] ^= (uint8_t)(1u << pick(8));
                a = cat({a, f});
                break;
            }
            default: {                 // a good frame with a lying payload size
                a = cat({a, frame(payload(1, 480u + pick(2000), 4), 1 << 20, (int32_t)pick(5) - 2)});
                break;
            }
            }
        }
        if (pick(3) == 0 && !a.empty()) {        // truncated: at every offset of a header over the iterations, or anywhere
            const size_t cut = pick(2) ? (size_t)pick(16) : (size_t)pick((uint32_t)a.size());
            a.resize(a.size() > cut ? a.size() - cut : 0);
        }
        char name[32];
        snprintf(name, sizeof name, "random %d", it);
        check(name, a, pick(2) != 0, t);
    }
}

}  // namespace

int main()
{
    Tally c, r;
    crafted(&c);
    printf("crafted %d frames %d gaps %d clean %d\n", c.archives, c.frames, c.gaps, c.clean);
    random_archives(&r);
    printf("random %d frames %d gaps %d clean %d\n", r.archives, r.frames, r.gaps, r.clean);
    printf("all-ok %d\n", fails);
    return fails ? 1 : 0;
}
