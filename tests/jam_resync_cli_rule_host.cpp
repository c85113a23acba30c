// The resync rule of damaged stock-CLI .jam archives (jampack_amd/csrc/jam_resync.hpp with jrs::HostSrc::cli -- what jpk_jam_index_recover
// runs for kind JPK_JAM_INDEX_CLI in front of its decode) on the CPU: jrs::walk over jrs::HostSrc{..., cli = true} under several windows
// and candidate caps against a brute-force walk of this file's own, which tries every offset with the checks written out here: a header
// without a staged bit, chunk headers that walk, and a declared size of at most (int64_t)(BlockSize * 1.05) + 4096 behind the trailer.
// Archives are made of synthetic frames whose payloads are chunk headers the chunk walk accepts; the declared sizes stand at BlockSize,
// BlockSize + 1, the cap and the cap + 1.  Crafted damage and 800 random archives.  Built with -fsanitize=address,undefined by
// tests/test_jam_resync_cli_rule_host.py; every archive lives in a heap block of exactly its size.
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

constexpr int32_t MiB = 1 << 20;
constexpr int64_t CAP = (int64_t)(MiB * 1.05) + 4096;        // what a stock-CLI frame of BlockSize 1 MiB may declare behind the trailer

void put_u32(Bytes &b, size_t at, uint32_t v) { memcpy(b.data() + at, &v, 4); }
void leb(Bytes &b, uint32_t v) { uint8_t t[5]; const uint32_t n = pre::leb_write(v, t); b.insert(b.end(), t, t + n); }

// one chunk that declares `olen` bytes: 256 frequencies, olen, clen, rlen, clen bytes (fill)
void chunk(Bytes &p, uint32_t olen, uint32_t clen, uint8_t fill)
{
    for (int s = 0; s < 256; s++) leb(p, s == 7 ? olen : 0u);
    leb(p, olen); leb(p, clen); leb(p, olen / 2);
    p.insert(p.end(), (size_t)clen, fill);
}

// a payload of `chunks` chunks that declare `olen` bytes each
Bytes payload(int chunks, uint32_t olen, uint8_t fill)
{
    Bytes p;
    for (int c = 0; c < chunks; c++) chunk(p, olen, 16u + (uint32_t)c, fill);
    return p;
}

// a payload that declares `total` bytes in all: chunks of at most JPK_ANS_CHUNK
Bytes payload_of(int64_t total, uint8_t fill)
{
    Bytes p;
    uint32_t c = 0;
    do {
        const uint32_t olen = (uint32_t)(total < JPK_ANS_CHUNK ? total : JPK_ANS_CHUNK);
        chunk(p, olen, 16u + c++, fill);
        total -= olen;
    } while (total > 0);
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

// the rule, written out: every check of a plausible header (no staged bit: bit 30 puts the field above MAX_BLOCKSIZE), the chunk walk, the
// declared size -- cli: against the stage buffers of the stock CLI, otherwise against the BlockSize
bool valid_ref(const uint8_t *in, int64_t n, int64_t o, bool cli, int64_t *span)
{
    if (o + 15 > n) return false;
    if (in[o] != 'J' || in[o + 1] != 'A' || in[o + 2] != 'M') return false;
    int32_t psize, field;
    memcpy(&psize, in + o + 7, 4);
    memcpy(&field, in + o + 11, 4);
    if (field < (1 << 20) || field > (1000 << 20)) return false;
    if (psize < 0 || psize > (1000 << 20) || o + 15 + (int64_t)psize > n) return false;
    int64_t dec = 0;
    if (jrs::ans_decoded_size(in + o + 15, psize, &dec, nullptr) != JPK_OK) return false;
    const int64_t cap = cli ? (int64_t)(field * 1.05) + 4096 : field;
    if (dec < JPK_TRAILER_BYTES || dec - JPK_TRAILER_BYTES > cap) return false;
    *span = 15 + (int64_t)psize;
    return true;
}

std::vector<Span> brute(const uint8_t *in, int64_t n, bool cli)
{
    std::vector<Span> out;
    int64_t g = 0;
    int32_t frames = 0;
    while (g < n) {
        int64_t o = g, span = 0;
        while (o < n && !valid_ref(in, n, o, cli, &span)) o++;
        if (o > g) out.push_back(Span{g, o - g, frames, true});
        if (o == n) break;
        out.push_back(Span{o, span, frames++, false});
        g = o + span;
    }
    return out;
}

std::vector<Span> rule(const uint8_t *in, int64_t n, bool cli, int64_t W, int32_t K)
{
    std::vector<Span> out;
    std::vector<int64_t> offs((size_t)(K < 1 ? jrs::DEFAULT_CANDS : K));
    jrs::HostSrc src{in, n, false, offs.data(), cli};
    int32_t frames = 0;
    const int rc = jrs::walk(src, n, W, K, [&](const JamFrame &f) {
        CHECK(!f.staged && f.block_size >= MiB, "a frame with a staged bit");
        out.push_back(Span{f.payload_off - 15, 15 + (int64_t)f.psize, frames++, false});
    }, [&](int64_t o, int64_t len) { out.push_back(Span{o, len, frames, true}); });
    CHECK(rc == JPK_OK, "walk status %d", rc);
    return out;
}

struct Tally { int archives = 0, frames = 0, gaps = 0, clean = 0; };

// -> the frames of the model
int check(const char *name, const Bytes &a, bool cli, Tally *t)
{
    // a heap block of exactly the archive's size: one byte read past it is the sanitizer's
    uint8_t *in = new uint8_t[a.size() ? a.size() : 1];
    if (!a.empty()) memcpy(in, a.data(), a.size());
    const int64_t n = (int64_t)a.size();
    const std::vector<Span> want = brute(in, n, cli);
    int64_t at = 0;
    for (const Span &s : want) { CHECK(s.off == at && s.len > 0, "%s: the model does not tile at %lld", name, (long long)at); at += s.len; }
    CHECK(at == n, "%s: the model ends at %lld of %lld", name, (long long)at, (long long)n);
    const int64_t Ws[] = {0, 1, 15, 16, 64, 4096};
    const int32_t Ks[] = {0, 1, 2, 4};
    for (int64_t W : Ws)
        for (int32_t K : Ks) {
            const std::vector<Span> got = rule(in, n, cli, W, K);
            CHECK(got == want, "%s: W %lld K %d: %zu spans, the model has %zu", name, (long long)W, K, got.size(), want.size());
        }
    t->archives++;
    bool gap = false;
    int frames = 0;
    for (const Span &s : want) { if (s.gap) { t->gaps++; gap = true; } else frames++; }
    t->frames += frames;
    if (!gap) t->clean++;
    delete[] in;
    return frames;
}

Bytes cat(const std::vector<Bytes> &parts)
{
    Bytes a;
    for (const Bytes &p : parts) a.insert(a.end(), p.begin(), p.end());
    return a;
}

void crafted(Tally *t)
{
    std::vector<Bytes> f;
    for (int k = 0; k < 5; k++) f.push_back(frame(payload(1 + k % 2, 600u + 100u * (uint32_t)k, (uint8_t)('J' + k)), MiB));
    std::vector<size_t> s(6, 0);
    for (int k = 0; k < 5; k++) s[(size_t)k + 1] = s[(size_t)k] + f[(size_t)k].size();
    const Bytes a = cat(f);
    Bytes b;
    CHECK(check("undamaged", a, true, t) == 5, "undamaged");
    CHECK(check("empty", Bytes(), true, t) == 0, "empty");
    // what a frame may declare: BlockSize and the cap hold, the cap + 1 never; above BlockSize only a stock-CLI frame
    const int64_t sizes[] = {MiB, (int64_t)MiB + 1, CAP, CAP + 1};
    const int with_cli[] = {3, 3, 3, 2}, without[] = {3, 2, 2, 2};
    for (int i = 0; i < 4; i++) {
        char name[48];
        b = cat({f[0], frame(payload_of(sizes[i] + JPK_TRAILER_BYTES, 2), MiB), f[1]});
        snprintf(name, sizeof name, "declares %lld", (long long)sizes[i]);
        CHECK(check(name, b, true, t) == with_cli[i], "%s: frames of a stock-CLI walk", name);
        CHECK(check(name, b, false, t) == without[i], "%s: frames of a plain walk", name);
    }
    // the cap follows the BlockSize: 2 MiB + 1 at BlockSize 2 MiB only for a stock-CLI frame, its cap + 1 never
    b = cat({f[0], frame(payload_of(2 * (int64_t)MiB + 1 + JPK_TRAILER_BYTES, 2), 2 * MiB), f[1]});
    CHECK(check("declares 2 MiB + 1", b, true, t) == 3 && check("declares 2 MiB + 1", b, false, t) == 2, "2 MiB + 1");
    b = cat({f[0], frame(payload_of((int64_t)(2 * MiB * 1.05) + 4096 + 1 + JPK_TRAILER_BYTES, 2), 2 * MiB), f[1]});
    CHECK(check("declares cap(2 MiB) + 1", b, true, t) == 2, "cap(2 MiB) + 1");
    // less than the trailer
    b = cat({f[0], frame(payload_of(JPK_TRAILER_BYTES - 1, 2), MiB), f[1]});
    CHECK(check("declares less than the trailer", b, true, t) == 2, "trailer - 1");
    b = cat({f[0], frame(payload_of(JPK_TRAILER_BYTES, 2), MiB), f[1]});
    CHECK(check("declares the trailer", b, true, t) == 3, "trailer");
    // a staged header is never plausible for a stock-CLI archive; bit 31 never
    b = cat({f[0], frame(payload(1, 900u, 1), MiB | (1 << 30)), f[3]});
    CHECK(check("staged_header", b, true, t) == 2, "staged_header");
    b = cat({f[0], frame(payload(1, 900u, 1), (int32_t)(0x80000000u | (uint32_t)MiB | (1u << 30))), f[3]});
    CHECK(check("bit_31", b, true, t) == 2, "bit_31");
    // crafted damage
    b = a; b[s[2]] ^= 1; CHECK(check("magic", b, true, t) == 4, "magic");
    b = a; put_u32(b, s[2] + 11, (uint32_t)(MiB - 1)); CHECK(check("blocksize_low", b, true, t) == 4, "blocksize_low");
    b = a; put_u32(b, s[2] + 11, (uint32_t)((1000 << 20) + 1)); CHECK(check("blocksize_high", b, true, t) == 4, "blocksize_high");
    b = a; put_u32(b, s[2] + 7, (uint32_t)-5); CHECK(check("negative_payload", b, true, t) == 4, "negative_payload");
    b = a; put_u32(b, s[2] + 7, (uint32_t)-1); CHECK(check("payload_minus_one", b, true, t) == 4, "payload_minus_one");
    b = a; put_u32(b, s[2] + 7, (uint32_t)((1000 << 20) + 1)); CHECK(check("payload_above_max", b, true, t) == 4, "payload_above_max");
    b = a; put_u32(b, s[4] + 7, (uint32_t)(a.size() - s[4])); CHECK(check("payload_past_end", b, true, t) == 4, "payload_past_end");
    for (size_t extra = 1; extra <= 15; extra++) { b = a; b.insert(b.end(), a.begin(), a.begin() + (ptrdiff_t)extra); check("trailing", b, true, t); }
    for (size_t cut = 0; cut <= 15; cut++) { b.assign(a.begin(), a.begin() + (ptrdiff_t)(s[2] + cut)); check("truncated_header", b, true, t); }
    b.assign(a.begin(), a.begin() + (ptrdiff_t)(s[4] + 15 + 40)); CHECK(check("truncated_payload", b, true, t) == 4, "truncated_payload");
    b = a; put_u32(b, s[2] + 7, (uint32_t)(s[3] - s[2] - 16)); check("psize_minus_1", b, true, t);
    b = a; put_u32(b, s[1] + 7, (uint32_t)(s[3] - s[1] - 15)); check("psize_swallows_next", b, true, t);
    b = a; b[s[2] + 15] ^= 1; check("first_payload_byte", b, true, t);
    b = a; b.insert(b.begin() + (ptrdiff_t)s[2], 37, (uint8_t)0x5A); CHECK(check("inserted_37", b, true, t) == 5, "inserted_37");
    b = a; b[s[1]] ^= 1; b[s[2] + 1] ^= 1; CHECK(check("two_lost", b, true, t) == 3, "two_lost");
    b = a; b[2] ^= 1; CHECK(check("first_lost", b, true, t) == 4, "first_lost");
    b.assign(a.begin(), a.begin() + 14); CHECK(check("fourteen_bytes", b, true, t) == 0, "fourteen_bytes");
    const Bytes decoy = frame(Bytes(), MiB, 100);
    b = a; b[s[2]] ^= 1; memcpy(b.data() + s[2] + 15, decoy.data(), 15); CHECK(check("decoy_in_lost_payload", b, true, t) == 4, "decoy_in_lost_payload");
    { std::vector<Bytes> p = {f[0], f[1]}; for (int i = 0; i < 40; i++) p.push_back(decoy); p.push_back(f[2]); p.push_back(f[3]); CHECK(check("decoy_flood", cat(p), true, t) == 4, "decoy_flood"); }
    // a decoy whose payload passes the chunk walk is a frame of the walk; the decode behind it (not this program's) turns it into a gap
    b = a; b[s[3]] ^= 1;
    { const Bytes d = frame(payload(1, 700u, 0), MiB); CHECK(d.size() + 15 < f[3].size(), "the decoy fits"); memcpy(b.data() + s[3] + 15, d.data(), d.size()); }
    CHECK(check("decoy_that_walks", b, true, t) == 5, "decoy_that_walks");
}

void random_archives(Tally *t)
{
    std::mt19937 rng(20261021u);
    auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const int32_t bounds[] = {0, 1, -1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1000 << 20) - 1, 1000 << 20, (1000 << 20) + 1, (1 << 30) | (1 << 20), (1 << 30) | ((1 << 20) - 1),
                              (int32_t)0x80100000u, (int32_t)0xC0100000u, 0x7FFFFFFF};
    const int64_t edges[] = {MiB - 1, MiB, (int64_t)MiB + 1, CAP - 1, CAP, CAP + 1, CAP + 2};
    for (int it = 0; it < 800; it++) {
        Bytes a;
        const int parts = 1 + (int)pick(6);
        for (int p = 0; p < parts; p++) {
            switch (pick(8)) {
            case 0: case 1: case 2: {  // a good frame
                a = cat({a, frame(payload(1 + (int)pick(2), 480u + pick(3000), (uint8_t)pick(256)), 1 << 20)});
                break;
            }
            case 3: {                  // "JAM"-dense junk
                const int n = (int)pick(60);
                for (int i = 0; i < n; i++) a.push_back((uint8_t)"JAMJA"[pick(5)]);
                break;
            }
            case 4: {                  // a header with fields around the bounds (staged bits among them), then some bytes
                Bytes h = frame(Bytes(), bounds[pick(14)]);
                put_u32(h, 7, pick(3) ? (uint32_t)pick(40) : (uint32_t)bounds[pick(14)]);
                a = cat({a, h, Bytes(pick(40), (uint8_t)0x80)});
                break;
            }
            case 5: {                  // a good frame with a damaged byte
                Bytes f = frame(payload(1, 480u + pick(2000), 3), 1 << 20);
                f[pick((uint32_t)f.size())] ^= (uint8_t)(1u << pick(8));
                a = cat({a, f});
                break;
            }
            case 6: {                  // a frame that declares a size around BlockSize and the cap; sometimes with a staged header
                a = cat({a, frame(payload_of(edges[pick(7)] + JPK_TRAILER_BYTES, (uint8_t)pick(256)), (1 << 20) | (pick(5) == 0 ? (1 << 30) : 0))});
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
        check(name, a, true, t);
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
