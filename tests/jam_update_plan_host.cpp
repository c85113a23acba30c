// The plan of an archive update (jampack_amd/csrc/jam_update_plan.hpp) against a brute-force byte map: one owner per raw byte, one class per
// frame.  Stand-alone, header only, built with -fsanitize=address,undefined by tests/test_jam_update_plan_host.py and run directly.
// Prints "crafted <cases> refused <r>", "random 2000 all3 <a> multi <m> refused <r>" and "all-ok 0"; a mismatch prints a FAIL line.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../jampack_amd/csrc/jam_update_plan.hpp"

namespace {
int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { g_fail++; printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Case {
    std::vector<int64_t> sizes, weight;      // per frame: raw bytes, pass weight
    std::vector<int64_t> off, len;           // the writes
    jup::Limits lim{128, 4ull << 30};
};

struct Seen { bool refused = false, all3 = false, multi = false; size_t passes = 0; };

// the byte map: owner[b] = (write, offset in the write) of raw byte b, write -1: untouched.  False: the writes are refused
bool brute(const std::vector<int64_t> &ro, const Case &c, std::vector<std::pair<int32_t, int64_t>> &owner)
{
    const int64_t raw_len = ro.back();
    owner.assign((size_t)raw_len, {-1, 0});
    for (size_t r = 0; r < c.off.size(); r++) {
        if (c.off[r] < 0 || c.len[r] < 0 || c.off[r] > raw_len || c.len[r] > raw_len - c.off[r]) return false;
        for (int64_t b = 0; b < c.len[r]; b++) {
            if (owner[(size_t)(c.off[r] + b)].first >= 0) return false;
            owner[(size_t)(c.off[r] + b)] = {(int32_t)r, b};
        }
    }
    return true;
}

Seen run(const Case &c, const char *name)
{
    Seen s;
    const size_t F = c.sizes.size();
    std::vector<int64_t> ro(F + 1, 0);
    for (size_t k = 0; k < F; k++) ro[k + 1] = ro[k] + c.sizes[k];
    std::vector<std::pair<int32_t, int64_t>> owner;
    const bool want_ok = brute(ro, c, owner);
    const int32_t n = (int32_t)c.off.size();
    const bool ok = jup::check(ro, n, c.off.data(), c.len.data());
    EXPECT(ok == want_ok, "%s: verdict %d, the byte map says %d", name, (int)ok, (int)want_ok);
    s.refused = !want_ok;
    if (!ok || !want_ok) return s;
    const jup::Plan p = jup::make(ro, c.weight, n, c.off.data(), c.len.data(), c.lim);
    // classes, and the frames several writes cover together
    EXPECT(p.cls.size() == F, "%s: %zu classes", name, p.cls.size());
    bool has[3] = {false, false, false};
    std::vector<int32_t> rew;
    for (size_t k = 0; k < F && k < p.cls.size(); k++) {
        int64_t touched = 0;
        std::vector<int32_t> ws;
        for (int64_t b = ro[k]; b < ro[k + 1]; b++)
            if (owner[(size_t)b].first >= 0) { touched++; if (ws.empty() || ws.back() != owner[(size_t)b].first) ws.push_back(owner[(size_t)b].first); }
        const uint8_t want = touched == 0 ? jup::KEPT : touched == c.sizes[k] ? jup::WHOLE : jup::PART;
        EXPECT(p.cls[k] == want, "%s: frame %zu class %d, the byte map says %d", name, k, (int)p.cls[k], (int)want);
        has[want] = true;
        if (want != jup::KEPT) rew.push_back((int32_t)k);
        if (want == jup::WHOLE && ws.size() > 1) s.multi = true;
    }
    s.all3 = has[0] && has[1] && has[2];
    EXPECT(p.rewritten == rew, "%s: rewritten frames", name);
    // pieces: they rebuild the byte map, lie inside one frame and one write each, ascend, and piece_at cuts them by rewritten frame
    std::vector<std::pair<int32_t, int64_t>> got((size_t)ro.back(), {-1, 0});
    for (size_t i = 0; i < p.pieces.size(); i++) {
        const jup::Piece &pc = p.pieces[i];
        const bool in = pc.len > 0 && pc.write >= 0 && pc.write < n && pc.frame >= 0 && (size_t)pc.frame < F && pc.write_off >= 0 && pc.write_off + pc.len <= c.len[(size_t)pc.write] &&
                        pc.frame_off >= 0 && pc.frame_off + pc.len <= c.sizes[(size_t)pc.frame];
        EXPECT(in, "%s: piece %zu out of its frame or its write", name, i);
        if (!in) return s;
        if (i) {
            const jup::Piece &q = p.pieces[i - 1];
            EXPECT(q.frame < pc.frame || (q.frame == pc.frame && q.frame_off + q.len <= pc.frame_off), "%s: piece %zu not ascending", name, i);
        }
        for (int64_t b = 0; b < pc.len; b++) {
            auto &g = got[(size_t)(ro[(size_t)pc.frame] + pc.frame_off + b)];
            EXPECT(g.first < 0, "%s: piece %zu writes a byte twice", name, i);
            g = {pc.write, pc.write_off + b};
        }
    }
    EXPECT(got == owner, "%s: the pieces do not rebuild the byte map", name);
    EXPECT(p.piece_at.size() == rew.size() + 1 && p.piece_at.front() == 0 && p.piece_at.back() == p.pieces.size(), "%s: piece_at ends", name);
    for (size_t q = 0; q + 1 < p.piece_at.size() && q < rew.size(); q++) {
        EXPECT(p.piece_at[q] < p.piece_at[q + 1], "%s: rewritten frame %zu without a piece", name, q);
        for (size_t i = p.piece_at[q]; i < p.piece_at[q + 1] && i < p.pieces.size(); i++) EXPECT(p.pieces[i].frame == rew[q], "%s: piece %zu in the wrong frame", name, i);
    }
    // passes: they tile the rewritten frames in order, keep the limits, are as long as the limits allow, and their stretches tile [0, tail_f0)
    size_t q = 0;
    int32_t f = 0;
    for (size_t i = 0; i < p.passes.size(); i++) {
        const jup::Pass &ps = p.passes[i];
        EXPECT(ps.q0 == q && ps.q1 > ps.q0 && ps.q1 <= rew.size() && ps.f0 == f, "%s: pass %zu starts wrong", name, i);
        if (!(ps.q0 == q && ps.q1 > ps.q0 && ps.q1 <= rew.size())) return s;
        uint64_t sum = 0;
        for (size_t j = ps.q0; j < ps.q1; j++) sum += (uint64_t)c.weight[(size_t)rew[j]];
        EXPECT(ps.q1 - ps.q0 <= c.lim.frames && (ps.q1 - ps.q0 == 1 || sum <= c.lim.weight), "%s: pass %zu over its limits", name, i);
        if (ps.q1 < rew.size()) EXPECT(ps.q1 - ps.q0 == c.lim.frames || sum + (uint64_t)c.weight[(size_t)rew[ps.q1]] > c.lim.weight, "%s: pass %zu ends early", name, i);
        EXPECT(ps.f1 == rew[ps.q1 - 1] + 1, "%s: pass %zu stretch end", name, i);
        q = ps.q1;
        f = ps.f1;
    }
    EXPECT(q == rew.size() && p.tail_f0 == f, "%s: the passes leave frames out", name);
    for (size_t k = (size_t)p.tail_f0; k < F; k++) EXPECT(p.cls[k] == jup::KEPT, "%s: frame %zu behind the last pass is not kept", name, k);
    s.passes = p.passes.size();
    return s;
}

Case make_case(std::vector<int64_t> sizes, std::vector<std::pair<int64_t, int64_t>> w)
{
    Case c;
    c.sizes = sizes;
    c.weight = sizes;
    for (auto &x : w) { c.off.push_back(x.first); c.len.push_back(x.second); }
    return c;
}

void crafted()
{
    int cases = 0, refused = 0;
    auto go = [&](const char *name, const Case &c, bool want_refused, size_t want_passes = (size_t)-1) {
        const Seen s = run(c, name);
        cases++;
        refused += s.refused;
        EXPECT(s.refused == want_refused, "%s: refused %d", name, (int)s.refused);
        if (want_passes != (size_t)-1) EXPECT(s.passes == want_passes, "%s: %zu passes, not %zu", name, s.passes, want_passes);
    };
    go("empty_index", make_case({}, {}), false, 0);
    go("empty_index_zero_write", make_case({}, {{0, 0}}), false, 0);
    go("empty_index_write", make_case({}, {{0, 1}}), true);
    go("no_write", make_case({5, 7}, {}), false, 0);
    go("frames_of_0_and_1", make_case({0, 1, 0, 1, 0}, {{0, 1}}), false, 1);
    go("frames_of_0_and_1_both", make_case({0, 1, 0, 1, 0}, {{1, 1}, {0, 1}}), false, 1);
    go("frame_of_0_spanned", make_case({3, 0, 3}, {{2, 2}}), false, 1);
    go("tiled_by_2", make_case({4, 10, 4}, {{9, 5}, {4, 5}}), false, 1);
    go("tiled_by_3", make_case({4, 9, 4}, {{10, 3}, {4, 3}, {7, 3}}), false, 1);
    go("tiled_by_2_across_edges", make_case({4, 10, 4}, {{2, 7}, {9, 7}}), false, 1);
    go("one_short_of_the_edge", make_case({8, 8}, {{0, 7}}), false, 1);
    go("one_past_the_edge", make_case({8, 8}, {{0, 9}}), false, 1);
    go("starts_one_before_the_edge", make_case({8, 8}, {{7, 2}}), false, 1);
    go("zero_at_raw_len", make_case({8, 8}, {{16, 0}}), false, 0);
    go("ends_at_raw_len", make_case({8, 8}, {{15, 1}}), false, 1);
    go("one_at_raw_len", make_case({8, 8}, {{16, 1}}), true);
    go("past_raw_len", make_case({8, 8}, {{10, 7}}), true);
    go("negative_off", make_case({8, 8}, {{-1, 2}}), true);
    go("negative_len", make_case({8, 8}, {{3, -1}}), true);
    go("huge_len", make_case({8, 8}, {{1, INT64_MAX}}), true);
    go("zero_on_an_edge", make_case({8, 8}, {{8, 0}, {0, 0}}), false, 0);
    go("zero_inside_a_write", make_case({8, 8}, {{2, 5}, {4, 0}}), false, 1);
    go("overlap_by_one", make_case({8, 8}, {{2, 5}, {6, 4}}), true);
    go("end_to_end", make_case({8, 8}, {{2, 5}, {7, 4}}), false, 1);
    go("identical", make_case({8, 8}, {{2, 5}, {2, 5}}), true);
    go("contained", make_case({8, 8}, {{2, 9}, {4, 1}}), true);
    go("whole_archive", make_case({3, 0, 5, 1}, {{0, 9}}), false, 1);
    // pass edges by count: 129 and 257 rewritten frames of the default limits, a byte each
    for (int frames : {128, 129, 256, 257}) {
        Case c;
        for (int k = 0; k < frames + 3; k++) { c.sizes.push_back(2); c.weight.push_back(2); }
        for (int k = 0; k < frames; k++) { c.off.push_back(2 * (k + (k > 100 ? 2 : 0))); c.len.push_back(1); }      // two kept frames inside a pass
        go(("count_" + std::to_string(frames)).c_str(), c, false, (size_t)(frames + 127) / 128);
    }
    // a pass cut by weight: chained frames weigh their BlockSize whatever their raw size; one frame alone may exceed the limit
    {
        Case c = make_case({4, 4, 4, 4, 4}, {{0, 20}});
        c.weight = {1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30};
        go("weight_4_GiB", c, false, 2);
        c.weight = {(int64_t)3 << 30, (int64_t)3 << 30, 1, (int64_t)5 << 30, 1};
        go("weight_uneven", c, false, 4);
        c.lim = jup::Limits{2, 4ull << 30};
        c.weight = {1, 1, 1, 1, 1};
        go("count_2", c, false, 3);
    }
    printf("crafted %d refused %d\n", cases, refused);
}

void randoms()
{
    std::mt19937_64 rng(20240611);
    auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    int all3 = 0, multi = 0, refused = 0;
    for (int it = 0; it < 2000; it++) {
        Case c;
        const int F = (int)rnd(0, 12);
        for (int k = 0; k < F; k++) {
            c.sizes.push_back(rnd(0, 4) == 0 ? 0 : rnd(1, 30));
            c.weight.push_back(rnd(0, 1) ? c.sizes.back() : rnd(30, 64));
        }
        c.lim = jup::Limits{(size_t)rnd(1, 4), (uint64_t)rnd(1, 150)};
        std::vector<int64_t> ro(1, 0);
        for (int64_t s : c.sizes) ro.push_back(ro.back() + s);
        const int64_t raw_len = ro.back();
        std::vector<std::pair<int64_t, int64_t>> w;
        if (rnd(0, 4) == 0 && raw_len >= 2) {
            // disjoint intervals between sorted cut points, whatever frames they span
            std::vector<int64_t> cut;
            for (int i = 0, m = 2 * (int)rnd(1, 5); i < m; i++) cut.push_back(rnd(0, raw_len));
            std::sort(cut.begin(), cut.end());
            for (size_t i = 0; i + 1 < cut.size(); i += 2) if (cut[i + 1] > cut[i]) w.push_back({cut[i], cut[i + 1] - cut[i]});
        } else {
            // frame by frame: kept, tiled exactly by 1..3 writes, or partly covered
            for (int k = 0; k < F; k++) {
                const int64_t a = ro[(size_t)k], n = c.sizes[(size_t)k];
                const int how = (int)rnd(0, 9);
                if (n == 0 || how < 3) continue;
                if (how < 6 || n == 1) {
                    const int64_t parts = std::min<int64_t>(n, rnd(1, 3));
                    std::vector<int64_t> cut{0, n};
                    while ((int64_t)cut.size() < parts + 1) { const int64_t x = rnd(1, n - 1); if (std::find(cut.begin(), cut.end(), x) == cut.end()) cut.push_back(x); }
                    std::sort(cut.begin(), cut.end());
                    for (size_t i = 0; i + 1 < cut.size(); i++) w.push_back({a + cut[i], cut[i + 1] - cut[i]});
                } else {
                    const int64_t len = rnd(1, n - 1), o = rnd(0, n - len);
                    w.push_back({a + o, len});
                }
            }
        }
        for (int i = 0, m = (int)rnd(0, 2); i < m; i++) w.push_back({rnd(0, raw_len), 0});
        if (rnd(0, 11) == 0) {
            // a write that must be refused
            const int how = (int)rnd(0, 3);
            if (how == 0 && !w.empty() && w[0].second > 0) w.push_back(w[0]);
            else if (how == 1 && !w.empty() && w[0].second > 0) w.push_back({w[0].first + w[0].second - 1, 1});
            else if (how == 2) w.push_back({-rnd(1, 3), 1});
            else w.push_back({raw_len - rnd(0, std::min<int64_t>(raw_len, 2)), 3});
        }
        std::shuffle(w.begin(), w.end(), rng);
        for (auto &x : w) { c.off.push_back(x.first); c.len.push_back(x.second); }
        const Seen s = run(c, ("random_" + std::to_string(it)).c_str());
        all3 += s.all3; multi += s.multi; refused += s.refused;
    }
    printf("random 2000 all3 %d multi %d refused %d\n", all3, multi, refused);
}
}  // namespace

int main()
{
    crafted();
    randoms();
    printf("all-ok %d\n", g_fail);
    return g_fail ? 1 : 0;
}
