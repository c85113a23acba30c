// jam_update_plan.hpp -- what an update of a .jam archive (jpk_dev_jam_update / jpk_jam_update; DESIGN 4.6, "Updating an archive") does to which
// frame, worked out on the host from the index's raw offsets and the writes alone, written once for both entries (jam_archive.hip) and a
// stand-alone program (tests/jam_update_plan_host.cpp) that compares it with a byte map under a sanitizer:
//   check     the argument verdict: every write inside [0, raw_len], the writes with len > 0 pairwise disjoint (end to end is allowed)
//   make      for every frame whether it is KEPT, WHOLE (the union of the writes covers every byte of it: it is not decoded) or PART (it is
//             decoded first); the pieces that overlay the sources onto the rewritten frames; the passes over the rewritten frames in index
//             order, each with the stretch of the output it ends -- the kept frames since the pass before, and its own
// Pure functions over the standard library: no HIP header, no ABI header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace jup {

enum : uint8_t { KEPT = 0, WHOLE = 1, PART = 2 };

// len bytes of write `write`, from its byte write_off on, become the bytes of frame `frame` from its byte frame_off on
struct Piece { int32_t write; int64_t write_off; int32_t frame; int64_t frame_off; int64_t len; };

// One pass: the rewritten frames rewritten[q0, q1), and the stretch of the output that its splice writes, frames [f0, f1) -- f0 is the
// f1 of the pass before (0 for the first one), f1 the frame behind the pass's last rewritten one, so a stretch holds the kept frames in
// front of and between its new ones.  The frames behind the last pass's f1 are all kept.
struct Pass { size_t q0, q1; int32_t f0, f1; };

struct Plan {
    std::vector<uint8_t> cls;            // per frame: KEPT, WHOLE or PART
    std::vector<int32_t> rewritten;      // the frames that are not KEPT, ascending
    std::vector<Piece> pieces;           // ascending in (frame, frame_off); piece_at[q] .. piece_at[q + 1] are those of rewritten[q]
    std::vector<size_t> piece_at;
    std::vector<Pass> passes;
    int32_t tail_f0 = 0;                 // frames [tail_f0, F) lie behind the last pass: kept, one run
};

// the limits of a pass: the same as the reader's and the writers' (jam_archive.hip: JPK_JAM_PASS_FRAMES, JAM_PASS_RAW)
struct Limits { size_t frames; uint64_t weight; };

// raw_off: F + 1 ascending entries from 0, raw_off[k] = the raw bytes in front of frame k, the last one raw_len.  True: the n writes are
// ones an update takes.  O(n log n), nothing is kept.
inline bool check(const std::vector<int64_t> &raw_off, int32_t n, const int64_t *off, const int64_t *len)
{
    if (raw_off.empty() || n < 0 || (n > 0 && (!off || !len))) return false;
    const int64_t raw_len = raw_off.back();
    std::vector<int32_t> by;
    for (int32_t r = 0; r < n; r++) {
        if (off[r] < 0 || len[r] < 0 || off[r] > raw_len || len[r] > raw_len - off[r]) return false;
        if (len[r] > 0) by.push_back(r);
    }
    std::sort(by.begin(), by.end(), [&](int32_t a, int32_t b) { return off[a] < off[b]; });
    for (size_t i = 1; i < by.size(); i++)
        if (off[by[i - 1]] + len[by[i - 1]] > off[by[i]]) return false;
    return true;
}

// The plan of writes that passed check().  weight[k] is what frame k weighs in a pass (a chained frame its BlockSize, a plain one its raw
// size: jam_weight).  A frame of 0 raw bytes is always KEPT; a write of 0 bytes touches nothing.
inline Plan make(const std::vector<int64_t> &raw_off, const std::vector<int64_t> &weight, int32_t n, const int64_t *off, const int64_t *len, Limits lim)
{
    const size_t F = raw_off.size() - 1;
    Plan p;
    p.cls.assign(F, KEPT);
    std::vector<int32_t> by;
    for (int32_t r = 0; r < n; r++) if (len[r] > 0) by.push_back(r);
    std::sort(by.begin(), by.end(), [&](int32_t a, int32_t b) { return off[a] < off[b]; });
    // the writes in ascending order and disjoint: their pieces come out ascending in (frame, frame_off)
    std::vector<int64_t> covered(F, 0);
    for (int32_t r : by) {
        const int64_t a = off[r], b = a + len[r];
        size_t f = (size_t)(std::upper_bound(raw_off.begin(), raw_off.end(), a) - raw_off.begin()) - 1;      // the frame that holds byte a
        for (; f < F && raw_off[f] < b; f++) {
            const int64_t lo = std::max(a, raw_off[f]), hi = std::min(b, raw_off[f + 1]);
            if (hi <= lo) continue;                                       // (a frame of 0 raw bytes)
            p.pieces.push_back(Piece{r, lo - a, (int32_t)f, lo - raw_off[f], hi - lo});
            covered[f] += hi - lo;
        }
    }
    p.piece_at.push_back(0);
    size_t at = 0;
    for (size_t f = 0; f < F; f++) {
        if (!covered[f]) continue;
        p.cls[f] = covered[f] == raw_off[f + 1] - raw_off[f] ? WHOLE : PART;
        p.rewritten.push_back((int32_t)f);
        while (at < p.pieces.size() && (size_t)p.pieces[at].frame == f) at++;
        p.piece_at.push_back(at);
    }
    // the passes: at most lim.frames rewritten frames and lim.weight of weight each, one frame at least
    int32_t f0 = 0;
    for (size_t q = 0; q < p.rewritten.size();) {
        size_t e = q;
        uint64_t sum = 0;
        while (e < p.rewritten.size() && e - q < lim.frames && (e == q || sum + (uint64_t)weight[(size_t)p.rewritten[e]] <= lim.weight))
            sum += (uint64_t)weight[(size_t)p.rewritten[e++]];
        const int32_t f1 = p.rewritten[e - 1] + 1;
        p.passes.push_back(Pass{q, e, f0, f1});
        f0 = f1;
        q = e;
    }
    p.tail_f0 = f0;
    return p;
}

}  // namespace jup
