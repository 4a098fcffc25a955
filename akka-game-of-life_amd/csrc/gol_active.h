// gol_active.h -- active-row stepping as pure functions of plain integers:
// the rows of a plane that can hold a live cell as a short sorted list of
// disjoint runs [lo, hi), and the arithmetic a pass does with them (grow by
// the pass depth, what to clear in the destination plane, runs from the scan's
// block bitmap, when to scan, when to give up and step the whole plane).
// Standard library only -- no HIP, no context -- so tests/active_probe.cpp
// checks it with a plain host compiler (tests/test_active_model.py), and
// tests/find_probe.cpp the pattern search's anchor rows (tests/test_find_model.py).
// gol_ring.cpp's one_pass applies it.  Results never depend on these choices.
// DESIGN.md section 5c.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace golactive {

constexpr int32_t kActiveBlock = 64;  // runs start and end on multiples of it (or at `rows`)
constexpr int kMaxRuns = 8;           // runs kept per plane: more are merged across the smallest gaps
constexpr int kFirstBackoff = 4;      // passes between scans of a board that keeps scanning dense: the first wait,
constexpr int kMaxBackoff = 256;      // ... and the longest (each wait four times the last)

struct Run {
    int32_t lo, hi;  // local rows [lo, hi)
};
using Runs = std::vector<Run>;

inline int64_t row_count(const Runs& runs) {
    int64_t n = 0;
    for (const Run& r : runs) n += r.hi - r.lo;
    return n;
}

// Any runs inside [0, rows) as the invariant keeps them: block-aligned
// (clipped at `rows`), sorted, disjoint (touching runs merged) and at most
// kMaxRuns of them, the smallest gaps closed first.  A superset of the input.
inline Runs normalize(Runs runs, int32_t rows) {
    Runs in;
    for (Run r : runs) {
        r.lo = std::max<int32_t>(r.lo, 0);
        r.hi = std::min<int32_t>(r.hi, rows);
        if (r.lo >= r.hi) continue;
        r.lo = r.lo / kActiveBlock * kActiveBlock;
        r.hi = (int32_t)std::min<int64_t>(((int64_t)r.hi + kActiveBlock - 1) / kActiveBlock * kActiveBlock, rows);
        in.push_back(r);
    }
    std::sort(in.begin(), in.end(), [](const Run& a, const Run& b) { return a.lo < b.lo; });
    Runs out;
    for (const Run& r : in) {
        if (!out.empty() && r.lo <= out.back().hi)
            out.back().hi = std::max(out.back().hi, r.hi);
        else
            out.push_back(r);
    }
    while ((int)out.size() > kMaxRuns) {
        size_t best = 1;
        for (size_t k = 2; k < out.size(); ++k)
            if (out[k].lo - out[k - 1].hi < out[best].lo - out[best - 1].hi) best = k;
        out[best - 1].hi = out[best].hi;
        out.erase(out.begin() + (std::ptrdiff_t)best);
    }
    return out;
}

// The rows a pass of G generations must step and may write: every run grown
// by G rows on both sides -- clamped at the plane's ends on a clipped board,
// wrapped and split at the seam on a torus -- then normalized.
inline Runs dilate(const Runs& runs, int G, int32_t rows, bool wrap_y) {
    Runs grown;
    for (const Run& r : runs) {
        if (r.lo >= r.hi) continue;
        const int64_t lo = (int64_t)r.lo - G, hi = (int64_t)r.hi + G;
        if (!wrap_y) {
            grown.push_back({(int32_t)std::max<int64_t>(lo, 0), (int32_t)std::min<int64_t>(hi, rows)});
        } else if (hi - lo >= rows) {
            grown.push_back({0, rows});
        } else {
            grown.push_back({(int32_t)std::max<int64_t>(lo, 0), (int32_t)std::min<int64_t>(hi, rows)});
            if (lo < 0) grown.push_back({(int32_t)(lo + rows), rows});
            if (hi > rows) grown.push_back({0, (int32_t)(hi - rows)});
        }
    }
    return normalize(std::move(grown), rows);
}

// The rows of `a` that are not in `b` (both sorted and disjoint): what a pass
// clears in the destination plane.
inline Runs subtract(const Runs& a, const Runs& b) {
    Runs out;
    size_t j = 0;
    for (const Run& r : a) {
        int32_t lo = r.lo;
        while (j < b.size() && b[j].hi <= lo) ++j;
        for (size_t k = j; k < b.size() && b[k].lo < r.hi; ++k) {
            if (b[k].lo > lo) out.push_back({lo, b[k].lo});
            lo = std::max(lo, b[k].hi);
        }
        if (lo < r.hi) out.push_back({lo, r.hi});
    }
    return out;
}

// Pattern search (gol_find): the anchor rows at which a
// pattern `ph` rows tall can have a row inside `runs` -- every run grown
// upward by ph - 1 rows, clamped at row 0 on a clipped board, wrapped and
// split at the seam on a torus.  Sorted, disjoint, touching runs merged; exact
// to the row (not block-aligned, no cap: there are at most twice the input's).
inline Runs anchor_rows(const Runs& runs, int ph, int32_t rows, bool wrap_y) {
    Runs grown;
    for (const Run& r : runs) {
        const int64_t hi = std::min<int64_t>(r.hi, rows), lo = (int64_t)std::max<int32_t>(r.lo, 0) - (ph - 1);
        if (std::max<int32_t>(r.lo, 0) >= hi) continue;
        grown.push_back({(int32_t)std::max<int64_t>(lo, 0), (int32_t)hi});
        if (wrap_y && lo < 0) grown.push_back({(int32_t)std::max<int64_t>(lo + rows, 0), rows});
    }
    std::sort(grown.begin(), grown.end(), [](const Run& a, const Run& b) { return a.lo < b.lo; });
    Runs out;
    for (const Run& r : grown) {
        if (!out.empty() && r.lo <= out.back().hi)
            out.back().hi = std::max(out.back().hi, r.hi);
        else
            out.push_back(r);
    }
    return out;
}

// The rows of `a` inside [lo, hi) (a sorted and disjoint): the part of the
// anchor rows one run of owned window rows launches.
inline Runs clip(const Runs& a, int64_t lo, int64_t hi) {
    Runs out;
    for (const Run& r : a) {
        const int64_t l = std::max<int64_t>(r.lo, lo), h = std::min<int64_t>(r.hi, hi);
        if (l < h) out.push_back({(int32_t)l, (int32_t)h});
    }
    return out;
}

// Runs from the scan's bitmap: bit k of `bits` (32 per word) is block
// lo_block + k, k < n.  Normalized, so the last block is clipped at `rows`.
inline Runs from_bitmap(const uint32_t* bits, int32_t lo_block, int32_t n, int32_t rows) {
    Runs runs;
    for (int32_t k = 0; k < n; ++k) {
        if (!((bits[k >> 5] >> (k & 31)) & 1u)) continue;
        const int32_t lo = (lo_block + k) * kActiveBlock;
        if (!runs.empty() && runs.back().hi == lo)
            runs.back().hi = lo + kActiveBlock;
        else
            runs.push_back({lo, lo + kActiveBlock});
    }
    return normalize(std::move(runs), rows);
}

// Scan again once the runs have grown to twice what the last scan left, plus
// four blocks: a pattern that stays put is scanned every few passes, a board
// that fills up geometrically less often.
inline bool scan_due(int64_t rows_now, int64_t rows_at_last_scan) {
    return rows_now >= 2 * rows_at_last_scan + 4 * kActiveBlock;
}

// More than half the plane: the pass runs as one launch over every row.
inline bool dense(int64_t rows_launched, int64_t rows) { return rows_launched > rows / 2; }

// Passes to wait before the next scan after a scan left the pass dense: 4, 16,
// 64, 256, 256 ... while scans keep finding the board dense.  A scan of a
// dense board reads a whole plane and drains the stream: on a seeded 65536^2
// torus each costs about 0.14 ms next to 0.33 ms for a pass of 10 generations,
// and waits of 1, 2, 4 ... 64 put six of them into the first 60 passes (+4.3 %
// over 600 generations, where mode-off windows span 0.2-0.5 %).  With these
// waits a board seeded with the mode on runs +0.14 %, within that spread
// (scripts/active_bench.py, profiles/active_rows.txt).
inline int next_backoff(int backoff) {
    return backoff <= 0 ? kFirstBackoff : std::min(4 * backoff, kMaxBackoff);
}

}  // namespace golactive
