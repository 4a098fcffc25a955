// gol_soup.h -- the soups of a batch (include/gol.h gol_soup_batch*; DESIGN.md
// section 5l) as far as they need no device: the one validator, the raw bits,
// the symmetry groups as the steps the kernel applies, the fundamental domain
// and the host generator behind gol_soup_batch_rows.  No HIP header: plain
// C++ (tests/soup_probe.cpp compiles it alone); under hipcc the functions the
// kernel shares (mix, raw_row, steps) are device functions too.  Not installed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gol.h"

#if defined(__HIPCC__)
#define GOL_SOUP_FN __host__ __device__ inline
#else
#define GOL_SOUP_FN inline
#endif

namespace golsoup {

constexpr int32_t kMaxSide = 64;  // a stored board's width and height, so a window's

// gol_batch_seed's function of a counter (include/gol.h): splitmix64.
GOL_SOUP_FN uint64_t mix(uint64_t seed, uint64_t c) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (c + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Window row v of soup number `soup` before any symmetry: bit u is
// t(u) < density, t(u) the 8-bit value whose bit j is bit u of
// Z[j] = mix(seed, (soup * 64 + v) * 8 + j).  The comparator runs bit-sliced
// over the 64 columns from plane 0 upward.  All 64 bits are returned: the
// caller masks to the window's width.
GOL_SOUP_FN uint64_t raw_row(uint64_t seed, int32_t density, uint64_t soup, int32_t v) {
    const uint64_t c0 = (soup * 64ull + (uint64_t)(int64_t)v) * 8ull;
    uint64_t lt = 0ull;
    for (int j = 0; j < 8; ++j) {
        const uint64_t z = mix(seed, c0 + (uint64_t)j);
        lt = ((density >> j) & 1) ? (~z | lt) : (~z & lt);
    }
    return lt;
}

// A symmetry group as at most three steps, three bits each, the first step in
// the lowest bits and 0 where there is none.  A step maps a cell by T (u, v) ->
// (v, u), then X (u, v) -> (w - 1 - u, v), then Y (u, v) -> (u, h - 1 - v), each
// where its bit is set; the group is every product of a subset of the steps,
// taken in their order (C4: XY, then R = X T; D8: T, X, Y).  The kernel ORs an
// image per step, the host enumerates the subsets: one table for both.
constexpr uint32_t kStepT = 1u, kStepX = 2u, kStepY = 4u;
constexpr int kSteps = 3;
GOL_SOUP_FN uint32_t steps(int32_t symmetry) {
    switch (symmetry) {
        case GOL_SOUP_C2: return kStepX | kStepY;
        case GOL_SOUP_C4: return (kStepX | kStepY) | ((kStepT | kStepX) << 3);
        case GOL_SOUP_D2_X: return kStepX;
        case GOL_SOUP_D2_Y: return kStepY;
        case GOL_SOUP_D2_DIAG: return kStepT;
        case GOL_SOUP_D4_PLUS: return kStepX | (kStepY << 3);
        case GOL_SOUP_D4_DIAG: return kStepT | ((kStepX | kStepY) << 3);
        case GOL_SOUP_D8: return kStepT | (kStepX << 3) | (kStepY << 6);
        default: return 0u;  // GOL_SOUP_C1
    }
}
GOL_SOUP_FN bool needs_square(int32_t symmetry) {
    const uint32_t s = steps(symmetry);
    return ((s | (s >> 3) | (s >> 6)) & kStepT) != 0u;
}

// Whether boards [first, first + count) of a batch of `boards` boards of
// width x height stored cells can be given the soups of *s (null: fine), or
// the reason they are refused.  What gol_soup_batch_check reports and what
// gol_soup_batch, gol_soup_batch_rows and launch_batch_soup do first.
inline const char* soup_args(int32_t width, int32_t height, int32_t boards, const gol_soup_spec* s, int64_t first,
                             int64_t count) {
    if (!s) return "spec is null";
    if (s->w < 1 || s->h < 1) return "w and h must be at least 1";
    if (s->x < 0 || s->y < 0 || (int64_t)s->x + s->w > width || (int64_t)s->y + s->h > height)
        return "the window must lie inside the stored board (no wrap)";
    if (s->density < 1 || s->density > 255) return "density must be 1 .. 255";
    if (s->symmetry < GOL_SOUP_C1 || s->symmetry > GOL_SOUP_D8) return "unknown symmetry";
    if (needs_square(s->symmetry) && s->w != s->h) return "this symmetry needs a square window (w == h)";
    if (first < 0 || count < 1 || first >= boards || count > (int64_t)boards - first)
        return "boards [first, first + count) outside the batch";
    return nullptr;
}

// What a call needs of a (valid) spec beyond the raw bits: per window cell the
// member of its orbit with the smallest (v, u), and the fundamental domain --
// row v's mask of the cells that are that member themselves.  A function of
// the spec alone.
struct Plan {
    uint64_t domain[kMaxSide];
    uint8_t cu[kMaxSide][kMaxSide], cv[kMaxSide][kMaxSide];  // [v][u]
};
inline void make_plan(const gol_soup_spec& s, Plan* p) {
    const uint32_t st = steps(s.symmetry);
    for (int32_t v = 0; v < kMaxSide; ++v) p->domain[v] = 0ull;
    for (int32_t v = 0; v < s.h; ++v)
        for (int32_t u = 0; u < s.w; ++u) {
            int32_t bu = u, bv = v;
            for (uint32_t subset = 1; subset < (1u << kSteps); ++subset) {
                int32_t a = u, b = v;
                for (int k = 0; k < kSteps; ++k) {
                    const uint32_t g = (subset >> k) & 1u ? (st >> (3 * k)) & 7u : 0u;
                    if (g & kStepT) {
                        const int32_t t = a;
                        a = b;
                        b = t;
                    }
                    if (g & kStepX) a = s.w - 1 - a;
                    if (g & kStepY) b = s.h - 1 - b;
                }
                if (b < bv || (b == bv && a < bu)) {
                    bu = a;
                    bv = b;
                }
            }
            p->cu[v][u] = (uint8_t)bu;
            p->cv[v][u] = (uint8_t)bv;
            if (bu == u && bv == v) p->domain[v] |= 1ull << u;
        }
}

// The `height` rows of the board that holds soup number `soup`.
inline void board_rows(const gol_soup_spec& s, const Plan& p, int32_t height, uint64_t soup, uint64_t* rows) {
    uint64_t raw[kMaxSide];
    for (int32_t v = 0; v < s.h; ++v) raw[v] = raw_row(s.seed, s.density, soup, v);
    for (int32_t y = 0; y < height; ++y) rows[y] = 0ull;
    for (int32_t v = 0; v < s.h; ++v) {
        uint64_t r = 0ull;
        for (int32_t u = 0; u < s.w; ++u) r |= ((raw[p.cv[v][u]] >> p.cu[v][u]) & 1ull) << u;
        rows[s.y + v] = r << s.x;
    }
}

// Boards first .. first + count - 1 of a batch in its host layout
// ([count][height]): board b holds soup number index0 + b.  The arguments are
// the caller's to have validated (soup_args).
inline void batch_rows(const gol_soup_spec& s, int32_t height, int64_t first, int64_t count, uint64_t* rows_out) {
    Plan p;
    make_plan(s, &p);
    for (int64_t i = 0; i < count; ++i)
        board_rows(s, p, height, s.index0 + (uint64_t)(first + i), rows_out + (size_t)i * (size_t)height);
}

}  // namespace golsoup
