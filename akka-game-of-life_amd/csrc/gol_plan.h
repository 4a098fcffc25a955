// gol_plan.h -- the schedule of a pass as pure functions of plain integers:
// the band plan of one launch (band height, the small-board cut, the tail
// split, rows and bands per range, grid size), the XCD chunk and the depth
// planner.  Standard library only -- no HIP, no context, no environment -- so
// tests/schedule_probe.cpp checks it with a plain host compiler
// (tests/test_schedule_model.py).  gol_schedule.cpp gathers the inputs from a
// context and the environment.  Automatic tuning (scripts/tune.py sweeps on
// MI355X, profiles/r01_* .. r06_*): results never depend on these choices.
// DESIGN.md section 4.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace golplan {

// Deepest pass the cost table covers: gol::kMaxGensPerPass (gol_schedule.cpp
// asserts they agree).
constexpr int kMaxGens = 12;

constexpr int kDefaultXcdChunk = 8;

// Blocks per XCD chunk of the step kernels' block order (gol_stencil.h
// xcd_block).  `env_chunk`: the GOL_XCD_CHUNK override (A/B experiments; 1 =
// dispatch order), 0 when not set.
// Multi-generation passes: kDefaultXcdChunk.  Single-generation passes (the
// 6-row band paths, whose seams are read by two bands at about the same time):
// four bands' blocks per XCD, so three of every four band seams stay in one
// XCD's L2.  Same-box sweep (profiles/r03_g1_xcd_chunk.txt, HBM fraction by
// kernel time, chunk 8 / 16 / 32 / 64): 262144^2 (8 blocks per band) 0.76-0.78
// / 0.79-0.80 / 0.80 / 0.75-0.77, 65536^2 (2 blocks per band) 0.75 / 0.75 /
// 0.73-0.75 / 0.72.
inline int xcd_chunk(int gens, int strips, int env_chunk, int waves_per_wg) {
    if (env_chunk) return env_chunk;
    if (gens != 1) return kDefaultXcdChunk;
    const int blocks_per_band = (strips + waves_per_wg - 1) / waves_per_wg;
    return std::min(64, std::max(kDefaultXcdChunk, 4 * blocks_per_band));
}

// `band_rows`: the fixed band of the tuning (0: automatic).
// `resident`: waves the whole GPU holds at once for this kernel (0: unknown).
inline int pick_band(int band_rows, int64_t rows, int strips, int gens, int64_t resident) {
    if (band_rows > 0) return band_rows;
    // Single-generation passes: 6-row bands -- short streams, many in
    // flight, each band's 8 rows issued at once by step_kernel's straight-line
    // band path; the band seams (2 halo rows per 6) hit the caches.  Same-box
    // sweep with the band paths (profiles/r03_g1_band_heights.txt, HBM
    // fraction by kernel time, bands 4 / 6 / 8): 262144^2 0.738 / 0.774 /
    // 0.755, x 32768 0.734 / 0.762 / 0.749, 65536^2 0.752 / 0.760 / 0.753
    // (round 2, ring loop only: 4 rows best, profiles/r02_g1_band_sweep.txt).
    if (gens == 1) return 6;
    // Multi-generation passes recompute 2G halo rows per band: keep bands
    // >= 64 rows, aim at ~8192 waves, cap at 256 rows.
    const int64_t bands = std::max<int64_t>(1, 8192 / std::max(1, strips));
    int64_t band = (rows + bands - 1) / bands;
    band = std::max<int64_t>(band, 64);
    band = std::min<int64_t>(band, 256);
    // Wave quantization on wide boards: when a pass is only a few rounds of
    // resident waves, the last round is partly empty.  Model a pass as
    // ceil(waves / resident) rounds of (band + 2G) stream rows and shrink the
    // band (down to 60 %) when that fills the rounds better.  Measured on
    // the N = 8 per-rank shape (262144 x 32768, 1.7 rounds at band 256):
    // band 216 1.5-10 % faster on two boxes; with more rounds the effect is
    // within box-to-box noise (profiles/r01_band_quantization.txt).  Narrow
    // boards (< 32 strips) keep the plain choice (the model mispredicts 65536^2).
    // Narrow boards at 7- and 8-generation passes (4 waves per SIMD): 256-row
    // bands with the tail split below.  Same-box sweep at 65536^2, G = 8
    // (profiles/r02_band_sweep.txt): 0.0384 ms per generation vs 0.0405 for
    // the plain choice (137 rows, no tail) and 0.0471 for 256 rows without
    // the tail; at G = 6 the plain choice stays best.
    if (strips < 32 && gens >= 7 && resident > 0) return (int)std::min<int64_t>(256, std::max<int64_t>(rows, 1));
    // Wide boards at 7- to 12-generation passes, when the pass is many rounds
    // of resident waves: the tallest band (up to 1024 rows at G >= 10, 768
    // below) that still leaves >= 3.5 rounds, the tail split evening out the
    // end.  A band of B rows recomputes ~(G - 1) / B of its stage rows as
    // halo, so taller bands issue fewer VALU per cell.  Same-box sweep on the
    // bench's window (profiles/r03_band_262144.txt, 5 rounds, 262144^2,
    // passes 12 + 8): 1024 + 768 116.1k, 768 + 512 115.9k, 576 + 384 115.5k,
    // the previous 384 + ~256 114.4k GCUPS; on the N = 8 per-rank shape
    // (262144 x 32768, < 2 rounds) taller bands lost up to 6 %
    // (profiles/r03_band_32768.txt), so it keeps the rules below.
    if (strips >= 32 && gens >= 7 && resident > 0) {
        const int cap = gens >= 10 ? 1024 : 768;
        for (const int b : {1024, 768, 512}) {
            if (b > cap) continue;
            const int64_t waves = (rows + b - 1) / b * strips;
            if (2 * waves >= 7 * resident) return (int)std::min<int64_t>(b, std::max<int64_t>(rows, 1));
        }
    }
    // Wide boards at 10- to 12-generation passes (3 waves per SIMD, 2G halo
    // rows per band): 384-row bands when that is still >= 3 rounds of
    // resident waves, else 256, both with the tail split.  Same-box sweep at
    // G = 12 (profiles/r02_deep_band_sweep.txt, 4 rounds, ms per generation):
    // 262144^2 0.5660 (384) vs 0.5821 (the plain choice), x 131072 0.2882 vs
    // 0.2926, x 65536 0.1464 vs 0.1483, x 32768 0.0745 (256) vs 0.0761.
    if (strips >= 32 && gens >= 10 && resident > 0) {
        const int64_t waves384 = (rows + 383) / 384 * strips;
        return (int)std::min<int64_t>(waves384 >= 3 * resident ? 384 : 256, std::max<int64_t>(rows, 1));
    }
    if (resident > 0 && strips >= 32) {
        auto cost = [&](int64_t b) -> double {
            const int64_t waves = (rows + b - 1) / b * strips;
            return (double)((waves + resident - 1) / resident) * (double)(b + 2 * gens);
        };
        const int64_t full = (rows + band - 1) / band * strips;
        if (full >= resident && full <= 3 * resident) {
            int64_t best = band;
            double best_cost = cost(band);
            for (int64_t b = band - 1; b >= std::max<int64_t>(64, band * 6 / 10); --b) {
                const double c = cost(b);
                if (c < best_cost * 0.99) {
                    best = b;
                    best_cost = c;
                }
            }
            band = best;
        }
    }
    return (int)band;
}

// Small boards (round 6).  The rules above were measured on boards of
// >= 65536 columns and rows, where a pass is at least one round of resident
// waves.  On a small board they leave the GPU nearly empty -- a 4096^2 pass
// of G = 10 in 256-row bands is 2 strips x 16 bands = 32 waves, each
// streaming 276 rows through 10 stages one dependent instruction after the
// other (14.4 us per generation).  When the chosen band gives fewer waves than
// the GPU holds at once, the band is cut to about 1.5 rounds of resident waves
// (rows x strips / (1.5 resident), a multiple of 4, >= 4 rows), trading the
// taller bands' smaller halo share for parallelism.  Same-box sweep of depth x
// band (scripts/small_sweep.py, profiles/r06_small_sweep.txt, us per
// generation, unhashed): 4096^2 14.4 -> 2.3 at G = 10 in 4-row bands, 8192^2
// 14.4 -> 3.1-3.3, 16384^2 14.3 -> 5.3, 32768^2 18.1 -> 11.9; G = 10 stays the
// best depth (or within 3 % of it) at every size, hashed or not, so the
// planner plans hashed passes on these boards with the unhashed cost row
// (gol_schedule.cpp small_board).  Returns the band, or 0 when the board fills
// the GPU (the rules above stand).
inline int small_board_band(int band_rows, int64_t rows, int strips, int gens, int band, int64_t resident) {
    if (band_rows > 0 || gens <= 1 || resident <= 0 || strips <= 0 || band <= 0) return 0;
    const int64_t waves = (rows + band - 1) / band * strips;
    if (waves >= resident) return 0;
    int64_t b = (2 * rows * strips + 3 * resident - 1) / (3 * resident);
    b = std::max<int64_t>((b + 3) / 4 * 4, 4);
    return (int)std::min<int64_t>(b, band);
}

// Tail split of a pass's rows (DESIGN.md §4 "Band schedule").  The
// dispatcher hands workgroups to CUs as slots free up, so a pass of a few
// rounds of resident waves ends with uneven per-SIMD tails: the CUs that got
// the last full-height bands finish late.  The last `frac` x resident waves
// therefore cover their rows in bands of band / div, dispatched after the
// bulk.  Default: one resident round's worth of waves in bands of band / 4
// for tall (>= 768-row) bands, band / 6 below.  Round 1 chose band / 3
// (profiles/r01_tail_sweep.txt: +4 % on the N = 8 per-rank shape 262144 x
// 32768, +2 % at x 65536, +1 % at x 131072 and 262144^2).  Round 6 re-swept
// the divisor on the paired G = 10 kernels, scored per probed GHz
// (scripts/band_scan.py, profiles/r06_tail/; tail1_* and tail2_* against /3,
// tail3_* against /4).  /4 over /3: 262144^2 (1024-row bands) +1.6 %, hashed
// +1.8 %; 65536^2 (256) +4.0 %; 262144^2 at G = 12 -0.3 %.  /6 over /4:
// 131072^2 (384) +2.4 %, 262144 x 32768 (256) +2.4 %, hashed +2.9 %,
// 262144 x 65536 (384) +0.2 %, 65536^2 -0.1 %, 262144^2 -3.6 %.
// GOL_TAIL="frac,div" overrides it (A/B sweeps); frac 0 disables it.
struct TailSplit {
    int32_t rows = 0;  // rows at the end of the range in short bands (0: none)
    int32_t band = 0;
};

// The GOL_TAIL override as gol_schedule.cpp parsed it.
struct TailOverride {
    bool present = false;  // the variable exists, even empty: narrow boards below G = 7 split too
    bool set = false;      // ... and is not empty: frac and div replace the defaults (malformed: frac 0)
    double frac = 0.0;
    int div = 0;
};

constexpr double kTailFrac = 1.0;
constexpr int kTailDiv = 6;
constexpr int kTailDivTall = 4;  // bands of >= kTailTallBand rows
constexpr int kTailTallBand = 768;

inline TailSplit tail_split(int band_rows, int64_t rows, int strips, int band, int64_t resident, int gens,
                            const TailOverride& env) {
    double frac = kTailFrac;
    int div = band >= kTailTallBand ? kTailDivTall : kTailDiv;
    if (env.set) {
        frac = env.frac;
        div = env.div;
    } else if (band_rows > 0) {
        return {};  // a fixed band (tuning) is taken literally
    }
    TailSplit t;
    // narrow boards (< 32 strips, e.g. 65536^2 with 17) measured neutral to
    // -3.6 % at G = 6 (profiles/r01_tail_sweep.txt, r01_band_sweep.txt): off
    // unless forced; at G >= 7 they take 256-row bands (pick_band), which need it
    if (frac <= 0.0 || div < 2 || resident <= 0 || strips <= 0 || (!env.present && strips < 32 && gens < 7)) return t;
    const int64_t waves = (rows + band - 1) / band * strips;
    if (waves <= resident) return t;  // a single round: nothing to even out
    const int b2 = std::max(8, band / div);
    int64_t trows = (int64_t)(frac * (double)resident / strips) * b2;
    trows = std::min<int64_t>(trows, rows / 2) / b2 * b2;
    if (trows <= 0) return t;
    t.rows = (int32_t)trows;
    t.band = b2;
    return t;
}

// How one launch cuts its rows up: what the step kernels read from
// gol::StepParams (row_lo, row_hi, band, nbands), the waves and the grid.
struct BandPlan {
    int32_t row_lo[2] = {0, 0}, row_hi[2] = {0, 0};
    int32_t band[2] = {0, 0}, nbands[2] = {0, 0};
    int64_t waves = 0;   // strips x bands over both ranges
    int grid = 0;        // workgroups: ceil(waves / waves_per_wg)
    bool small = false;  // the small-board cut applied
};

// The band plan of a launch of `gens` generations over `n` (1 or 2) row ranges
// [lo[i], hi[i]) of `strips` column strips.  Two ranges (the boundary blocks
// of a sharded pass) share one band, picked for the longer of them without
// the occupancy-based rules; a single range of a multi-generation pass takes
// them (`resident`), then the small-board cut or the tail split.  `tail_env()`
// returns the TailOverride; it is called only where a tail split is
// considered, so a caller that reads the environment there reads it for
// those launches alone.
template <class TailEnv>
BandPlan band_plan(int n, const int32_t* lo, const int32_t* hi, int strips, int gens, int64_t resident, int band_rows,
                   TailEnv&& tail_env, int waves_per_wg) {
    BandPlan bp;
    int64_t maxlen = 0;
    for (int i = 0; i < n; ++i) maxlen = std::max<int64_t>(maxlen, hi[i] - lo[i]);
    if (n != 1 || gens <= 1) resident = 0;
    int band = pick_band(band_rows, maxlen, strips, gens, resident);
    const int small = n == 1 ? small_board_band(band_rows, maxlen, strips, gens, band, resident) : 0;
    if (small > 0) band = small;
    bp.small = small > 0;
    bp.band[0] = bp.band[1] = band;
    int nr = n;
    for (int i = 0; i < n; ++i) {
        bp.row_lo[i] = lo[i];
        bp.row_hi[i] = hi[i];
    }
    if (n == 1 && gens > 1 && small == 0) {  // a small board's pass is ~1.5 rounds: no tail to even out
        const TailSplit t = tail_split(band_rows, hi[0] - lo[0], strips, band, resident, gens, tail_env());
        if (t.rows > 0) {  // bulk [lo, hi - t.rows) in `band` rows, tail in t.band rows
            nr = 2;
            bp.row_hi[0] = hi[0] - t.rows;
            bp.row_lo[1] = bp.row_hi[0];
            bp.row_hi[1] = hi[0];
            bp.band[1] = t.band;
        }
    }
    for (int i = 0; i < 2; ++i) {
        bp.nbands[i] = i < nr ? (bp.row_hi[i] - bp.row_lo[i] + bp.band[i] - 1) / bp.band[i] : 0;
        bp.waves += (int64_t)bp.nbands[i] * strips;
    }
    bp.grid = (int)((bp.waves + waves_per_wg - 1) / waves_per_wg);
    return bp;
}

// Pass planner (DESIGN.md section 4 "Pass planner").  Relative time of one
// pass of G generations (G = 1..12, G = 6 -> 1), from scripts/depth_sweep.py
// (min of 3 rounds, reseeded board) on the row-pair-shared B3/S23 kernels
// (profiles/r04_pair_depth_sweep.txt; round 4).  Up to G = 6 a pass costs
// about the same (the sweep over the plane is HBM-bound); deeper passes cost
// more but less per generation.  The paired kernels hold 3 waves per SIMD up
// to G = 10 and 2 at G = 11 and 12 (rings of 174-197 VGPRs), so G = 10 is the
// cheapest per generation on both wide (>= 32 column strips) and narrow
// boards, unhashed and hashed, except narrow hashed boards where G = 7 ties it.
// Earlier rounds' per-row circuit tables: profiles/r01_depth_sweep.txt,
// r02_depth_sweep_deep.txt, r02_hash_deep_ab.txt.
constexpr double kPassCost[2][2][kMaxGens + 1] = {
    // [hashed][wide]; G = 0 .. 12
    {{0, 0.755, 0.984, 0.995, 0.987, 0.964, 1.00, 1.068, 1.274, 1.346, 1.459, 1.893, 2.022},   // narrow (65536^2)
     {0, 0.739, 1.084, 1.088, 1.045, 1.020, 1.00, 1.073, 1.223, 1.340, 1.446, 1.696, 1.809}},  // wide (262144^2)
    {{0, 0.642, 0.846, 0.859, 0.880, 0.894, 1.00, 1.077, 1.353, 1.449, 1.553, 2.109, 2.256},   // narrow, hashed
     {0, 0.615, 0.904, 0.908, 0.883, 0.861, 1.00, 1.084, 1.278, 1.382, 1.496, 1.806, 1.941}}}; // wide, hashed

// Depths of the passes that advance `n` generations, none deeper than `cap`
// (<= kMaxGens).  A fixed depth (`fixed_depth` > 0, the tuning's
// gens_per_pass; `cap` is it or less) is taken literally (the last pass
// shorter); otherwise the plan minimises the summed pass cost of the
// [hashed_row][wide] table row (a DP over n, n <= 1024: callers plan per
// chunk), deepest passes first (12 + 8 ran 3 % faster than 8 + 12 from the
// bench's fresh board with the per-row circuit, profiles/r02_plan_mix_ab.txt).
inline std::vector<int> plan_depths(uint32_t n, int cap, int fixed_depth, bool hashed_row, bool wide) {
    std::vector<int> plan;
    if (fixed_depth > 0 || cap == 1) {
        for (uint32_t g = 0; g < n; g += plan.back()) plan.push_back((int)std::min<uint32_t>(cap, n - g));
        return plan;
    }
    const double* cost = kPassCost[hashed_row ? 1 : 0][wide ? 1 : 0];
    std::vector<double> best(n + 1, 0.0);
    std::vector<int> pick(n + 1, 1);
    for (uint32_t m = 1; m <= n; ++m) {
        best[m] = 1e300;
        for (int G = 1; G <= cap && (uint32_t)G <= m; ++G) {
            const double c = best[m - G] + cost[G];
            if (c < best[m] - 1e-12) {
                best[m] = c;
                pick[m] = G;
            }
        }
    }
    for (uint32_t m = n; m > 0; m -= (uint32_t)pick[m]) plan.push_back(pick[m]);
    std::sort(plan.begin(), plan.end(), std::greater<int>());
    return plan;
}

}  // namespace golplan
