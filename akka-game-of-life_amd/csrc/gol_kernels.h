// gol_kernels.h -- internal interface between the C-ABI host layer
// (gol_capi.cpp and the units gol_ctx.h lists) and the gfx950 kernels
// (gol_stencil.h, gol_step.hip -- built once per pass depth --, gol_misc.hip,
// gol_region.hip, gol_find.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <type_traits>
#include <utility>

namespace gol {

constexpr int kWaveLanes = 64;   // CDNA wavefront
#ifndef GOL_WAVES_PER_WG
#define GOL_WAVES_PER_WG 4
#endif
constexpr int kWavesPerWG = GOL_WAVES_PER_WG;  // waves per workgroup (256-thread workgroups)
constexpr int kHashSlots = 64;   // sharded hash accumulators (one cache line each)
constexpr int kHashSlotStride = 8;  // u64 per slot => 64 B apart
constexpr int kHashGenStride = kHashSlots * kHashSlotStride;  // u64 per generation
constexpr int kPopSlotWord = 1;     // a slot's population count (series instances): the u64 after its hash sum
static_assert(kPopSlotWord < kHashSlotStride, "the population count shares the hash sum's line");
constexpr int kMaxGensPerPass = 12;  // temporal blocking depth supported by the kernels
// Deepest pass of the 16-byte-lane (words_per_lane = 4) generic-rule and
// clipped instances that keeps every variable in registers: deeper ones spill
// (448-640 B of scratch per lane), so they are not built (gol_stencil.h
// kBuilt) and gol_set_tuning / the planner never ask for them.
constexpr int kMaxGensVec4Generic = 7;

// State hash keys (oracle/gol_oracle.c
// oracle_hash_packed, oracle/oracle.py np_hash).  The hash is a function of
// the cells alone: the canonical words E (even columns) and O (odd columns)
// of column group g = columns 64g .. 64g + 63 of global row y contribute
// (E * A(y, 0) + O * A(y, 1)) * B(g) mod 2^64 -- on the pair layout exactly
// the device words, elsewhere their unzipped row-major words.
//   A(y, 0) = ((t ^ (t >> 15)) << 1) | 1,  t = y * kHashRowMul (mod 2^32)
//   A(y, 1) = A(y, 0) + kHashOddAdd        (even: stays odd)
//   B(g)    = murmur3 fmix32(g + kHashPairAdd) | 1
// Both keys odd, so a single-word change always changes the sum.
constexpr uint32_t kHashRowMul = 0x9E3779B1u;
constexpr uint32_t kHashOddAdd = 0x6A09E666u;
constexpr uint32_t kHashPairAdd = 0x7F4A7C15u;

// Launch `kernel` and return the status of this launch alone.
// hipLaunchKernel returns it directly; hipGetLastError() after a
// triple-chevron launch would instead report -- and clear -- whatever status
// an earlier call of this thread left pending (DESIGN.md section 2 "HIP
// status discipline").  The arguments are converted to the kernel's parameter
// types first, as a direct call would.
template <typename... KArgs, typename... Args>
hipError_t launch_kernel(void (*kernel)(KArgs...), dim3 grid, dim3 block, hipStream_t stream, Args&&... args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "kernel argument count");
    std::tuple<std::remove_cv_t<KArgs>...> vals(std::forward<Args>(args)...);
    return std::apply(
        [&](auto&... v) {
            void* argv[] = {static_cast<void*>(&v)...};
            return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, argv, 0, stream);
        },
        vals);
}

__host__ __device__ __forceinline__ uint32_t hash_row_key(int64_t y) {
    const uint32_t t = (uint32_t)y * kHashRowMul;
    return ((t ^ (t >> 15)) << 1) | 1u;
}

__host__ __device__ __forceinline__ uint32_t hash_pair_key(uint32_t k) {
    uint32_t h = k + kHashPairAdd;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h | 1u;
}

// One launch advances G generations (G = `gens`, 1..kMaxGensPerPass) over up
// to two local row ranges, each cut into bands of its own height: the whole
// shard (one range, or a bulk range plus a tail of shorter bands), or the two
// boundary row blocks of a sharded pass.  Waves are numbered range 0's bands
// first, then range 1's (the order the dispatcher hands them out).
struct StepParams {
    const uint32_t* cur;       // local row 0 of the current plane
    uint32_t* nxt;             // local row 0 of the next plane
    const uint32_t* halo_top;  // rows -G .. -1 (halo_stride apart)
    const uint32_t* halo_bot;  // rows rows .. rows+G-1
    unsigned long long* hash_slots;  // G * kHashGenStride u64 (hash sums, population counts), or null
    int64_t pitch;             // words between rows (multiple of 64)
    int64_t grow0;             // global row of local row 0
    int64_t vis_rows;          // global rows [0, vis_rows) are visible (clipped)
    int64_t vis_cols;          // columns [0, vis_cols) are visible (clipped)
    int64_t width;             // cells per row
    int32_t wwords;            // words per row = ceil(width / 32)
    int32_t rows;              // local rows
    int32_t row_lo[2];
    int32_t row_hi[2];
    int32_t nbands[2];
    int32_t band[2];           // output rows streamed by one wave, per range
    int32_t strips;            // column strips per row
    int32_t wrap_x;            // torus in x
    int32_t wrap_y;            // unsharded torus: local rows wrap modulo `rows`
    int64_t halo_stride;       // words between halo rows (0: one row repeated)
    uint32_t birth;
    uint32_t survive;
    int32_t xcd_chunk;         // consecutive blocks kept on one XCD (gol_stencil.h xcd_block; <= 1: off)
    unsigned long long* clk;   // launch clock probe slot (kClockSlotWords u64), or null (gol_stencil.h clock_probe_*)
};

using StepKernel = void (*)(StepParams);  // every step kernel's type

// Per launch: kClockSubSlots sub-slots one 64-B line apart, each summing
// core-clock ticks and 100 MHz reference ticks of the sampled workgroups.
constexpr int kClockSubSlots = 64;
constexpr int kClockSubWords = 8;
constexpr int kClockSampleEvery = 4;
constexpr int kClockSlotWords = kClockSubSlots * kClockSubWords;

// Whole-row waves: a B3/S23 torus in the pair layout whose row is exactly one
// wave of 2-word lanes (64 pairs, 4096 columns -- BASELINE.json configs[1])
// runs its kWholeRowGens-deep passes as one strip without halo lanes: the
// lane-edge words come from a wave rotate, so every lane is an output lane
// and the row takes one wave per band instead of two (62 + 2 pairs).
constexpr int kWholeRowGens = 10;
constexpr int kWholeRowVec = 2;
inline bool whole_row_fits(int vec, int gens, bool life, bool clipped, int ilv, bool torus, int64_t wwords) {
    return torus && life && !clipped && ilv == 2 && vec == kWholeRowVec && gens == kWholeRowGens &&
           wwords == (int64_t)kWaveLanes * kWholeRowVec;
}

// The step kernel instance of a pass.  vec: words per lane (1, 2 or 4); gens:
// generations per pass; ilv: the plane's interleave (1 row-major, 2 pairs; vec
// a multiple of it); life: B3/S23 fast path (torus only); hash: fuse the
// per-generation state hash; clipped: reference geometry; whole_row: one strip
// is the whole torus row (whole_row_fits); pop: fuse the per-generation
// population count (with or without the hash; the population-series instances,
// kernels of their own).  Multi-generation passes at
// vec <= 2 run the horizontal-first kernel, at vec = 4 the vertical-first one.
struct StepInstance {
    int vec, gens, ilv;
    bool life, hash, clipped, whole_row;
    bool pop;
};

// Strip geometry of a launch: words covered per wave (multi-generation strips
// keep one halo lane per side, whole-row waves none).
inline int strip_words(const StepInstance& k) {
    return (k.gens == 1 || k.whole_row ? kWaveLanes : kWaveLanes - 2) * k.vec;
}

// hipErrorInvalidValue for an instance that is not built.
hipError_t launch_step(const StepParams& p, const StepInstance& k, int grid_x, int grid_y, hipStream_t stream);

// Resident 256-thread workgroups per CU of the instance
// (hipOccupancyMaxActiveBlocksPerMultiprocessor); 0 if unknown or not built.
int resident_blocks_per_cu(const StepInstance& k);

// Seeded board in the device layout (ilv: words per interleave group).
hipError_t launch_seed(uint32_t* plane, int64_t pitch, int32_t wwords, int64_t width,
                       int64_t grow0, int32_t rows, uint64_t seed, int ilv, hipStream_t stream);

// Row-major words <-> pair-interleaved words (ilv 2), `rows` rows of `wwords`
// (even) words, `pitch` words apart in the source and `dst_pitch` (<= 0:
// `pitch`) in the destination (src != dst).
hipError_t launch_convert(const uint32_t* src, uint32_t* dst, int64_t pitch, int32_t wwords, int32_t rows,
                          bool to_device, int ilv, hipStream_t stream, int64_t dst_pitch = 0);

// Partial state hash of `rows` device rows of interleave `ilv` (1 or 2).
hipError_t launch_hash(const uint32_t* plane, int64_t pitch, int32_t wwords, int64_t grow0,
                       int32_t rows, int ilv, unsigned long long* slots, hipStream_t stream);

// folded[g] = sum of generation g's hash accumulators, g < gens, which it
// clears; `folded` may be mapped host memory (8 bytes per generation cross
// PCIe instead of the 4 KiB of accumulators).
hipError_t launch_fold(unsigned long long* slots, uint32_t gens, unsigned long long* folded, hipStream_t stream);
// The same after passes of the population-series instances: folded[g] the
// hash sum and folded_pop[g] the population of generation g; both words of
// every slot are cleared.
hipError_t launch_fold_series(unsigned long long* slots, uint32_t gens, unsigned long long* folded,
                              unsigned long long* folded_pop, hipStream_t stream);

// DPP / lane-shift self test: out[64*4] (see gol_selftest in gol_capi.cpp).
hipError_t launch_selftest(const uint32_t* in, uint32_t* out, hipStream_t stream);

// ---- census and windows (gol_region.hip) -------------------------------------

// Census accumulators: kCensusSlots slots one 64-byte line apart, each
// {population, min_x, max_x, min_y, max_y} as 64-bit values (the box signed,
// global coordinates); the identity is {0, INT64_MAX, -1, INT64_MAX, -1}.
constexpr int kCensusSlots = 64;
constexpr int kCensusSlotStride = 8;  // u64 per slot
constexpr int kCensusValues = 5;

// Every slot to the identity.
hipError_t launch_census_reset(unsigned long long* slots, hipStream_t stream);
// Population and bounding box of `rows` device rows (16-byte loads: `plane`
// 16-byte aligned, `pitch` a multiple of 4 words) into the slots.
hipError_t launch_census(const uint32_t* plane, int64_t pitch, int32_t wwords, int64_t grow0, int32_t rows, int ilv,
                         unsigned long long* slots, hipStream_t stream);
// out[0..5) = the slots combined (sum, min, max), which are left at the
// identity; `out` may be mapped host memory.
hipError_t launch_census_fold(unsigned long long* slots, unsigned long long* out, hipStream_t stream);

// Row occupancy (active-row stepping, gol_active.cpp): bit b of `bits` (`nwords`
// words, zero before the first launch that shares them) is set iff block b of
// kOccupancyBlock rows of the plane holds a non-zero word, for the blocks of
// local rows [lo, hi), lo a multiple of the block; other bits are left alone.
// 16-byte loads, as launch_census.  launch_density_export exports the bitmap
// and leaves it zero.
constexpr int kOccupancyBlock = 64;  // golactive::kActiveBlock (gol_active.cpp asserts they agree)
hipError_t launch_row_occupancy(const uint32_t* plane, int64_t pitch, int32_t wwords, int32_t lo, int32_t hi,
                                uint32_t* bits, int32_t nwords, hipStream_t stream);

// Window columns [x0, x0 + w) (modulo the row: 32 * wwords columns) of
// `nrows` device rows starting at `src`, as packed row-major rows of
// ceil(w / 32) words in `stage`; bits past w are zero.
hipError_t launch_region_gather(const uint32_t* src, int64_t pitch, int32_t wwords, int ilv, int32_t nrows, int64_t x0,
                                int64_t w, uint32_t* stage, hipStream_t stream);
// The reverse: `stage` (as above; bits past w ignored) combined into columns
// [x0, x0 + w) of `nrows` device rows starting at `dst` under `mode`
// (GOL_REGION_*), modulo `width` if wrap_x; every other bit is left as it is.
hipError_t launch_region_scatter(uint32_t* dst, int64_t pitch, int32_t wwords, int64_t width, int ilv, int32_t nrows,
                                 int64_t x0, int64_t w, const uint32_t* stage, int mode, bool wrap_x,
                                 hipStream_t stream);

// Density map (gol_density): the live cells of `nrows` device rows starting at
// `src` -- window rows from `win_row` on -- per T x T tile, T = 1 << lg, tiles
// anchored at the window origin.  `grid` is the rows' own part of the map: its
// row 0 is tile row win_row >> lg, rows are `tw` counts apart and there are
// `grid_rows` = the tile rows the window rows meet.  The two regimes meet at
// T = 64: from there on a 64-column group meets at most two tiles, below it a
// tile lies inside one 32-column window word.
constexpr int kDensityCoarseLog2 = 6;
// lg >= kDensityCoarseLog2.  Board columns [xa, xb) (no wrap; xa is window
// column `koff`) are added to the grid with atomics: zero it first; pieces of
// one window may share it.  16-byte loads, as launch_census.
hipError_t launch_density_coarse(const uint32_t* src, int64_t pitch, int32_t wwords, int ilv, int32_t nrows,
                                 int64_t win_row, int64_t xa, int64_t xb, int64_t koff, int lg, uint32_t* grid,
                                 int64_t tw, int64_t grid_rows, hipStream_t stream);
// lg < kDensityCoarseLog2.  Window columns [x0, x0 + w) (modulo the row, as
// launch_region_gather); tw = ceil(w / T).  Every count of the grid is stored.
hipError_t launch_density_fine(const uint32_t* src, int64_t pitch, int32_t wwords, int ilv, int32_t nrows,
                               int64_t win_row, int64_t x0, int64_t w, int lg, uint32_t* grid, int64_t tw,
                               int64_t grid_rows, hipStream_t stream);
// out[0..n) = grid[0..n), which is left zero; `out` may be mapped host memory
// (one launch in place of a copy and the next call's memset).
hipError_t launch_density_export(uint32_t* grid, uint32_t* out, int64_t n, hipStream_t stream);

// ---- pattern search (gol_find.hip) --------------------------------------------

// Match counters: kFindSlots sharded 64-bit counters one 64-byte line apart,
// then (on a line of its own) the cursor of the hit list; zero when clean.
constexpr int kFindSlots = 64;
constexpr int kFindSlotStride = 8;  // u64 per slot
constexpr int kFindCursorWord = kFindSlots * kFindSlotStride;
constexpr int kFindWords = kFindCursorWord + kFindSlotStride;
constexpr int kFindValues = 2;  // the fold's result: the count, the cursor

// A cared cell of the pattern as the kernel reads it: row i, column k, state.
constexpr uint32_t find_cell(int i, int k, bool alive) {
    return (uint32_t)i | ((uint32_t)k << 8) | ((alive ? 1u : 0u) << 16);
}

// One launch searches anchor rows [a_lo, a_hi) (local rows) at the window's
// columns: window word m holds anchor columns x0 + 32 m .. + 31 (modulo the
// width on a torus), the last one under last_mask.  Pattern rows past `rows`
// wrap into the plane (wrap_y: the shard is a whole torus) or read dead;
// columns past the row wrap (wrap_x) or read dead.
struct FindParams {
    const uint32_t* plane;      // local row 0 of the current plane
    const uint32_t* cells;      // ncells cared cells (find_cell), the live ones first
    unsigned long long* slots;  // kFindWords counters
    long long* hits;            // max_hits (x, y) pairs, or null (count only)
    int64_t pitch;
    int64_t max_hits;
    int64_t grow0;              // global row of local row 0
    int64_t x0, width;
    int32_t wwords, rows;
    int32_t a_lo, a_hi;
    int32_t sw;                 // words of a window row = ceil(w / 32)
    uint32_t last_mask;
    int32_t c_first, sh;        // x0 / 32, x0 % 32
    int32_t nw;                 // row-major words a lane reads per pattern row: 1 .. 4
    int32_t ncells;
    int32_t prefilter;          // the first cell of the list is live and the rows take 16-byte loads that wrap
                                // whole (find_prefilter_fits): empty neighbourhoods are refused a KiB at a time
    int32_t wrap_x, wrap_y;
};
// The prefilter reads the plane in 16-byte units: they must wrap whole on a
// torus (every board of 128 k columns; the planes' alignment and pitch always
// fit).  Without it every item runs the matching loop, which leaves after the
// first cell's loads where nothing is alive.
inline bool find_prefilter_fits(bool wrap_x, int32_t wwords) { return !wrap_x || wwords % 4 == 0; }
// Adds the matches to the counters and their positions (global coordinates)
// to the hit list; positions past max_hits are dropped.
hipError_t launch_find(const FindParams& p, int ilv, hipStream_t stream);
// out[0] = the counters' sum, out[1] = the cursor; all left zero.  `out` may
// be mapped host memory.
hipError_t launch_find_fold(unsigned long long* slots, unsigned long long* out, hipStream_t stream);

}  // namespace gol
