// gol_region.hip -- the board seen from the user's side of the C ABI without
// moving a plane: the census (population and bounding box in one pass over
// the plane), windows gathered from / scattered into the device layout, and
// the density map of a window (gol_census, gol_read_region, gol_write_region,
// gol_density in gol_region.cpp), and the row-occupancy scan of active-row
// stepping (gol_active.cpp).
#include <algorithm>

#include "gol_kernels.h"
#include "gol_layout.h"

namespace gol {

namespace {

constexpr int kCensusThreads = kWaveLanes * 4;

// ---- census ------------------------------------------------------------------
// A slot is one 64-byte line of five 64-bit values: population, min_x, max_x,
// min_y, max_y (the box as signed values; identity INT64_MAX / -1).

__device__ __forceinline__ int ctz32(uint32_t x) { return x ? __builtin_ctz(x) : 32; }
__device__ __forceinline__ int top32(uint32_t x) { return x ? 31 - __builtin_clz(x) : -1; }

// Lowest / highest live column of a 16-byte chunk (four words, not all zero),
// relative to the chunk's first column.  Row-major: x = 32 c + b.  Pair
// layout: word 2 g + j, bit b is x = 64 g + 2 b + j.
template <int ILV>
__device__ __forceinline__ int chunk_min(const uint32_t* w) {
    if (ILV == 2) {
        const bool first = (w[0] | w[1]) != 0;
        const uint32_t e = first ? w[0] : w[2], o = first ? w[1] : w[3];
        return (first ? 0 : 64) + min(2 * ctz32(e), 2 * ctz32(o) + 1);
    }
    const unsigned long long lo = w[0] | ((unsigned long long)w[1] << 32);
    const unsigned long long hi = w[2] | ((unsigned long long)w[3] << 32);
    return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(hi);
}
template <int ILV>
__device__ __forceinline__ int chunk_max(const uint32_t* w) {
    if (ILV == 2) {
        const bool last = (w[2] | w[3]) != 0;
        const uint32_t e = last ? w[2] : w[0], o = last ? w[3] : w[1];
        return (last ? 64 : 0) + max(2 * top32(e), 2 * top32(o) + 1);
    }
    const unsigned long long lo = w[0] | ((unsigned long long)w[1] << 32);
    const unsigned long long hi = w[2] | ((unsigned long long)w[3] << 32);
    return hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
}

// One pass over `rows` rows: 16-byte loads, a 256-thread workgroup covering
// 2^lgx chunks of 256 >> lgx rows per iteration (so narrow boards keep their
// lanes busy and the only division is workgroup-uniform).  Each lane keeps a
// population and a box in local coordinates; the bit scan runs only for
// chunks that can still move the lane's column extent, so a dense board pays
// for the load and four popcounts.  Lanes, waves and the workgroup are
// reduced before one set of atomics per workgroup on a sharded accumulator.
template <int ILV>
__global__ __launch_bounds__(kCensusThreads) void census_kernel(const uint32_t* __restrict__ plane, int64_t pitch,
                                                                int32_t wwords, int64_t grow0, int32_t rows, int lgx,
                                                                unsigned long long* slots) {
    const int bx = 1 << lgx, by = kCensusThreads >> lgx;
    const int tx = threadIdx.x & (bx - 1), ty = threadIdx.x >> lgx;
    const int32_t chunks = (wwords + 3) / 4;
    const int32_t xtiles = (chunks + bx - 1) >> lgx;
    const int64_t items = (int64_t)((rows + by - 1) / by) * xtiles;
    unsigned long long pop = 0;
    int minx = INT32_MAX, maxx = -1, miny = INT32_MAX, maxy = -1;
    constexpr int kInFlight = 2;  // tiles loaded before the first is counted: 2 KiB per wave on its way
    for (int64_t it0 = blockIdx.x; it0 < items; it0 += (int64_t)kInFlight * gridDim.x) {
        uint4 v[kInFlight];
        int32_t row[kInFlight], chunk[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int64_t it = it0 + (int64_t)u * gridDim.x;
            const int64_t yt = it / xtiles;
            const int32_t xt = (int32_t)(it - yt * xtiles);
            const int64_t r = yt * by + ty;
            const int32_t q = xt * bx + tx;
            row[u] = (int32_t)r;
            chunk[u] = q;
            v[u] = make_uint4(0u, 0u, 0u, 0u);  // outside the plane: nothing alive
            if (it < items && r < rows && q < chunks)
                v[u] = *reinterpret_cast<const uint4*>(plane + r * pitch + 4 * (int64_t)q);
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int32_t q = chunk[u];
            uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            if (4 * q + 3 >= wwords) {  // the row's last chunk: words of the pitch padding do not count
#pragma unroll
                for (int i = 1; i < 4; ++i)
                    if (4 * q + i >= wwords) w[i] = 0;
            }
            if ((w[0] | w[1] | w[2] | w[3]) == 0) continue;
            pop += (uint32_t)(__popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]));
            miny = min(miny, row[u]);
            maxy = max(maxy, row[u]);
            const int x = 128 * q;  // width < 2^31
            if (x < minx) minx = min(minx, x + chunk_min<ILV>(w));
            if (x + 127 > maxx) maxx = max(maxx, x + chunk_max<ILV>(w));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pop += __shfl_xor(pop, off, kWaveLanes);
        minx = min(minx, __shfl_xor(minx, off, kWaveLanes));
        maxx = max(maxx, __shfl_xor(maxx, off, kWaveLanes));
        miny = min(miny, __shfl_xor(miny, off, kWaveLanes));
        maxy = max(maxy, __shfl_xor(maxy, off, kWaveLanes));
    }
    constexpr int kWaves = kCensusThreads / kWaveLanes;
    __shared__ unsigned long long s_pop[kWaves];
    __shared__ int s_box[kWaves][4];
    const int wave = threadIdx.x / kWaveLanes;
    if ((threadIdx.x & (kWaveLanes - 1)) == 0) {
        s_pop[wave] = pop;
        s_box[wave][0] = minx;
        s_box[wave][1] = maxx;
        s_box[wave][2] = miny;
        s_box[wave][3] = maxy;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
        pop += s_pop[k];
        minx = min(minx, s_box[k][0]);
        maxx = max(maxx, s_box[k][1]);
        miny = min(miny, s_box[k][2]);
        maxy = max(maxy, s_box[k][3]);
    }
    if (pop == 0) return;  // nothing alive here: the slot keeps its identity
    unsigned long long* slot = slots + (size_t)(blockIdx.x % kCensusSlots) * kCensusSlotStride;
    long long* box = reinterpret_cast<long long*>(slot);
    atomicAdd(slot, pop);
    atomicMin(box + 1, (long long)minx);
    atomicMax(box + 2, (long long)maxx);
    atomicMin(box + 3, grow0 + miny);
    atomicMax(box + 4, grow0 + maxy);
}

__device__ __forceinline__ void census_identity(unsigned long long* slot) {
    slot[0] = 0ull;
    slot[1] = (unsigned long long)INT64_MAX;
    slot[2] = (unsigned long long)-1ll;
    slot[3] = (unsigned long long)INT64_MAX;
    slot[4] = (unsigned long long)-1ll;
}

static_assert(kCensusSlots == kWaveLanes, "one accumulator per lane");
__global__ __launch_bounds__(kWaveLanes) void census_reset_kernel(unsigned long long* slots) {
    census_identity(slots + (size_t)threadIdx.x * kCensusSlotStride);
}

// One wave: lane k takes slot k and leaves its identity behind, the wave
// combines them, lane 0 stores the five values to `out` -- mapped
// page-locked host memory, read after the stream synchronises.
__global__ __launch_bounds__(kWaveLanes) void census_fold_kernel(unsigned long long* slots, unsigned long long* out) {
    unsigned long long* slot = slots + (size_t)threadIdx.x * kCensusSlotStride;
    unsigned long long pop = slot[0];
    long long minx = (long long)slot[1], maxx = (long long)slot[2];
    long long miny = (long long)slot[3], maxy = (long long)slot[4];
    census_identity(slot);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pop += __shfl_xor(pop, off, kWaveLanes);
        minx = min(minx, __shfl_xor(minx, off, kWaveLanes));
        maxx = max(maxx, __shfl_xor(maxx, off, kWaveLanes));
        miny = min(miny, __shfl_xor(miny, off, kWaveLanes));
        maxy = max(maxy, __shfl_xor(maxy, off, kWaveLanes));
    }
    if (threadIdx.x == 0) {  // vector stores
        out[0] = pop;
        out[1] = (unsigned long long)minx;
        out[2] = (unsigned long long)maxx;
        out[3] = (unsigned long long)miny;
        out[4] = (unsigned long long)maxy;
    }
}

// ---- windows -------------------------------------------------------------------

// Row-major word c of a device row.
__device__ __forceinline__ uint32_t load_row_major(const uint32_t* row, int32_t c, int ilv) {
    if (ilv == 2) {
        const uint32_t q[2] = {row[c & ~1], row[(c & ~1) + 1]};
        return row_major_word(q, c & 1);
    }
    return row[c];
}

// 32 window columns of a device row: row-major words c0 and c1 (the next one,
// modulo the row) funnel-shifted by sh = x0 % 32.
__device__ __forceinline__ uint32_t window_word(const uint32_t* row, int32_t c0, int32_t c1, int sh, int ilv) {
    const uint32_t lo = load_row_major(row, c0, ilv), hi = load_row_major(row, c1, ilv);
    return (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> sh);
}

// One thread per window word: word m of window row r holds window columns
// 32 m .. 32 m + 31 = board columns from x0 + 32 m on, i.e. row-major words
// c_first + m and the next one (modulo the row: torus widths are multiples
// of 32) funnel-shifted by sh = x0 % 32.  The row's last word keeps only the
// columns below w.
__global__ void region_gather_kernel(const uint32_t* __restrict__ src, int64_t pitch, int32_t wwords, int ilv,
                                     int32_t nrows, int32_t c_first, int sh, int32_t sw, uint32_t last_mask,
                                     uint32_t* __restrict__ stage) {
    const int64_t total = (int64_t)nrows * sw;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = k / sw;
        const int32_t m = (int32_t)(k - r * sw);
        int32_t c0 = c_first + m;  // c_first < wwords, m < sw <= wwords
        if (c0 >= wwords) c0 -= wwords;
        const int32_t c1 = c0 + 1 == wwords ? 0 : c0 + 1;
        uint32_t v = window_word(src + r * pitch, c0, c1, sh, ilv);
        if (m == sw - 1) v &= last_mask;
        stage[k] = v;
    }
}

// Window columns k0 .. k0 + 31 of a staged window row (sw words, the last one
// valid under last_mask) as a word, with the mask of those that exist:
// columns outside [0, w) read as absent.
__device__ __forceinline__ void window_bits(const uint32_t* srow, int32_t sw, uint32_t last_mask, int64_t k0,
                                            uint32_t& val, uint32_t& mask) {
    val = mask = 0u;
    if (k0 <= -32 || k0 >= 32 * (int64_t)sw) return;
    const int64_t m = k0 >> 5;  // floor: -1 for -32 < k0 < 0
    const int s = (int)(k0 & 31);
    uint32_t v[2], mk[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t j = m + i;
        const bool in = j >= 0 && j < sw;
        mk[i] = in ? (j == sw - 1 ? last_mask : 0xFFFFFFFFu) : 0u;
        v[i] = in ? srow[j] & mk[i] : 0u;
    }
    val = (uint32_t)(((((unsigned long long)v[1]) << 32) | v[0]) >> s);
    mask = (uint32_t)(((((unsigned long long)mk[1]) << 32) | mk[0]) >> s);
}

// The new value of row-major word c of a board row under the window: column
// x = 32 c + b is window column x - x0, or x - x0 + width where the window
// wraps the row (a word can take bits from both ends of a window as wide as
// the board); the two never claim the same bit because w <= width.
__device__ __forceinline__ uint32_t apply_window(uint32_t old, int32_t c, const uint32_t* srow, int32_t sw,
                                                 uint32_t last_mask, int64_t x0, int64_t width, int wrap_x, int mode) {
    uint32_t val, mask;
    window_bits(srow, sw, last_mask, 32 * (int64_t)c - x0, val, mask);
    if (wrap_x) {
        uint32_t v2, m2;
        window_bits(srow, sw, last_mask, 32 * (int64_t)c - x0 + width, v2, m2);
        val |= v2;
        mask |= m2;
    }
    switch (mode) {
        case 0: return (old & ~mask) | val;  // GOL_REGION_COPY
        case 1: return old | val;            // GOL_REGION_OR
        case 2: return old ^ val;            // GOL_REGION_XOR
        default: return old & ~val;          // GOL_REGION_CLEAR
    }
}

// Owner computes: one thread per destination unit -- a word of a row-major
// row, a pair of the pair layout -- of the `nunits` units per row the window
// touches, starting at unit u_first and wrapping modulo the row's `units`
// (nunits <= units, so every unit has one owner: no atomics, no races).
__global__ void region_scatter_kernel(uint32_t* __restrict__ dst, int64_t pitch, int32_t units, int ilv, int32_t nrows,
                                      int32_t u_first, int32_t nunits, int64_t x0, int64_t width, int wrap_x,
                                      const uint32_t* __restrict__ stage, int32_t sw, uint32_t last_mask, int mode) {
    const int64_t total = (int64_t)nrows * nunits;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = k / nunits;
        int32_t u = u_first + (int32_t)(k - r * nunits);  // u_first < units, the rest < nunits <= units
        if (u >= units) u -= units;
        uint32_t* row = dst + r * pitch;
        const uint32_t* srow = stage + r * sw;
        if (ilv == 2) {
            const uint32_t q[2] = {row[2 * u], row[2 * u + 1]};
            const uint32_t old[2] = {row_major_word(q, 0), row_major_word(q, 1)};
            uint32_t rm[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                rm[i] = apply_window(old[i], 2 * u + i, srow, sw, last_mask, x0, width, wrap_x, mode);
            if (rm[0] != old[0] || rm[1] != old[1]) {
                row[2 * u] = device_word(rm, 0);
                row[2 * u + 1] = device_word(rm, 1);
            }
        } else {
            const uint32_t old = row[u];
            const uint32_t now = apply_window(old, u, srow, sw, last_mask, x0, width, wrap_x, mode);
            if (now != old) row[u] = now;
        }
    }
}

// ---- density map ---------------------------------------------------------------
// Live cells per T x T tile (T = 1 << lg) of a window, tiles anchored at the
// window origin.  The host cuts the window into pieces that wrap neither way:
// a run of owned rows (window row `wrow0` on) times board columns [xa, xb),
// whose first column is window column `koff`.  `grid` is the run's part of the
// map: row 0 is tile row wrow0 >> lg, `tw` counts per row, `grows` rows.

// Bits [lo, hi) of a word, 0 <= lo, hi <= 32; empty when hi <= lo.
__device__ __forceinline__ uint32_t bit_range(int lo, int hi) {
    return hi > lo ? (uint32_t)(((1ull << hi) - 1ull) & ~((1ull << lo) - 1ull)) : 0u;
}

// Columns [lo, hi) (0 <= lo, hi <= 64) of a 64-column group as masks of its
// two device words.  Pair layout: word j, bit b is column 2 b + j, so the
// columns are bits ceil((lo - j) / 2) .. ceil((hi - j) / 2) - 1 of word j.
template <int ILV>
__device__ __forceinline__ void group_masks(int lo, int hi, uint32_t& m0, uint32_t& m1) {
    if (ILV == 2) {
        m0 = bit_range((lo + 1) >> 1, (hi + 1) >> 1);
        m1 = bit_range(lo >> 1, hi >> 1);
    } else {
        m0 = bit_range(min(lo, 32), min(hi, 32));
        m1 = bit_range(max(lo, 32) - 32, max(hi, 32) - 32);
    }
}

constexpr int kDensityInFlight = 4;                       // 16-byte loads a lane issues before it counts
constexpr int kDensityLdsTiles = 2 * kCensusThreads + 2;  // tiles a workgroup's columns can meet at T >= 64

// Coarse tiles (T >= 64): the census's pass -- 16-byte loads, a workgroup of
// 2^lgx chunks times 256 >> lgx rows -- with the lane's chunk fixed over a slab
// of up to 2^lgr <= T window rows of one tile row.  A 64-column group meets at
// most two tiles, so a lane holds two masks per word (all ones or zero away
// from tile edges and the ends of the piece; columns outside [xa, xb), padding
// words included, are in neither) and four counters.  The workgroup sums its
// lanes per tile in LDS and adds what is not zero to the grid: one vector
// atomic per tile, slab and workgroup.
template <int ILV>
__global__ __launch_bounds__(kCensusThreads) void density_coarse_kernel(const uint32_t* __restrict__ plane,
                                                                        int64_t pitch, int32_t nrows, int64_t wrow0,
                                                                        int64_t xa, int64_t xb, int64_t koff,
                                                                        int32_t q_first, int32_t nchunks, int lgx,
                                                                        int lg, int lgr, unsigned* grid, int64_t tw,
                                                                        int64_t grows) {
    __shared__ unsigned s_cnt[kDensityLdsTiles];
    const int bx = 1 << lgx, by = kCensusThreads >> lgx;
    const int tx = threadIdx.x & (bx - 1), ty = threadIdx.x >> lgx;
    const int32_t xtiles = (nchunks + bx - 1) >> lgx;
    const int64_t slab0 = wrow0 >> lgr;
    const int64_t items = (((wrow0 + nrows - 1) >> lgr) - slab0 + 1) * xtiles;
    const int span = 2 * bx + 2;
    for (int t = threadIdx.x; t < span; t += kCensusThreads) s_cnt[t] = 0u;
    __syncthreads();
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t sl = it / xtiles;
        const int32_t xt = (int32_t)(it - sl * xtiles);
        // the slab's rows: local rows [r_lo, r_hi) of the run, all of tile row `trow` of the grid
        const int64_t wlo = max(wrow0, (slab0 + sl) << lgr), whi = min(wrow0 + nrows, (slab0 + sl + 1) << lgr);
        const int32_t r_lo = (int32_t)(wlo - wrow0), r_hi = (int32_t)(whi - wrow0);
        const int64_t trow = (wlo >> lg) - (wrow0 >> lg);
        // the workgroup's first tile and the lane's chunk
        const int32_t qb = q_first + xt * bx, q = qb + tx;
        const int64_t tbase = (max(xa, 128 * (int64_t)qb) - xa + koff) >> lg;
        const bool live = q < q_first + nchunks;
        uint32_t m[2][2][2];  // [group][tile: first, next][word]
        int lt[2];            // the group's first tile, relative to tbase
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int64_t g0 = 128 * (int64_t)q + 64 * g;
            const int lo = (int)min(max(xa - g0, (int64_t)0), (int64_t)64);
            const int hi = live ? (int)min(max(xb - g0, (int64_t)0), (int64_t)64) : 0;
            const int64_t xc = min(max(g0, xa), xb - 1);  // the group's first column of the piece, or the nearest one
            const int64_t t = (xc - xa + koff) >> lg;
            // tile t + 1 begins at this column of the group
            const int s = (int)min(max(((t + 1) << lg) - koff + xa - g0, (int64_t)lo), (int64_t)max(lo, hi));
            group_masks<ILV>(lo, s, m[g][0][0], m[g][0][1]);
            group_masks<ILV>(s, hi, m[g][1][0], m[g][1][1]);
            lt[g] = (int)(t - tbase);
        }
        uint32_t cnt[2][2] = {{0u, 0u}, {0u, 0u}};
        if (live) {
            const uint32_t* col = plane + 4 * (int64_t)q;
            for (int32_t r0 = r_lo + ty; r0 < r_hi; r0 += kDensityInFlight * by) {
                uint4 v[kDensityInFlight];
#pragma unroll
                for (int u = 0; u < kDensityInFlight; ++u) {
                    const int32_t r = r0 + u * by;
                    v[u] = make_uint4(0u, 0u, 0u, 0u);
                    if (r < r_hi) v[u] = *reinterpret_cast<const uint4*>(col + r * pitch);
                }
#pragma unroll
                for (int u = 0; u < kDensityInFlight; ++u) {
                    const uint32_t w[2][2] = {{v[u].x, v[u].y}, {v[u].z, v[u].w}};
#pragma unroll
                    for (int g = 0; g < 2; ++g)
#pragma unroll
                        for (int k = 0; k < 2; ++k)
                            cnt[g][k] += (uint32_t)(__popc(w[g][0] & m[g][k][0]) + __popc(w[g][1] & m[g][k][1]));
                }
            }
        }
        // A count that is not zero belongs to a tile of the piece, which the two range checks below
        // cannot refuse; they stay so that a slip in this arithmetic shows as a wrong count in the
        // tests and never as a store outside the grid.
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (cnt[g][k] != 0u && (unsigned)(lt[g] + k) < (unsigned)span) atomicAdd(&s_cnt[lt[g] + k], cnt[g][k]);
        __syncthreads();
        for (int t = threadIdx.x; t < span; t += kCensusThreads) {
            const unsigned c = s_cnt[t];
            if (c == 0u) continue;
            s_cnt[t] = 0u;  // left clean for the next item
            if (tbase + t < tw && trow < grows) atomicAdd(grid + trow * tw + tbase + t, c);
        }
        __syncthreads();
    }
}

// Fine tiles (T <= 32): one thread per tile of the run's part of the map.  A
// tile lies inside one 32-column word of the window, gathered as
// region_gather_kernel gathers it; the thread counts the tile's bits of that
// word over the tile's rows and stores the count (every tile has one owner).
__global__ void density_fine_kernel(const uint32_t* __restrict__ src, int64_t pitch, int32_t wwords, int ilv,
                                    int32_t nrows, int64_t wrow0, int32_t c_first, int sh, int64_t w, int lg,
                                    unsigned* __restrict__ grid, int64_t tw, int64_t grows) {
    const int64_t total = grows * tw;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ti = idx / tw, k = idx - ti * tw;
        const int64_t wtop = ((wrow0 >> lg) + ti) << lg;  // the tile's first window row
        const int32_t r_lo = (int32_t)(max(wrow0, wtop) - wrow0);
        const int32_t r_hi = (int32_t)(min(wrow0 + nrows, wtop + ((int64_t)1 << lg)) - wrow0);
        const int64_t c = k << lg;  // the tile's first window column
        const int o = (int)(c & 31);
        const uint32_t mask = bit_range(o, o + (int)min((int64_t)1 << lg, w - c));
        int32_t c0 = c_first + (int32_t)(c >> 5);  // c_first < wwords, c / 32 < ceil(w / 32) <= wwords
        if (c0 >= wwords) c0 -= wwords;
        const int32_t c1 = c0 + 1 == wwords ? 0 : c0 + 1;
        unsigned count = 0u;
        for (int32_t r = r_lo; r < r_hi; ++r) count += (unsigned)__popc(window_word(src + r * pitch, c0, c1, sh, ilv) & mask);
        grid[idx] = count;
    }
}

// The grid's first n counts to `out` -- mapped page-locked host memory, read
// after the stream synchronises -- leaving the grid zero for the next call.
__global__ void density_export_kernel(unsigned* __restrict__ grid, unsigned* __restrict__ out, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const unsigned c = grid[idx];
        out[idx] = c;
        if (c != 0u) grid[idx] = 0u;
    }
}

// ---- row occupancy ---------------------------------------------------------------
// Which blocks of kOccupancyBlock rows hold a non-zero word (active-row
// stepping, gol_active.cpp): bit b of `bits` is set iff block b of the plane
// does, for the blocks of local rows [lo, hi), lo a multiple of the block.
// The census's pass -- 16-byte loads, kOccInFlight on their way, a workgroup
// of 2^lgx chunks times 256 >> lgx rows -- with an OR in place of the counts.
// The layout does not matter (a non-zero word is a live word in either), nor
// do the words of the pitch padding, which are zero.  A workgroup takes `per`
// consecutive tiles, row tile by row tile, so the blocks it meets are
// consecutive: its waves mark them in an LDS copy of the bitmap words they
// fall into (a wave's rows of one tile lie in one block, so the ballot of a
// tile is one block's), and the words that are not zero go out at the end --
// at most one vector atomic per workgroup and bitmap word, none for empty
// blocks.
constexpr int kOccInFlight = 4;
constexpr int kOccLdsWords = 130;  // bitmap words a workgroup's rows can meet (launch_row_occupancy sizes the grid)
constexpr int kOccRowsPerWG = 131072;

__global__ __launch_bounds__(kCensusThreads) void row_occupancy_kernel(const uint32_t* __restrict__ plane, int64_t pitch,
                                                                       int32_t chunks, int32_t lo, int32_t hi, int lgx,
                                                                       int64_t per, unsigned* bits, int32_t nwords) {
    __shared__ unsigned s_bits[kOccLdsWords];
    const int bx = 1 << lgx, by = kCensusThreads >> lgx;
    const int tx = threadIdx.x & (bx - 1), ty = threadIdx.x >> lgx;
    const int32_t xtiles = (chunks + bx - 1) >> lgx;
    const int64_t items = (int64_t)((hi - lo + by - 1) / by) * xtiles;
    const int64_t it_lo = min((int64_t)blockIdx.x * per, items), it_hi = min(items, it_lo + per);
    // the bitmap word of the first block this workgroup can meet
    const int32_t w0 = (int32_t)(((lo + (it_lo / xtiles) * by) / kOccupancyBlock) >> 5);
    for (int t = threadIdx.x; t < kOccLdsWords; t += kCensusThreads) s_bits[t] = 0u;
    __syncthreads();
    int32_t marked = -1;  // the block this wave marked last
    for (int64_t it0 = it_lo; it0 < it_hi; it0 += kOccInFlight) {
        uint4 v[kOccInFlight];
        int32_t row[kOccInFlight];
#pragma unroll
        for (int u = 0; u < kOccInFlight; ++u) {
            const int64_t it = it0 + u;
            const int64_t yt = it / xtiles;
            const int32_t xt = (int32_t)(it - yt * xtiles);
            const int64_t r = lo + yt * by + ty;
            const int32_t q = xt * bx + tx;
            row[u] = (int32_t)min(r, (int64_t)INT32_MAX);
            v[u] = make_uint4(0u, 0u, 0u, 0u);  // outside the rows: nothing alive
            if (it < it_hi && r < hi && q < chunks)
                v[u] = *reinterpret_cast<const uint4*>(plane + r * pitch + 4 * (int64_t)q);
        }
#pragma unroll
        for (int u = 0; u < kOccInFlight; ++u) {
            const bool any = __ballot((v[u].x | v[u].y | v[u].z | v[u].w) != 0u) != 0ull;  // wave-uniform
            const int32_t blk = __builtin_amdgcn_readfirstlane(row[u] / kOccupancyBlock);
            if (!any || blk == marked) continue;
            marked = blk;
            const int32_t idx = (blk >> 5) - w0;
            if ((threadIdx.x & (kWaveLanes - 1)) == 0 && (unsigned)idx < (unsigned)kOccLdsWords)
                atomicOr(&s_bits[idx], 1u << (blk & 31));
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kOccLdsWords; t += kCensusThreads) {
        const unsigned b = s_bits[t];
        if (b != 0u && w0 + t < nwords) atomicOr(bits + w0 + t, b);
    }
}

int grid_for(int64_t total) { return (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 2048)); }

uint32_t last_word_mask(int64_t w) { return w % 32 ? (uint32_t)((1ull << (w % 32)) - 1ull) : 0xFFFFFFFFu; }

}  // namespace

hipError_t launch_census_reset(unsigned long long* slots, hipStream_t stream) {
    return launch_kernel(census_reset_kernel, dim3(1), dim3(kWaveLanes), stream, slots);
}

hipError_t launch_census(const uint32_t* plane, int64_t pitch, int32_t wwords, int64_t grow0, int32_t rows, int ilv,
                         unsigned long long* slots, hipStream_t stream) {
    // 16-byte loads: rows must start 16-byte aligned and hold whole chunks
    if ((ilv != 1 && ilv != 2) || pitch % 4 != 0 || pitch < (wwords + 3) / 4 * 4 || rows < 1 || wwords < 1 ||
        (reinterpret_cast<uintptr_t>(plane) & 15) != 0)
        return hipErrorInvalidValue;
    const int32_t chunks = (wwords + 3) / 4;
    int lgx = 0;
    while (lgx < 8 && (1 << lgx) < chunks) ++lgx;
    const int bx = 1 << lgx, by = kCensusThreads >> lgx;
    const int64_t items = (int64_t)((rows + by - 1) / by) * ((chunks + bx - 1) / bx);
    // memory-bound: at most 8 workgroups per CU of a 256-CU part, the rest by grid stride
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(items, 2048));
    if (ilv == 2)
        return launch_kernel(census_kernel<2>, dim3(blocks), dim3(kCensusThreads), stream, plane, pitch, wwords, grow0,
                             rows, lgx, slots);
    return launch_kernel(census_kernel<1>, dim3(blocks), dim3(kCensusThreads), stream, plane, pitch, wwords, grow0,
                         rows, lgx, slots);
}

hipError_t launch_census_fold(unsigned long long* slots, unsigned long long* out, hipStream_t stream) {
    return launch_kernel(census_fold_kernel, dim3(1), dim3(kWaveLanes), stream, slots, out);
}

hipError_t launch_row_occupancy(const uint32_t* plane, int64_t pitch, int32_t wwords, int32_t lo, int32_t hi,
                                uint32_t* bits, int32_t nwords, hipStream_t stream) {
    // 16-byte loads, as the census; every block of the rows has its bit in the bitmap
    if (pitch % 4 != 0 || pitch < (wwords + 3) / 4 * 4 || wwords < 1 || lo < 0 || lo >= hi || lo % kOccupancyBlock != 0 ||
        (reinterpret_cast<uintptr_t>(plane) & 15) != 0 || !bits ||
        ((int64_t)hi + kOccupancyBlock - 1) / kOccupancyBlock > 32 * (int64_t)nwords)
        return hipErrorInvalidValue;
    const int32_t chunks = (wwords + 3) / 4;
    int lgx = 0;
    while (lgx < 8 && (1 << lgx) < chunks) ++lgx;
    const int bx = 1 << lgx, by = kCensusThreads >> lgx;
    const int64_t xtiles = (chunks + bx - 1) / bx;
    const int64_t items = (int64_t)((hi - lo + by - 1) / by) * xtiles;
    // memory-bound, as the census: at most 2048 workgroups, more only where one would otherwise meet more
    // rows than its LDS bitmap covers (kOccLdsWords)
    static_assert((kOccRowsPerWG + 3 * kCensusThreads) / kOccupancyBlock + 1 <= 32 * (kOccLdsWords - 1), "LDS bitmap");
    const int64_t blocks = std::max<int64_t>({1, std::min<int64_t>(items, 2048), ((int64_t)hi - lo) / kOccRowsPerWG + 1});
    const int64_t per = (items + blocks - 1) / blocks;
    return launch_kernel(row_occupancy_kernel, dim3((unsigned)((items + per - 1) / per)), dim3(kCensusThreads), stream,
                         plane, pitch, chunks, lo, hi, lgx, per, reinterpret_cast<unsigned*>(bits), nwords);
}

hipError_t launch_region_gather(const uint32_t* src, int64_t pitch, int32_t wwords, int ilv, int32_t nrows, int64_t x0,
                                int64_t w, uint32_t* stage, hipStream_t stream) {
    if ((ilv != 1 && ilv != 2) || nrows < 1 || w < 1 || w > 32 * (int64_t)wwords || x0 < 0 || x0 >= 32 * (int64_t)wwords)
        return hipErrorInvalidValue;
    const int32_t sw = (int32_t)((w + 31) / 32);
    return launch_kernel(region_gather_kernel, dim3(grid_for((int64_t)nrows * sw)), dim3(256), stream, src, pitch,
                         wwords, ilv, nrows, (int32_t)(x0 / 32), (int)(x0 % 32), sw, last_word_mask(w), stage);
}

hipError_t launch_region_scatter(uint32_t* dst, int64_t pitch, int32_t wwords, int64_t width, int ilv, int32_t nrows,
                                 int64_t x0, int64_t w, const uint32_t* stage, int mode, bool wrap_x,
                                 hipStream_t stream) {
    if ((ilv != 1 && ilv != 2) || wwords % ilv != 0 || nrows < 1 || w < 1 || w > width || x0 < 0 || x0 >= width ||
        width > 32 * (int64_t)wwords || mode < 0 || mode > 3 || (!wrap_x && x0 + w > width))
        return hipErrorInvalidValue;
    const int64_t span = 32 * ilv;  // columns per unit
    const int32_t units = wwords / ilv;
    const int32_t nunits = (int32_t)std::min<int64_t>(units, (x0 % span + w + span - 1) / span);
    const int32_t sw = (int32_t)((w + 31) / 32);
    return launch_kernel(region_scatter_kernel, dim3(grid_for((int64_t)nrows * nunits)), dim3(256), stream, dst, pitch,
                         units, ilv, nrows, (int32_t)(x0 / span), nunits, x0, width, wrap_x ? 1 : 0, stage, sw,
                         last_word_mask(w), mode);
}

hipError_t launch_density_coarse(const uint32_t* src, int64_t pitch, int32_t wwords, int ilv, int32_t nrows,
                                 int64_t win_row, int64_t xa, int64_t xb, int64_t koff, int lg, uint32_t* grid,
                                 int64_t tw, int64_t grid_rows, hipStream_t stream) {
    // 16-byte loads, as the census: aligned rows that hold whole chunks
    if ((ilv != 1 && ilv != 2) || pitch % 4 != 0 || pitch < (wwords + 3) / 4 * 4 || nrows < 1 || win_row < 0 ||
        xa < 0 || xa >= xb || xb > 32 * (int64_t)wwords || koff < 0 || lg < kDensityCoarseLog2 || lg > 15 || tw < 1 ||
        grid_rows != ((win_row + nrows - 1) >> lg) - (win_row >> lg) + 1 || ((koff + xb - xa - 1) >> lg) >= tw ||
        (reinterpret_cast<uintptr_t>(src) & 15) != 0)
        return hipErrorInvalidValue;
    const int32_t q_first = (int32_t)(xa / 128), nchunks = (int32_t)((xb + 127) / 128) - q_first;
    int lgx = 0;
    while (lgx < 8 && (1 << lgx) < nchunks) ++lgx;
    // a slab: up to 64 rows per lane, within one tile row
    const int lgr = std::min(lg, 8 - lgx + 6);
    const int64_t slabs = ((win_row + nrows - 1) >> lgr) - (win_row >> lgr) + 1;
    const int64_t items = slabs * ((nchunks + (1 << lgx) - 1) >> lgx);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(items, 2048));  // as the census
    unsigned* g = reinterpret_cast<unsigned*>(grid);
    if (ilv == 2)
        return launch_kernel(density_coarse_kernel<2>, dim3(blocks), dim3(kCensusThreads), stream, src, pitch, nrows,
                             win_row, xa, xb, koff, q_first, nchunks, lgx, lg, lgr, g, tw, grid_rows);
    return launch_kernel(density_coarse_kernel<1>, dim3(blocks), dim3(kCensusThreads), stream, src, pitch, nrows,
                         win_row, xa, xb, koff, q_first, nchunks, lgx, lg, lgr, g, tw, grid_rows);
}

hipError_t launch_density_fine(const uint32_t* src, int64_t pitch, int32_t wwords, int ilv, int32_t nrows,
                               int64_t win_row, int64_t x0, int64_t w, int lg, uint32_t* grid, int64_t tw,
                               int64_t grid_rows, hipStream_t stream) {
    if ((ilv != 1 && ilv != 2) || nrows < 1 || win_row < 0 || w < 1 || w > 32 * (int64_t)wwords || x0 < 0 ||
        x0 >= 32 * (int64_t)wwords || lg < 0 || lg >= kDensityCoarseLog2 || tw != ((w - 1) >> lg) + 1 ||
        grid_rows != ((win_row + nrows - 1) >> lg) - (win_row >> lg) + 1)
        return hipErrorInvalidValue;
    return launch_kernel(density_fine_kernel, dim3(grid_for(grid_rows * tw)), dim3(256), stream, src, pitch, wwords,
                         ilv, nrows, win_row, (int32_t)(x0 / 32), (int)(x0 % 32), w, lg,
                         reinterpret_cast<unsigned*>(grid), tw, grid_rows);
}

hipError_t launch_density_export(uint32_t* grid, uint32_t* out, int64_t n, hipStream_t stream) {
    if (n < 1) return hipErrorInvalidValue;
    return launch_kernel(density_export_kernel, dim3(grid_for(n)), dim3(256), stream,
                         reinterpret_cast<unsigned*>(grid), reinterpret_cast<unsigned*>(out), n);
}

}  // namespace gol
