// gol_find.hip -- pattern search on the device (gol_find in gol_region.cpp;
// DESIGN.md section 5e): every anchor of a window of anchors at which the
// board equals a pattern under its care mask.  Word-parallel: a lane owns 32
// consecutive anchor columns of one anchor row and keeps their match bits in
// one register; a cared cell (k, i) ANDs in board row y + i funnel-shifted by
// k, inverted where the pattern cell is dead.  The cared cells come as a list,
// live cells first, read through wave-uniform loads.  Launches none of the
// step kernels and shares no code with them.
#include <algorithm>

#include "gol_kernels.h"
#include "gol_layout.h"

namespace gol {

namespace {

constexpr int kFindThreads = kWaveLanes * 4;
constexpr int kGroupTiles = 4;  // tiles of an item: 256 words of an anchor row, 16 bytes per lane of the prefilter
constexpr int kFindProbe = 4;   // items whose prefilter loads a wave issues before it looks at the first

// The 64 columns around row-major word c of a device row as loaded: the pair
// that holds it (pair layout) or the word itself.  c < 0 (off a clipped
// board's right edge) and a null row (off its bottom edge) read dead.
template <int ILV>
__device__ __forceinline__ uint2 load_unit(const uint32_t* row, int32_t c) {
    if (c < 0 || !row) return make_uint2(0u, 0u);
    if (ILV == 2) return *reinterpret_cast<const uint2*>(row + (c & ~1));  // rows are 16-byte aligned, c & ~1 even
    return make_uint2(row[c], 0u);
}
// ... and row-major word c of it.
template <int ILV>
__device__ __forceinline__ uint32_t unit_word(uint2 q, int32_t c) {
    if (ILV == 2) {
        const uint32_t p[2] = {q.x, q.y};
        return row_major_word(p, c & 1);
    }
    return q.x;
}

// Row-major word index c (0 <= c, a few words past the row at most on the
// boards that matter) inside the row: wrapped on a torus, -1 past a clipped row.
__device__ __forceinline__ int32_t word_index(int32_t c, int32_t wwords, int wrap_x) {
    if (c < wwords) return c;
    if (!wrap_x) return -1;
    c -= wwords;
    return c < wwords ? c : c % wwords;
}

// Local row a + i of the plane: wrapped where the shard is a whole torus,
// null (dead) past the last row of a clipped board.  The host launches only
// anchors whose rows stay inside the plane otherwise.
__device__ __forceinline__ const uint32_t* board_row(const FindParams& p, int32_t a, int i) {
    int32_t r = a + i;
    if (r >= p.rows) {
        if (!p.wrap_y) return nullptr;
        r -= p.rows;  // ph <= rows: one turn
    }
    return p.plane + (int64_t)r * p.pitch;
}

// The match bits left of `cand` for anchor row `a`, the lane's anchors
// starting at bit `sh` of row-major word c0: every cared cell ANDs in its
// shifted board row.  A pattern row's words are loaded when the list reaches
// it (live cells first, each group in row order: at most two visits a row) and
// converted from the pair layout only if the wave loaded a live word.  The
// whole wave leaves as soon as no lane has a candidate.
template <int ILV>
__device__ __forceinline__ uint32_t match_row(const FindParams& p, const uint32_t* __restrict__ cells, int32_t a,
                                               int32_t c0, uint32_t cand) {
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
    int cur_i = -1;
    for (int32_t j = 0; j < p.ncells; ++j) {
        const uint32_t cell = cells[j];  // wave-uniform: a scalar load
        const int i = (int)(cell & 63u), k = (int)((cell >> 8) & 63u);
        const uint32_t inv = (cell >> 16) & 1u ? 0u : 0xFFFFFFFFu;
        if (i != cur_i) {
            cur_i = i;
            const uint32_t* row = board_row(p, a, i);
            int32_t c[4];
            uint2 q[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                c[t] = t < p.nw ? word_index(c0 + t, p.wwords, p.wrap_x) : -1;
                q[t] = load_unit<ILV>(row, c[t]);
            }
            const uint32_t any = q[0].x | q[0].y | q[1].x | q[1].y | q[2].x | q[2].y | q[3].x | q[3].y;
            w0 = w1 = w2 = w3 = 0u;
            if (ILV == 1) {
                w0 = q[0].x, w1 = q[1].x, w2 = q[2].x, w3 = q[3].x;
            } else if (__ballot(any != 0u) != 0ull) {
                w0 = unit_word<ILV>(q[0], c[0]);
                w1 = unit_word<ILV>(q[1], c[1]);
                w2 = unit_word<ILV>(q[2], c[2]);
                w3 = unit_word<ILV>(q[3], c[3]);
            }
        }
        const int s = p.sh + k;  // < 32 + 64: words s / 32 and the next, of the four
        const int idx = s >> 5;
        const uint32_t lo = idx == 0 ? w0 : idx == 1 ? w1 : w2;
        const uint32_t hi = idx == 0 ? w1 : idx == 1 ? w2 : w3;
        cand &= __funnelshift_r(lo, hi, (uint32_t)(s & 31)) ^ inv;
        if (__ballot(cand != 0u) == 0ull) break;
    }
    return cand;
}

// The wave's matches: one add to a sharded counter, one reservation of slots
// in the hit list (none once the list is full: every slot below max_hits has
// an owner by then), the positions of the slots that exist.  Vector atomics
// and stores only.
__device__ __forceinline__ void emit(const FindParams& p, uint32_t cand, int32_t a, int64_t xbase, int wave_slot) {
    const int lane = threadIdx.x & (kWaveLanes - 1);
    const uint32_t n = (uint32_t)__popc(cand);
    uint32_t pre = n;  // inclusive prefix over the lanes
#pragma unroll
    for (int off = 1; off < kWaveLanes; off <<= 1) {
        const uint32_t t = __shfl_up(pre, off, kWaveLanes);
        if (lane >= off) pre += t;
    }
    const uint32_t total = __shfl(pre, kWaveLanes - 1, kWaveLanes);
    unsigned long long base = 0ull;
    if (lane == 0) {
        atomicAdd(p.slots + (size_t)wave_slot * kFindSlotStride, (unsigned long long)total);
        if (p.hits) {
            unsigned long long* cursor = p.slots + kFindCursorWord;
            base = (unsigned long long)p.max_hits;
            if (__atomic_load_n(cursor, __ATOMIC_RELAXED) < base) base = atomicAdd(cursor, (unsigned long long)total);
        }
    }
    if (!p.hits) return;
    base = __shfl(base, 0, kWaveLanes);
    unsigned long long slot = base + pre - n;
    const int64_t y = p.grow0 + a;
    while (cand != 0u && slot < (unsigned long long)p.max_hits) {
        const int b = __builtin_ctz(cand);
        cand &= cand - 1u;
        int64_t x = xbase + b;
        if (p.wrap_x && x >= p.width) x -= p.width;
        p.hits[2 * slot] = (long long)x;
        p.hits[2 * slot + 1] = (long long)y;
        ++slot;
    }
}

// Word index s of a 16-byte unit (s a multiple of 4, >= 0) inside the row:
// wrapped on a torus whose rows hold whole units, -1 past a clipped row.
__device__ __forceinline__ int32_t unit_index(int32_t s, int32_t wwords, int wrap_x) {
    if (s < wwords) return s;
    if (!wrap_x) return -1;
    s -= wwords;
    return s < wwords ? s : s % wwords;
}

// One wave per item: kGroupTiles consecutive tiles of one anchor row, a tile
// being 64 consecutive words of the window (32 anchor columns each, one per
// lane); items by grid stride, kFindProbe at a time.  With a live cared cell
// first in the list (p.prefilter), the candidates after that cell are a
// shifted copy of one board row, so an item can match only if the words that
// cell reads -- the item's 256 words from word c_first + idx0 on and the one
// after them -- hold a live cell: each lane loads 16 bytes of them (the last
// lane the 16 after the others' too), for all kFindProbe items before any is
// looked at, and an item whose words are all zero is done.  On a sparse board
// the search is these loads: the census's pace.  The layout does not matter
// to the test (a non-zero word is a live word in either), nor do the zero
// words of the pitch padding a clipped row's last unit takes in.
template <int ILV>
__global__ __launch_bounds__(kFindThreads) void find_kernel(FindParams p, const uint32_t* __restrict__ cells) {
    const int lane = threadIdx.x & (kWaveLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWaveLanes));  // everything below it: scalar
    constexpr int kWaves = kFindThreads / kWaveLanes;
    const int32_t wave_id = (int32_t)blockIdx.x * kWaves + wave;  // launch_find: at most 2048 workgroups
    const int32_t nwaves = (int32_t)gridDim.x * kWaves;
    const int32_t xtiles = (p.sw + kWaveLanes - 1) / kWaveLanes;
    const int32_t xgroups = (xtiles + kGroupTiles - 1) / kGroupTiles;
    const int32_t nrows = p.a_hi - p.a_lo;
    const int wave_slot = wave_id % kFindSlots;
    // the first cell's row and the first word it reads, relative to a lane's first word
    const uint32_t first = cells[0];
    const int i0 = (int)(first & 63u);
    const int idx0 = (p.sh + (int)((first >> 8) & 63u)) >> 5;
    // item = (anchor row yt, group xg), row-major; a wave's next item is nwaves further: no division in the loop
    const int32_t dy = nwaves / xgroups, dx = nwaves % xgroups;
    int64_t yt = wave_id / xgroups;  // may pass `nrows`, itself below 2^31
    int32_t xg = wave_id % xgroups;
    while (yt < nrows) {
        unsigned live = 0u;  // bit u: item u exists and can hold a match (wave-uniform)
        int32_t arow[kFindProbe], group[kFindProbe];
#pragma unroll
        for (int u = 0; u < kFindProbe; ++u) {
            arow[u] = p.a_lo + (int32_t)min(yt, (int64_t)nrows - 1);
            group[u] = xg;
            if (yt < nrows) {  // past the last item it stays there: dy and dx do not move it back
                live |= 1u << u;
                yt += dy, xg += dx;
                if (xg >= xgroups) xg -= xgroups, ++yt;
            }
        }
        if (p.prefilter) {
            uint4 q[kFindProbe], q_next[kFindProbe];
#pragma unroll
            for (int u = 0; u < kFindProbe; ++u) {
                q[u] = q_next[u] = make_uint4(0u, 0u, 0u, 0u);
                if (!((live >> u) & 1u)) continue;
                const uint32_t* row = board_row(p, arow[u], i0);
                if (!row) continue;  // past a clipped board: dead
                // the unit that holds the item's first word, then one per lane: words [s0, s0 + 260) cover
                // the item's words [c, c + 257)
                const int32_t s0 = (p.c_first + group[u] * (kGroupTiles * kWaveLanes) + idx0) & ~3;
                const int32_t s = unit_index(s0 + 4 * lane, p.wwords, p.wrap_x);
                if (s >= 0) q[u] = *reinterpret_cast<const uint4*>(row + s);
                if (lane == kWaveLanes - 1) {
                    const int32_t t = unit_index(s0 + 4 * kWaveLanes, p.wwords, p.wrap_x);
                    if (t >= 0) q_next[u] = *reinterpret_cast<const uint4*>(row + t);
                }
            }
#pragma unroll
            for (int u = 0; u < kFindProbe; ++u) {
                const uint32_t any = q[u].x | q[u].y | q[u].z | q[u].w | q_next[u].x | q_next[u].y | q_next[u].z | q_next[u].w;
                if (__ballot(any != 0u) == 0ull) live &= ~(1u << u);
            }
        }
#pragma unroll
        for (int u = 0; u < kFindProbe; ++u) {
            if (!((live >> u) & 1u)) continue;
            for (int t = 0; t < kGroupTiles; ++t) {
                const int32_t tile = group[u] * kGroupTiles + t;
                if (tile >= xtiles) break;
                const int32_t m = tile * kWaveLanes + lane;
                // lanes past the window's last word follow the last one with no candidates
                const uint32_t mask = m < p.sw - 1 ? 0xFFFFFFFFu : m == p.sw - 1 ? p.last_mask : 0u;
                const uint32_t cand = match_row<ILV>(p, cells, arow[u], p.c_first + min(m, p.sw - 1), mask);
                if (__ballot(cand != 0u) != 0ull) emit(p, cand, arow[u], p.x0 + 32 * (int64_t)m, wave_slot);
            }
        }
    }
}

static_assert(kFindSlots == kWaveLanes, "one counter per lane of the fold");
// One wave: lane k takes counter k and leaves zero behind, the wave sums them,
// lane 0 stores the count and the hit list's cursor (zeroed too) to `out` --
// mapped page-locked host memory, read after the stream synchronises.
__global__ __launch_bounds__(kWaveLanes) void find_fold_kernel(unsigned long long* slots, unsigned long long* out) {
    unsigned long long* slot = slots + (size_t)threadIdx.x * kFindSlotStride;
    unsigned long long n = *slot;
    if (n != 0ull) *slot = 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, kWaveLanes);
    if (threadIdx.x == 0) {  // vector stores
        out[0] = n;
        out[1] = slots[kFindCursorWord];
        slots[kFindCursorWord] = 0ull;
    }
}

// Workgroups of find_kernel<ILV> the device holds at once: the grid is no
// larger, so every workgroup is resident from the start and none runs alone
// behind the others (asked of the first device used: the parts of a node are alike).
template <int ILV>
int resident_find_blocks() {
    static int cached = 0;
    if (cached > 0) return cached;
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, find_kernel<ILV>, kFindThreads, 0) != hipSuccess ||
        cus < 1 || per_cu < 1) {
        (void)hipGetLastError();  // a failed query leaves its status on the thread: taken off
        return 1024;
    }
    return cached = cus * per_cu;
}

}  // namespace

hipError_t launch_find(const FindParams& p, int ilv, hipStream_t stream) {
    // every index the kernel forms stays inside the plane, the list and the hit list
    if ((ilv != 1 && ilv != 2) || !p.plane || !p.cells || !p.slots || p.ncells < 1 || p.ncells > 64 * 64 ||
        p.rows < 1 || p.wwords < 1 || p.wwords % ilv != 0 || p.pitch < p.wwords || p.pitch % 2 != 0 ||
        (reinterpret_cast<uintptr_t>(p.plane) & 7) != 0 || p.a_lo < 0 || p.a_lo >= p.a_hi || p.a_hi > p.rows ||
        p.sw < 1 || p.sw > p.wwords || p.c_first < 0 || p.c_first >= p.wwords || p.sh < 0 || p.sh > 31 || p.nw < 1 ||
        p.nw > 4 || p.max_hits < 0 || (p.max_hits > 0 && !p.hits) || (p.max_hits == 0 && p.hits) ||
        (p.wrap_x && p.width != 32 * (int64_t)p.wwords) ||
        // the prefilter's 16-byte loads: aligned rows that hold whole units, which wrap whole
        (p.prefilter && (p.pitch % 4 != 0 || p.pitch < (p.wwords + 3) / 4 * 4 ||
                         (reinterpret_cast<uintptr_t>(p.plane) & 15) != 0 || (p.wrap_x && p.wwords % 4 != 0))))
        return hipErrorInvalidValue;
    const int32_t xtiles = (p.sw + kWaveLanes - 1) / kWaveLanes;
    const int64_t items = (int64_t)(p.a_hi - p.a_lo) * ((xtiles + kGroupTiles - 1) / kGroupTiles);
    constexpr int kWaves = kFindThreads / kWaveLanes;
    // as many workgroups as are resident at once (at most 2048: find_kernel's 32-bit wave index), the rest by
    // grid stride
    const int resident = std::min(ilv == 2 ? resident_find_blocks<2>() : resident_find_blocks<1>(), 2048);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((items + kWaves - 1) / kWaves, resident));
    if (ilv == 2) return launch_kernel(find_kernel<2>, dim3(blocks), dim3(kFindThreads), stream, p, p.cells);
    return launch_kernel(find_kernel<1>, dim3(blocks), dim3(kFindThreads), stream, p, p.cells);
}

hipError_t launch_find_fold(unsigned long long* slots, unsigned long long* out, hipStream_t stream) {
    return launch_kernel(find_fold_kernel, dim3(1), dim3(kWaveLanes), stream, slots, out);
}

}  // namespace gol
