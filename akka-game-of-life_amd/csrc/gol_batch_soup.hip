// gol_batch_soup.hip -- the batch engine's soup kernel (gol_soup_batch in
// gol_batch.cpp): boards first .. first + count - 1 of a
// batch become random soups -- a window of any density in a dead board, under
// one of nine symmetries, soup number index0 + board a pure function of the
// seed and that number.
//
// batch_soup_kernel: the lane mapping of the step kernel (one 64-bit row per
// lane, k = 64 / height whole boards per wave), counted from board `first`.
// Per lane:
//   raw row     the eight splitmix64 words of the lane's window row and the
//               bit-sliced comparator t < density over them (gol_soup.h's
//               raw_row, the host generator's): the density is scalar, so
//               eight 64-bit operations and no per-cell work;
//   domain      the row masked to the group's fundamental domain, whose row
//               masks the host computed from the spec (p.domain): every orbit
//               keeps exactly one cell;
//   images      per step of the group (gol_soup.h's steps: at most three) the
//               row ORed with its image under the step's map --
//                 T  w permutes (pairs, where w > 32): bit u of the lane that
//                    holds window row v is bit v of the lane that holds row u;
//                 X  a 64-bit bit reversal and a shift, in the lane;
//                 Y  one permute pair from the lane that holds row h - 1 - v;
//               a source lane is always a window row of the lane's own board;
//   store       the row shifted to column x: one 8-byte store per active
//               lane, 0 outside the window.
// Idle lanes (past k * height, or of boards past the range) and the lanes
// outside the window compute along with an all-zero row and read their own
// lane; only active lanes store.  Every branch and loop condition is scalar
// (the step bits, w), so no lane branch surrounds a permute.  No LDS
// allocation, no scratch, no atomics.
#include "gol_batch.h"
#include "gol_batch_wave.h"
#include "gol_kernels.h"

namespace golbatch {

namespace {

__device__ __forceinline__ unsigned long long lane_read64(int byte_addr, unsigned long long v) {
    const uint32_t lo = lane_read(byte_addr, (uint32_t)v), hi = lane_read(byte_addr, (uint32_t)(v >> 32));
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

// The transpose of the w x w window held in the lanes row0_addr / 4 + u: bit u
// of the result is bit v of the row in that lane.  `stride` is 4 in the lanes
// that hold a window row and 0 in the others, whose row0_addr is their own
// lane (they read themselves, and their result is masked away by the caller).
// NARROW: w <= 32, the upper dwords are zero.  Every lane of the wave must be
// here.
template <bool NARROW>
__device__ __forceinline__ unsigned long long soup_transpose(unsigned long long m, int row0_addr, int stride, int v, int w) {
    unsigned long long t = 0ull;
    int addr = row0_addr;
    for (int u = 0; u < w; ++u) {  // scalar
        unsigned long long r;
        if constexpr (NARROW) r = (unsigned long long)lane_read(addr, (uint32_t)m);
        else r = lane_read64(addr, m);
        t |= ((r >> v) & 1ull) << u;
        addr += stride;
    }
    return t;
}

__global__ __launch_bounds__(kLanes* kWavesPerWG) void batch_soup_kernel(const SoupParams p) {
    const int lane = threadIdx.x & (kLanes - 1);
    const int32_t i0 = wave_index() * p.boards_per_wave;  // the wave's first board, counted from p.first
    if (i0 >= p.count) return;  // the grid's last workgroup: wave-uniform, and nothing below synchronises
    const int H = p.height;
    const int bl = lane / H, y = lane - bl * H;
    const int32_t i = i0 + bl;
    const bool active = bl < p.boards_per_wave && i < p.count;
    const int32_t board = p.first + i;                          // active lanes: < first + count <= boards
    const size_t idx = (size_t)board * (size_t)H + (size_t)y;  // active lanes: < boards * height
    const gol_soup_spec& s = p.spec;
    const int vy = y - s.y;
    const bool inwin = active && vy >= 0 && vy < s.h;
    const int v = inwin ? vy : 0;  // 0 .. h - 1 <= 63 in every lane

    const unsigned long long soup = s.index0 + (unsigned long long)(long long)board;
    const unsigned long long raw = golsoup::raw_row(s.seed, s.density, soup, v);
    unsigned long long m = inwin ? raw & p.domain[v] : 0ull;

    // the lane that holds window row 0 of this lane's board, and the one that holds row h - 1 - v
    const int row0 = lane - y + s.y;
    const int row0_addr = 4 * (inwin ? row0 : lane), stride = inwin ? 4 : 0;
    const int flip_addr = 4 * (inwin ? row0 + (s.h - 1 - v) : lane);
    const int xshift = 64 - s.w;  // 0 .. 63

#pragma nounroll
    for (int k = 0; k < golsoup::kSteps; ++k) {
        const uint32_t step = (p.steps >> (3 * k)) & 7u;  // scalar
        if (step == 0u) break;
        unsigned long long img = m;
        if (step & golsoup::kStepT) {
            const unsigned long long t = s.w <= 32 ? soup_transpose<true>(img, row0_addr, stride, v, s.w)
                                                   : soup_transpose<false>(img, row0_addr, stride, v, s.w);
            img = inwin ? t : 0ull;
        }
        if (step & golsoup::kStepX) img = __builtin_bitreverse64(img) >> xshift;
        if (step & golsoup::kStepY) img = lane_read64(flip_addr, img);
        m |= img;
    }

    if (active) p.plane[idx] = m << s.x;  // x + w <= width <= 64: no bit is lost
}

}  // namespace

hipError_t launch_batch_soup(const SoupParams& p, hipStream_t stream) {
    // every index the kernel forms stays inside the plane and the domain words, every source lane inside the wave
    if (!launch_geometry_ok(p.boards, p.width, p.height, p.boards_per_wave) || !p.plane || !p.domain ||
        golsoup::soup_args(p.width, p.height, p.boards, &p.spec, p.first, p.count) != nullptr)
        return hipErrorInvalidValue;
    SoupParams q = p;
    q.steps = golsoup::steps(p.spec.symmetry);
    return gol::launch_kernel(batch_soup_kernel, launch_grid(p.height, p.count), dim3(kLanes * kWavesPerWG), stream, q);
}

}  // namespace golbatch
