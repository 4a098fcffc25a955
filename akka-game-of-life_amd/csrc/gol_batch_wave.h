// gol_batch_wave.h -- what the batch engine's kernels share that is not the
// stencil (DESIGN.md sections 5f to 5j): the DPP prefix sum over a wave, the
// lane read, a wave's index in the grid and the per-board sum.  gol_batch_gen.h
// includes it; gol_batch_census.hip includes it alone, so that unit stays
// without gol_stencil.h.  Everything is force-inlined: the kernels keep their
// instruction streams (make asm-batch and its three siblings).  Device code
// only; not installed.
#pragma once
#include "gol_batch.h"

namespace golbatch {

constexpr int kDppRowShr = 0x110;      // row_shr:n = kDppRowShr + n (rows of 16 lanes)
constexpr int kDppRowBcast15 = 0x142;  // lane 15 of each row -> the next row
constexpr int kDppRowBcast31 = 0x143;  // lane 31 -> rows 2 and 3

// v + (v of the DPP source lane, 0 where there is none or the row is masked out)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}

// Inclusive prefix sum over the wave's 64 lanes: four shifts inside the rows
// of 16, then the two row broadcasts.  Every lane of the wave must be here.
__device__ __forceinline__ uint32_t wave_prefix_sum(uint32_t v) {
    v = dpp_add<kDppRowShr + 1, 0xf>(v);
    v = dpp_add<kDppRowShr + 2, 0xf>(v);
    v = dpp_add<kDppRowShr + 4, 0xf>(v);
    v = dpp_add<kDppRowShr + 8, 0xf>(v);
    v = dpp_add<kDppRowBcast15, 0xa>(v);
    v = dpp_add<kDppRowBcast31, 0xc>(v);
    return v;
}

__device__ __forceinline__ uint32_t lane_read(int byte_addr, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(byte_addr, (int)v);
}

// The wave's index in a grid of kWavesPerWG-wave workgroups, a scalar.
__device__ __forceinline__ int32_t wave_index() {
    const int wave_in_wg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kLanes));
    return (int32_t)blockIdx.x * kWavesPerWG + wave_in_wg;  // waves <= boards <= 2^22
}

// A sum over the lanes of a board (lane `lane` holds row y of its board's H,
// `active`: it holds one at all): the board's last lane has the wave's prefix
// sum up to itself, and the prefix before the board is the one of the lane
// before its first (none before lane 0).  So that last lane is the board's
// writer, and it alone gets the total.
struct BoardSum {
    bool writer, has_before;
    int before_addr;  // the lane to read the prefix before the board from (the lane itself where there is none)
    __device__ __forceinline__ BoardSum(bool active, int lane, int y, int H) {
        writer = active && y == H - 1;
        const int first_lane = lane - (H - 1);
        has_before = writer && first_lane > 0;
        before_addr = 4 * (has_before ? first_lane - 1 : lane);
    }
    // The board's total of v (idle lanes pass 0), valid in the writer lane.  Every lane of the wave must be here.
    __device__ __forceinline__ uint32_t total(uint32_t v) const {
        const uint32_t incl = wave_prefix_sum(v);
        const uint32_t before = lane_read(before_addr, incl);
        return incl - (has_before ? before : 0u);
    }
};

}  // namespace golbatch
