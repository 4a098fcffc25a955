// gol_layout.h -- the pair layout's bit shuffles (DESIGN.md "Data layout";
// oracle/gol_oracle.c oracle_to_pairs), shared by gol_misc.hip (seeding,
// conversion) and gol_region.hip (windows, census): row-major words
// (w0, w1) = columns 0..31, 32..63 of a pair <-> (e, o) = their even and odd
// columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gol {

__device__ __forceinline__ uint32_t even_bits(uint32_t x) {  // bits 0, 2, .., 30 -> 0 .. 15
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
__device__ __forceinline__ uint32_t spread_bits(uint32_t x) {  // bits 0 .. 15 -> 0, 2, .., 30
    x &= 0x0000FFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// Device word j of the pair whose row-major words are w[0..2).
__device__ __forceinline__ uint32_t device_word(const uint32_t* w, int j) {
    return even_bits(w[0] >> j) | (even_bits(w[1] >> j) << 16);
}
// Row-major word i of the pair whose device words are q[0..2).
__device__ __forceinline__ uint32_t row_major_word(const uint32_t* q, int i) {
    return spread_bits(q[0] >> (16 * i)) | (spread_bits(q[1] >> (16 * i)) << 1);
}

}  // namespace gol
