// gol_batch_find.hip -- pattern search on a batch (gol_find_batch in
// gol_batch.cpp): a list of patterns matched against
// every board of a batch in one launch, on the batch engine's lane mapping
// (gol_batch.h batch_lanes: one 64-bit row per lane, k = 64 / height whole
// boards per wave).  A unit of its own; what it has in common with the other
// batch units comes from gol_batch_gen.h and gol_batch_wave.h.
//
// batch_find_kernel: one 8-byte load per lane, then a wave-uniform loop over
// the launch's patterns and, inside it, over a pattern's rows.  The pattern
// table is read through wave-uniform loads: a row's (cells, care) pair, the
// cared columns and the shift distances are scalars.  Per pattern row i
//   row fetch   the board's row y + i by ds_bpermute_b32 (two dwords) from
//               lane l + i; on a torus the board's own first rows, `height`
//               lanes back, past its last row; on a clipped board zero there.
//               Never another board's lane.
//   matching    cand holds one bit per anchor x of the lane's row y.  For each
//               cared column k: cand &= shift_k(row) ^ inv, shift_k the rotate
//               right by k within `width` (torus) or the plain shift (clipped:
//               the plane holds no bit at x >= width, so cells past the board
//               read dead), inv all ones where the pattern cell is dead.
//   early exit  when no lane of the wave has a candidate left (a ballot).
// Per pattern: popcount of cand, batch_step_kernel's segmented sum (BoardSum:
// a DPP prefix over the wave and one permute), one uint32 store by the board's
// last lane; with match planes one 8-byte store of cand per lane.  No atomics, no
// LDS allocation, no scratch.
// Idle lanes (past k * height, or of boards past the batch) compute along with
// cand = 0 -- no lane branch surrounds a permute or DPP operation -- and
// neither store nor sum; active lanes never read them.
#include "gol_batch.h"
#include "gol_batch_gen.h"

namespace golbatch {

namespace {

template <bool CLIPPED>
__global__ __launch_bounds__(kLanes* kWavesPerWG) void batch_find_kernel(
    const FindParams p, const FindPattern* __restrict__ patterns, const unsigned long long* __restrict__ table_rows) {
    // the table ([npatterns] headers; the row array, 2 qwords per pattern row) comes as arguments of its own that
    // nothing the kernel stores to aliases: what lets it be read with scalar loads
    const int lane = threadIdx.x & (kLanes - 1);
    const int32_t board0 = wave_index() * p.boards_per_wave;
    if (board0 >= p.boards) return;  // the grid's last workgroup: wave-uniform, and nothing below synchronises
    const Lane L = lane_of<false>(p, lane, board0);  // the mapping alone: the topology enters at the row fetch
    const int H = L.H;
    const unsigned long long wmask = p.width >= 64 ? ~0ull : (1ull << p.width) - 1ull;
    const int wsh = p.width - 1;

    unsigned long long mine = 0ull;
    if (L.active) mine = p.plane[L.idx];
    const uint32_t mine_lo = (uint32_t)mine, mine_hi = (uint32_t)(mine >> 32);
    const BoardSum S(L.active, lane, L.y, H);  // counting: the board's last lane stores

    for (int32_t q = 0; q < p.count; ++q) {
        const int32_t pi = p.first + q;
        const FindPattern fp = patterns[pi];
        unsigned long long cand = L.active ? wmask : 0ull;  // every anchor of the stored row
        for (int32_t i = 0; i < fp.ph; ++i) {
            const unsigned long long* pr = table_rows + 2 * ((size_t)fp.row0 + (size_t)i);
            const unsigned long long cells = pr[0], care = pr[1];
            if (care == 0ull) continue;  // scalar: a row that cares for nothing
            // the board's row y + i (i < ph <= height: one wrap at most); source lanes stay in 0 .. 63 and in the board
            const int yy = L.y + i;
            int src = lane;
            bool dead = false;
            if constexpr (CLIPPED) {
                dead = yy >= H;
                if (L.active && !dead) src = lane + i;
            } else {
                if (L.active) src = yy >= H ? lane + i - H : lane + i;
            }
            const uint32_t lo = lane_read(4 * src, mine_lo), hi = lane_read(4 * src, mine_hi);
            const unsigned long long r = dead ? 0ull : (unsigned long long)lo | ((unsigned long long)hi << 32);
            unsigned long long c = care;  // scalar: the cared columns still to do
            do {
                const int k = __builtin_ctzll(c);  // 0 <= k < pw <= width
                c &= c - 1ull;
                const unsigned long long inv = (cells >> k) & 1ull ? 0ull : ~0ull;
                unsigned long long sh = r >> k;
                // torus: columns 0 .. k - 1 come round to bits width - k ..; shifted by 1 and by width - 1 - k
                // (0 .. 63 each), as width - k is 64 for k = 0 on a board of 64 columns.  Bits at x >= width may be
                // set in sh and in inv: cand has none and keeps none.
                if constexpr (!CLIPPED) sh |= (r << 1) << (wsh - k);
                cand &= sh ^ inv;
            } while (c != 0ull);
            if (__builtin_amdgcn_ballot_w64(cand != 0ull) == 0ull) break;  // wave-uniform
        }
        const uint32_t found = S.total((uint32_t)__builtin_popcountll(cand));  // idle lanes: cand = 0
        if (S.writer) p.counts[(size_t)L.board * (size_t)p.npatterns + (size_t)pi] = found;
        if (p.matches != nullptr && L.active)
            p.matches[((size_t)pi * (size_t)p.boards + (size_t)L.board) * (size_t)H + (size_t)L.y] = cand;
    }
}

}  // namespace

hipError_t launch_batch_find(const FindParams& p, const FindPattern* patterns, const unsigned long long* rows,
                             bool clipped, hipStream_t stream) {
    // every index the kernel forms stays inside the plane, the pattern headers, the counts and the match planes
    if (!launch_geometry_ok(p.boards, p.width, p.height, p.boards_per_wave) || !p.plane || !patterns || !rows ||
        !p.counts || p.npatterns < 1 || p.npatterns > kMaxFindPatterns || p.first < 0 || p.count < 1 ||
        p.count > p.npatterns - p.first)
        return hipErrorInvalidValue;
    const dim3 grid = launch_grid(p.height, p.boards), block(kLanes * kWavesPerWG);
    return clipped ? gol::launch_kernel(batch_find_kernel<true>, grid, block, stream, p, patterns, rows)
                   : gol::launch_kernel(batch_find_kernel<false>, grid, block, stream, p, patterns, rows);
}

}  // namespace golbatch
