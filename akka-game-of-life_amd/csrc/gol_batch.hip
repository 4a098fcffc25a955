// gol_batch.hip -- the batch engine's kernels (gol_batch_* in gol_batch.cpp;
// DESIGN.md section 5f): many independent boards of at most 64 x 64 stored
// cells, one 64-bit row per lane, k = 64 / height whole boards per wave.
//
// batch_step_kernel: one 8-byte load per lane, a run-time loop over the
// launch's generations entirely in registers, one store (with settle
// detection one more, the plane of the generation before).  No LDS traffic
// but the cross-lane permutes, no scratch.  Per generation:
//   vertical neighbours   torus, height 64: the DPP wave rotates;
//                         torus, height < 64: ds_bpermute_b32 from source
//                         lanes computed once (the board's own last / first
//                         row at its seams);
//                         clipped: the zero-filling DPP wave shifts of the
//                         row masked to its visible cells, dead at the seams;
//   horizontal neighbours shifts of the 64-bit column sums as two dwords; on
//                         a torus bit width - 1 wraps to bit 0 and back; boards
//                         of at most 32 columns run a loop without the upper dword;
//   count and rule        gol_stencil.h's bit-sliced adders and rule circuits
//                         (column sums first, as step_kernel);
//   population (POP)      popcount of the lane's row, a DPP prefix sum over
//                         the wave, one permute: the board's last lane
//                         subtracts the prefix before its board and stores
//                         (gol_batch_wave.h's BoardSum);
//   settle (SETTLE)       the row against the row of two generations ago, a
//                         ballot masked to the board's lanes.
// The generation itself is gol_batch_gen.h's, shared with batch_cycle_kernel
// (below: the same loops with cycle detection, early exit and fast-forward).
// Both kernels have RULES instances: every board under
// a rule word of its own, scalar masks where a wave is one board, per-lane
// conditions where it holds several -- the same loop bodies either way.
// Idle lanes (past k * height, or of boards past the batch) compute along --
// the loop has no lane branch around a cross-lane operation, so DPP and
// permutes see every lane -- and contribute to nothing: active lanes never read them (torus) or read them as
// dead rows (clipped), and they neither store, sum nor vote.
#include "gol_batch.h"
#include "gol_batch_gen.h"
#include "gol_stencil.h"

namespace golbatch {

namespace {

// The rule a RULES instance hands the generation in p's place (P: birth, survive).
struct RuleMasks {
    uint32_t birth, survive;
};
__device__ __forceinline__ RuleMasks rule_masks(uint32_t word) { return RuleMasks{word & 0x1FFu, (word >> 16) & 0x1FFu}; }

// RULES: every board under its own rule word,
// p.rules[board], loaded once before the loop (idle lanes take 0).  LIFE means
// nothing then: the generic adder runs.
template <bool LIFE, bool CLIPPED, bool POP, bool SETTLE, bool RULES = false>
__global__ __launch_bounds__(kLanes* kWavesPerWG) void batch_step_kernel(const StepParams p) {
    static_assert(!(RULES && LIFE), "the RULES instances are generic");
    const int lane = threadIdx.x & (kLanes - 1);
    const int32_t board0 = wave_index() * p.boards_per_wave;
    if (board0 >= p.boards) return;  // the grid's last workgroup: wave-uniform, and nothing below synchronises
    const int H = p.height;
    const int bl = lane / H, y = lane - bl * H;
    const int32_t board = board0 + bl;
    const bool active = bl < p.boards_per_wave && board < p.boards;
    const size_t idx = (size_t)board * (size_t)H + (size_t)y;  // active lanes: < boards * height

    const unsigned long long wmask = p.width >= 64 ? ~0ull : (1ull << p.width) - 1ull;
    const uint32_t wm_lo = (uint32_t)wmask, wm_hi = (uint32_t)(wmask >> 32);
    // torus: bit width - 1 inside its dword (the lower one iff width <= 32: the NARROW loops below)
    const uint32_t wsh = (uint32_t)(p.width - 1) & 31u;
    // clipped: the lane's row as its neighbours see it, and whether it has a row above / below in its board
    uint32_t sm_lo = 0xFFFFFFFFu, sm_hi = 0xFFFFFFFFu, upm = 0xFFFFFFFFu, dnm = 0xFFFFFFFFu;
    if constexpr (CLIPPED) {
        const unsigned long long vmask = p.vis_w >= 64 ? ~0ull : (1ull << p.vis_w) - 1ull;
        const bool seen = active && y < p.vis_h;
        sm_lo = seen ? (uint32_t)vmask : 0u;
        sm_hi = seen ? (uint32_t)(vmask >> 32) : 0u;
        upm = y > 0 ? 0xFFFFFFFFu : 0u;
        dnm = y < H - 1 ? 0xFFFFFFFFu : 0u;
    }
    // torus, height < 64: the lanes holding the rows above and below, inside the lane's own board
    const int up_addr = 4 * (active ? (y > 0 ? lane - 1 : lane + H - 1) : lane);
    const int dn_addr = 4 * (active ? (y < H - 1 ? lane + 1 : lane - (H - 1)) : lane);
    const GenConsts C{wm_lo, wm_hi, wsh, sm_lo, sm_hi, upm, dnm, up_addr, dn_addr};
    const BoardSum S(active, lane, y, H);  // population: the board's last lane stores
    // settle: the board's lanes in a ballot
    unsigned long long bm = ~0ull;
    if constexpr (SETTLE) {
        const unsigned long long hm = H >= 64 ? ~0ull : (1ull << H) - 1ull;
        bm = active ? hm << (bl * H) : ~0ull;
    }

    Row cur = {0u, 0u}, prev = {0u, 0u};
    uint32_t first = 0u;
    uint32_t word = 0u;  // RULES: the board's rule
    if (active) {
        const unsigned long long r = p.plane[idx];
        cur = {(uint32_t)r, (uint32_t)(r >> 32)};
        if constexpr (RULES) word = p.rules[board];
        if constexpr (SETTLE) {
            if (p.g0 > 0) {
                const unsigned long long q = p.prev[idx];
                prev = {(uint32_t)q, (uint32_t)(q >> 32)};
                first = p.settled[board];
            }
        }
    }

    // the four loops of gol_batch_gen.h's generation: rotates or permutes, wide or narrow; R: the rule (p, or a
    // RULES instance's masks)
    auto run = [&](auto ROT_, auto NARROW_, const auto& R) __attribute__((always_inline)) {
        constexpr bool ROT = decltype(ROT_)::value;
        constexpr bool NARROW = decltype(NARROW_)::value;
        if constexpr (NARROW) cur.hi = prev.hi = 0u;
        for (uint32_t g = 0; g < p.gens; ++g) {
            const Row nx = generation<LIFE, CLIPPED, ROT, NARROW>(R, C, cur);
            if constexpr (POP) {
                const uint32_t bits = (uint32_t)__builtin_popcount(nx.lo) + (NARROW ? 0u : (uint32_t)__builtin_popcount(nx.hi));
                const uint32_t pop = S.total(active ? bits : 0u);
                if (S.writer) p.pops[(size_t)board * p.pop_stride + g] = pop;
            }
            if constexpr (SETTLE) {
                const unsigned long long same = __ballot(nx.lo == prev.lo && (NARROW || nx.hi == prev.hi));
                const uint32_t gen = p.g0 + g + 1u;  // generation of the call that nx is
                if (gen >= 2u && first == 0u && (same & bm) == bm) first = gen;
                prev = cur;
            }
            cur = nx;
        }
    };
    // wave-uniform, outside the loop
    const bool rot = !CLIPPED && H == kLanes, narrow = p.width <= 32;
    if constexpr (!RULES) {  // written out, not shared with the paths below: so these instances keep their code
        if (rot && narrow) run(std::true_type{}, std::true_type{}, p);
        else if (rot) run(std::true_type{}, std::false_type{}, p);
        else if (narrow) run(std::false_type{}, std::true_type{}, p);
        else run(std::false_type{}, std::false_type{}, p);
    } else if (p.boards_per_wave == 1) {
        // the wave is one board (lane 0 is active): one rule, its masks scalar as the uniform generic instances'
        const RuleMasks R = rule_masks((uint32_t)__builtin_amdgcn_readfirstlane((int)word));
        if (rot && narrow) run(std::true_type{}, std::true_type{}, R);
        else if (rot) run(std::true_type{}, std::false_type{}, R);
        else if (narrow) run(std::false_type{}, std::true_type{}, R);
        else run(std::false_type{}, std::false_type{}, R);
    } else {
        // a rule per board, so per lane (rot needs height 64: the two permute loops); the rule is data, no branch
        const RuleMasks R = rule_masks(word);
        if (narrow) run(std::false_type{}, std::true_type{}, R);
        else run(std::false_type{}, std::false_type{}, R);
    }

    if (active) {
        p.plane[idx] = (unsigned long long)cur.lo | ((unsigned long long)cur.hi << 32);
        if constexpr (SETTLE) {
            p.prev[idx] = (unsigned long long)prev.lo | ((unsigned long long)prev.hi << 32);
            if (y == 0) p.settled[board] = first;
        }
    }
}

// batch_cycle_kernel (gol_cycle_step): batch_step_kernel's
// lane mapping and four loops, with Brent's cycle detection carried in
// registers -- the snapshot row, and per lane a copy of the generation its
// board's cycle was seen at (the period follows from it).  Per generation the new row against
// the snapshot, a ballot masked to the board's lanes; the snapshot is replaced
// at the generations 2^k - 1 of the call (scalar).  The main loop ends when
// every board of the wave has a period (idle lanes count as done); then each
// lane still owes (generations not run) mod period, and a second loop steps
// the whole wave while any lane owes one, keeping the new row by a select
// where the lane does.  Both loop conditions are ballots or scalars: no lane
// branch surrounds a DPP or permute.  A wave with an undetected board keeps
// stepping all its boards, which evolve truthfully.
template <bool LIFE, bool CLIPPED, bool RULES = false>
__global__ __launch_bounds__(kLanes* kWavesPerWG) void batch_cycle_kernel(const CycleParams p) {
    static_assert(!(RULES && LIFE), "the RULES instances are generic");
    const int lane = threadIdx.x & (kLanes - 1);
    const int32_t board0 = wave_index() * p.boards_per_wave;
    if (board0 >= p.boards) return;  // the grid's last workgroup: wave-uniform, and nothing below synchronises
    const Lane L = lane_of<CLIPPED>(p, lane, board0);
    const GenConsts C = L.consts();
    const unsigned long long bm = L.board_lanes();

    // `seen` alone is carried through the loops: the period is seen - (the snapshot generation seen is compared with)
    auto period_of = [](uint32_t seen_at) -> uint32_t {
        return seen_at ? seen_at - cycle_snapshot_generation(seen_at) : 0u;
    };
    Row cur = {0u, 0u}, snap = {0u, 0u};
    uint32_t seen = 1u;  // idle lanes: done with period 1, owing nothing
    uint32_t word = 0u;  // RULES: the board's rule
    if (L.active) {
        const unsigned long long r = p.plane[L.idx];
        cur = {(uint32_t)r, (uint32_t)(r >> 32)};
        seen = p.g0 > 0 ? p.seen[L.board] : 0u;
        if constexpr (RULES) word = p.rules[L.board];
    }
    const uint32_t seen_in = seen;
    // wave-uniform: some board of the wave has no period yet.  A later launch that finds none goes straight to the
    // fast-forward and touches neither the snapshot plane nor the per-board words.
    bool open = __builtin_amdgcn_ballot_w64(seen == 0u) != 0ull;
    const bool ran = open;
    if (ran) {
        snap = cur;  // the call's generation 0 is t_0
        if (L.active && p.g0 > 0) {
            const unsigned long long q = p.snap[L.idx];
            snap = {(uint32_t)q, (uint32_t)(q >> 32)};
        }
    }

    auto run = [&](auto ROT_, auto NARROW_, const auto& R) __attribute__((always_inline)) {
        constexpr bool ROT = decltype(ROT_)::value;
        constexpr bool NARROW = decltype(NARROW_)::value;
        if constexpr (NARROW) cur.hi = snap.hi = 0u;
        uint32_t g = 0u;  // scalar: generations run
        for (; g < p.gens && open; ++g) {
            const Row nx = generation<LIFE, CLIPPED, ROT, NARROW>(R, C, cur);
            const unsigned long long same =
                __builtin_amdgcn_ballot_w64(nx.lo == snap.lo && (NARROW || nx.hi == snap.hi));
            const uint32_t gen = p.g0 + g + 1u;  // generation of the call that nx is (<= 2^32 - 1)
            seen = seen == 0u && (same & bm) == bm ? gen : seen;
            if (cycle_is_snapshot(gen)) snap = nx;  // scalar
            cur = nx;
            open = __builtin_amdgcn_ballot_w64(seen == 0u) != 0ull;
        }
        // fast-forward: the loop above ended early only with a period in every lane; a board is on its cycle
        const uint32_t period = period_of(seen);
        uint32_t left = (p.gens - g) % (period ? period : 1u);
        while (__builtin_amdgcn_ballot_w64(left > 0u) != 0ull) {
            const Row nx = generation<LIFE, CLIPPED, ROT, NARROW>(R, C, cur);
            const bool owes = left > 0u;
            cur.lo = owes ? nx.lo : cur.lo;
            if constexpr (!NARROW) cur.hi = owes ? nx.hi : cur.hi;
            left -= owes ? 1u : 0u;
        }
    };
    // wave-uniform, outside the loops
    const bool rot = !CLIPPED && L.H == kLanes, narrow = p.width <= 32;
    if constexpr (!RULES) {  // written out, not shared with the paths below: so these instances keep their code
        if (rot && narrow) run(std::true_type{}, std::true_type{}, p);
        else if (rot) run(std::true_type{}, std::false_type{}, p);
        else if (narrow) run(std::false_type{}, std::true_type{}, p);
        else run(std::false_type{}, std::false_type{}, p);
    } else if (p.boards_per_wave == 1) {
        // the wave is one board (lane 0 is active): one rule, its masks scalar as the uniform generic instances'
        const RuleMasks R = rule_masks((uint32_t)__builtin_amdgcn_readfirstlane((int)word));
        if (rot && narrow) run(std::true_type{}, std::true_type{}, R);
        else if (rot) run(std::true_type{}, std::false_type{}, R);
        else if (narrow) run(std::false_type{}, std::true_type{}, R);
        else run(std::false_type{}, std::false_type{}, R);
    } else {
        // a rule per board, so per lane (rot needs height 64: the two permute loops); the rule is data, no branch
        const RuleMasks R = rule_masks(word);
        if (narrow) run(std::false_type{}, std::true_type{}, R);
        else run(std::false_type{}, std::false_type{}, R);
    }

    if (L.active) {
        p.plane[L.idx] = (unsigned long long)cur.lo | ((unsigned long long)cur.hi << 32);
        if (ran) {
            p.snap[L.idx] = (unsigned long long)snap.lo | ((unsigned long long)snap.hi << 32);
            if (L.y == 0) {
                const uint32_t period = period_of(seen);
                p.period[L.board] = period;
                p.seen[L.board] = seen;
                if (seen_in == 0u && seen != 0u) {  // one lane per newly detected board
                    atomicAdd(&p.counters[0], 1u);
                    atomicMax(&p.counters[1], period);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void batch_seed_kernel(unsigned long long* plane, int64_t words,
                                                          unsigned long long wmask, unsigned long long seed) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= words) return;
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)k + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    plane[k] = z & wmask;
}

// One thread per board: the state hash of include/gol.h with row0 = 0 and the
// one column group 0 -- E the row's even columns, O its odd ones -- and the
// population.  Off the step's path: a board's rows are read by one lane.
__global__ __launch_bounds__(256) void batch_hash_kernel(const unsigned long long* plane, int32_t height,
                                                          int64_t first, int64_t count, unsigned long long* hashes,
                                                          uint32_t* pops) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const unsigned long long* rows = plane + (size_t)(first + i) * (size_t)height;
    unsigned long long h = 0ull;
    uint32_t n = 0u;
    for (int y = 0; y < height; ++y) {
        const unsigned long long r = rows[y];
        const uint32_t u0 = unzip_bits((uint32_t)r), u1 = unzip_bits((uint32_t)(r >> 32));
        const uint32_t e = (u0 & 0xFFFFu) | (u1 << 16), o = (u0 >> 16) | (u1 & 0xFFFF0000u);
        const uint32_t ae = gol::hash_row_key(y);
        h += (unsigned long long)e * ae + (unsigned long long)o * (uint32_t)(ae + gol::kHashOddAdd);
        n += (uint32_t)__builtin_popcountll(r);
    }
    if (hashes) hashes[i] = h * (unsigned long long)gol::hash_pair_key(0u);
    if (pops) pops[i] = n;
}

template <bool LIFE, bool CLIPPED, bool RULES = false>
hipError_t launch_step_flags(const StepParams& p, dim3 grid, hipStream_t stream) {
    const dim3 block(kLanes * kWavesPerWG);
    const bool pop = p.pops != nullptr, settle = p.settled != nullptr;
    if (pop && settle)
        return gol::launch_kernel(batch_step_kernel<LIFE, CLIPPED, true, true, RULES>, grid, block, stream, p);
    if (pop) return gol::launch_kernel(batch_step_kernel<LIFE, CLIPPED, true, false, RULES>, grid, block, stream, p);
    if (settle) return gol::launch_kernel(batch_step_kernel<LIFE, CLIPPED, false, true, RULES>, grid, block, stream, p);
    return gol::launch_kernel(batch_step_kernel<LIFE, CLIPPED, false, false, RULES>, grid, block, stream, p);
}

}  // namespace

hipError_t launch_batch_step(const StepParams& p, bool life, bool clipped, bool rules, hipStream_t stream) {
    // every index the kernel forms stays inside the plane, the series, the settle words and the rule words
    if (!launch_geometry_ok(p.boards, p.width, p.height, p.boards_per_wave, clipped, p.vis_w, p.vis_h) ||
        rules != (p.rules != nullptr) || !p.plane || p.gens < 1 || (p.pops && p.pop_stride < p.gens) ||
        (p.settled && !p.prev))
        return hipErrorInvalidValue;
    const dim3 grid = launch_grid(p.height, p.boards);
    if (rules)
        return clipped ? launch_step_flags<false, true, true>(p, grid, stream)
                       : launch_step_flags<false, false, true>(p, grid, stream);
    if (life) return clipped ? launch_step_flags<true, true>(p, grid, stream) : launch_step_flags<true, false>(p, grid, stream);
    return clipped ? launch_step_flags<false, true>(p, grid, stream) : launch_step_flags<false, false>(p, grid, stream);
}

hipError_t launch_batch_cycle(const CycleParams& p, bool life, bool clipped, bool rules, hipStream_t stream) {
    // every index the kernel forms stays inside the two planes, the per-board words and the rule words
    if (!launch_geometry_ok(p.boards, p.width, p.height, p.boards_per_wave, clipped, p.vis_w, p.vis_h) ||
        rules != (p.rules != nullptr) || !p.plane || !p.snap || !p.period || !p.seen || !p.counters || p.gens < 1 ||
        p.gens > UINT32_MAX - p.g0)
        return hipErrorInvalidValue;
    const dim3 grid = launch_grid(p.height, p.boards), block(kLanes * kWavesPerWG);
    if (rules)
        return clipped ? gol::launch_kernel(batch_cycle_kernel<false, true, true>, grid, block, stream, p)
                       : gol::launch_kernel(batch_cycle_kernel<false, false, true>, grid, block, stream, p);
    if (life)
        return clipped ? gol::launch_kernel(batch_cycle_kernel<true, true>, grid, block, stream, p)
                       : gol::launch_kernel(batch_cycle_kernel<true, false>, grid, block, stream, p);
    return clipped ? gol::launch_kernel(batch_cycle_kernel<false, true>, grid, block, stream, p)
                   : gol::launch_kernel(batch_cycle_kernel<false, false>, grid, block, stream, p);
}

hipError_t launch_batch_seed(unsigned long long* plane, int64_t words, int32_t width, uint64_t seed,
                             hipStream_t stream) {
    if (!plane || words < 1 || width < 1 || width > kLanes) return hipErrorInvalidValue;
    const unsigned long long wmask = width >= 64 ? ~0ull : (1ull << width) - 1ull;
    return gol::launch_kernel(batch_seed_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), stream, plane, words,
                              wmask, (unsigned long long)seed);
}

hipError_t launch_batch_hashes(const unsigned long long* plane, int32_t height, int64_t first, int64_t count,
                               unsigned long long* hashes, uint32_t* pops, hipStream_t stream) {
    if (!plane || height < 1 || height > kLanes || first < 0 || count < 1 || (!hashes && !pops))
        return hipErrorInvalidValue;
    return gol::launch_kernel(batch_hash_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), stream, plane, height,
                              first, count, hashes, pops);
}

}  // namespace golbatch
