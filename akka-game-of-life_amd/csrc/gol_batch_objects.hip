// gol_batch_objects.hip -- the objects of every board of a batch
// (gol_objects_batch in gol_batch.cpp): each board cut
// into the connected components of its live cells, two cells linked iff their
// Chebyshev distance is at most `reach`, and per component one 16-byte record
// (translation-invariant hash, bounding box, population), on the batch
// engine's lane mapping (gol_batch.h batch_lanes: one 64-bit row per lane,
// k = 64 / height whole boards per wave).  A unit of its own; what it has in
// common with the other batch units comes from gol_batch_gen.h and
// gol_batch_wave.h.
//
// batch_objects_kernel: one 8-byte load per lane; `rem`, the board's cells not
// yet given to an object, stays in registers.  While any lane of the wave has
// a cell left (a ballot):
//   seed      per board the first lane with cells left (the ballot masked to
//             the board's lanes, its lowest bit); that lane alone seeds the
//             fill with its lowest cell.  A board with nothing left carries an
//             empty fill through the rest and produces nothing.
//   fill      f <- dilate^reach(f) & rem until no lane of the wave changes (a
//             ballot).  dilate: f | up | down, then | west | east of that.
//             Vertical neighbours as the step kernels get them (wave rotates
//             at height 64 on a torus, ds_bpermute through up_addr / dn_addr
//             on shorter tori, zero-filling DPP shifts masked by upm / dnm on
//             clipped boards: never another board's lane); horizontal ones by
//             the 64-bit-in-two-dwords shifts, on a torus with the wrap
//             between bit width - 1 and bit 0.  No run fill inside a row: a
//             step grows the fill by `reach` cells in every direction.
//   summary   row span: the ballot of f != 0 masked to the board; column
//             mask: an OR over the board's lanes (OR is idempotent: ceil(log2
//             height) doublings of "OR with the lane 2^s further on,
//             cyclically inside the board"); the box from the two masks
//             (span_of); population and hash: segmented sums (a DPP prefix
//             over the wave and one permute each; the 64-bit row terms go as
//             three limbs whose wave sums stay below 2^32); the board's last
//             lane stores the record with one 16-byte store if it has room,
//             and every lane of the board counts the object and takes it out
//             of rem.
// At the end the board's last lane stores the board's count.
//
// Why the loops end: a fill only grows and is bounded by rem, so it ends after
// at most (its cells + 1) steps; every object takes at least one cell out of
// rem, so a wave starts at most 4096 fills and runs at most 4096 + 4096 = 8192
// fill steps over all of them, whatever the boards hold.
// Every loop condition is a scalar or a ballot, no lane branch surrounds a DPP
// move or a permute, idle lanes (past k * height, or of boards past the range)
// compute along with empty rows and neither store nor vote.  No LDS
// allocation, no atomics, no scratch, plain vector stores only.
#include "gol_batch.h"
#include "gol_batch_gen.h"

namespace golbatch {

namespace {

using u64 = unsigned long long;

__device__ __forceinline__ int lowest_bit(u64 v) { return v ? __builtin_ctzll(v) : 0; }
__device__ __forceinline__ int bits_used(u64 v) { return v ? 64 - __builtin_clzll(v) : 0; }  // highest bit + 1

// An occupancy mask m of n bits (the object's columns, or its rows) as the
// box's (start, extent) on that axis.  Clipped: the plain minimum and maximum.
// Torus: the occupied positions leave at most one cyclic run of at least
// `reach` empty ones (two would disconnect the object); the box starts after
// it -- the one bit of m whose `reach` cyclic predecessors are all empty --
// and is n minus its length long; without such a run the object goes round:
// start 0, extent n.  n >= 3 on a torus, so the rotates by 1 and 2 are proper.
template <bool CLIPPED>
__device__ __forceinline__ void span_of(u64 m, int n, int reach, int& start, int& extent) {
    if constexpr (CLIPPED) {
        start = lowest_bit(m);
        extent = bits_used(m) - start;
    } else {
        const u64 nm = n >= 64 ? ~0ull : (1ull << n) - 1ull;
        const u64 e = ~m & nm;
        u64 s = m & (((e << 1) | (e >> (n - 1))) & nm);
        if (reach == 2) s &= ((e << 2) | (e >> (n - 2))) & nm;  // scalar
        start = lowest_bit(s);
        // m rotated right by start (0 .. n - 1; (m << 1) << (n - 1 - start) is m << (n - start) without a shift by 64)
        const u64 mr = ((m >> start) | ((m << 1) << (n - 1 - start))) & nm;
        extent = s ? bits_used(mr) : n;
    }
}

// ROT: the wave is one torus board of 64 rows
template <bool CLIPPED, bool ROT>
__device__ __forceinline__ Row dilate(const Lane& L, const Row& f, bool wide, uint32_t wsh) {
    Row a, b;
    if constexpr (CLIPPED) {
        a = {dpp_shr1_zero(f.lo) & L.upm, dpp_shr1_zero(f.hi) & L.upm};
        b = {dpp_shl1_zero(f.lo) & L.dnm, dpp_shl1_zero(f.hi) & L.dnm};
    } else if constexpr (ROT) {
        a = {dpp_ror1(f.lo), dpp_ror1(f.hi)};
        b = {dpp_rol1(f.lo), dpp_rol1(f.hi)};
    } else {
        a = {lane_read(L.up_addr, f.lo), lane_read(L.up_addr, f.hi)};
        b = {lane_read(L.dn_addr, f.lo), lane_read(L.dn_addr, f.hi)};
    }
    const Row v = {f.lo | a.lo | b.lo, f.hi | a.hi | b.hi};
    Row w = {v.lo << 1, __builtin_amdgcn_alignbit(v.hi, v.lo, 31)};  // column x - 1 at bit x
    Row e = {__builtin_amdgcn_alignbit(v.hi, v.lo, 1), v.hi >> 1};   // column x + 1 at bit x
    if constexpr (!CLIPPED) {  // bit width - 1 <-> bit 0; `wide` (width > 32: that bit is in the upper dword) is scalar
        w.lo |= ((wide ? v.hi : v.lo) >> wsh) & 1u;
        const uint32_t t = (v.lo & 1u) << wsh;
        e.lo |= wide ? 0u : t;
        e.hi |= wide ? t : 0u;
    }
    // bits at x >= width may be set here; the caller's `& rem` drops them, and what a second dilation makes of them
    // (bit width stands for column 0, which the wrap has set as well) is set anyway
    return {v.lo | w.lo | e.lo, v.hi | w.hi | e.hi};
}

template <bool CLIPPED>
__global__ __launch_bounds__(kLanes* kWavesPerWG) void batch_objects_kernel(const ObjectsParams p) {
    const int lane = threadIdx.x & (kLanes - 1);
    // the waves hold the range's boards from p.first on; p.boards is the range's end
    const int32_t board0 = p.first + wave_index() * p.boards_per_wave;
    if (board0 >= p.boards) return;  // the grid's last workgroup: wave-uniform, and nothing below synchronises
    const Lane L = lane_of<CLIPPED>(p, lane, board0);
    const int H = L.H;
    const u64 bm = L.board_lanes();
    const int board_sh = L.active ? L.bl * H : 0;  // the board's first lane
    const bool wide = p.width > 32;
    // the board's last lane sums and stores.  BoardSum's values as locals of the kernel, which the loop below
    // captures one by one: captured as the struct, one of its moves was placed two instructions later
    const BoardSum S(L.active, lane, L.y, H);
    const bool writer = S.writer, has_before = S.has_before;
    const int before_addr = S.before_addr;
    const size_t out = (size_t)(L.board - p.first);  // active lanes: < the range's boards

    Row rem = {0u, 0u};
    if (L.active) {
        const u64 r = p.plane[L.idx];
        rem = {(uint32_t)r, (uint32_t)(r >> 32)};
    }
    uint32_t n = 0u;  // the board's objects so far, the same in all its lanes

    auto run = [&](auto ROT_) __attribute__((always_inline)) {
        constexpr bool ROT = decltype(ROT_)::value;
        u64 left;  // the lanes that still hold cells
        while ((left = __builtin_amdgcn_ballot_w64((rem.lo | rem.hi) != 0u)) != 0ull) {
            // seed: the board's first lane with cells, its lowest cell (idle lanes hold none, so are never that lane)
            const u64 mine = left & bm;
            const bool seeded = L.active && mine != 0ull;
            const bool seeds = seeded && lane == lowest_bit(mine);
            Row f = {0u, 0u};
            if (seeds) {
                f.lo = rem.lo & (0u - rem.lo);
                f.hi = rem.lo ? 0u : rem.hi & (0u - rem.hi);
            }
            // fill: at most (the object's cells + 1) steps, see the head of the file
            bool grew;
            do {
                Row g = dilate<CLIPPED, ROT>(L, f, wide, L.wsh);
                if (p.reach == 2) g = dilate<CLIPPED, ROT>(L, g, wide, L.wsh);  // scalar
                g = {g.lo & rem.lo, g.hi & rem.hi};
                grew = __builtin_amdgcn_ballot_w64(g.lo != f.lo || g.hi != f.hi) != 0ull;
                f = g;
            } while (grew);

            // summary.  Rows: the board's lanes that hold a part of the object
            const u64 rows = (__builtin_amdgcn_ballot_w64((f.lo | f.hi) != 0u) & bm) >> board_sh;
            // columns: the OR over the board's lanes
            Row cm = f;
            for (int d = 1; d < H; d <<= 1) {  // scalar
                const int t = L.y + d;         // d < H: one wrap at most
                const int src = 4 * (L.active ? lane + (t >= H ? d - H : d) : lane);
                const uint32_t lo = lane_read(src, cm.lo), hi = lane_read(src, cm.hi);
                cm = {cm.lo | lo, cm.hi | hi};
            }
            const u64 cols = (u64)cm.lo | ((u64)cm.hi << 32);
            int x, w, y, h;
            span_of<CLIPPED>(cols, p.width, p.reach, x, w);
            span_of<CLIPPED>(rows, H, p.reach, y, h);
            // the object's row moved to the corner: columns by x (cyclically on a torus), the row key taken at
            // (the lane's row - y) mod height, so no row has to move; lanes without a part of it add 0
            const u64 fr = (u64)f.lo | ((u64)f.hi << 32);
            u64 tr = fr >> x;
            if constexpr (!CLIPPED) {
                const u64 wm = p.width >= 64 ? ~0ull : (1ull << p.width) - 1ull;
                tr = (tr | ((fr << 1) << (p.width - 1 - x))) & wm;
            }
            int ty = L.y - y;
            if (ty < 0) ty += H;
            const uint32_t u0 = unzip_bits((uint32_t)tr), u1 = unzip_bits((uint32_t)(tr >> 32));
            const uint32_t ev = (u0 & 0xFFFFu) | (u1 << 16), od = (u0 >> 16) | (u1 & 0xFFFF0000u);
            const uint32_t ae = gol::hash_row_key(ty);
            const u64 term = (u64)ev * ae + (u64)od * (uint32_t)(ae + gol::kHashOddAdd);
            // the board's sums, BoardSum::total's steps written out four abreast: the subtractions stay under the
            // writer's branch below (through S.total they left it, and the kernel was scheduled differently).  The
            // 64-bit terms go as limbs of 16, 16 and 32 bits: 64 lanes' limbs of 16 bits sum to less than 2^22, and
            // the upper limb is wanted modulo 2^32
            const uint32_t s_pop = wave_prefix_sum((uint32_t)__builtin_popcountll(fr));
            const uint32_t s_a = wave_prefix_sum((uint32_t)term & 0xFFFFu);
            const uint32_t s_b = wave_prefix_sum(((uint32_t)term >> 16) & 0xFFFFu);
            const uint32_t s_c = wave_prefix_sum((uint32_t)(term >> 32));
            const uint32_t b_pop = lane_read(before_addr, s_pop), b_a = lane_read(before_addr, s_a);
            const uint32_t b_b = lane_read(before_addr, s_b), b_c = lane_read(before_addr, s_c);
            if (writer && seeded && n < (uint32_t)p.max_objects) {
                const uint32_t pop = s_pop - (has_before ? b_pop : 0u);
                const u64 sum = (u64)(s_a - (has_before ? b_a : 0u)) + ((u64)(s_b - (has_before ? b_b : 0u)) << 16) +
                                ((u64)(s_c - (has_before ? b_c : 0u)) << 32);
                const u64 hash = sum * (u64)gol::hash_pair_key(0u);
                uint4 rec;  // gol_batch_object: hash, x y w h, population and the reserved 0
                rec.x = (uint32_t)hash;
                rec.y = (uint32_t)(hash >> 32);
                rec.z = (uint32_t)x | ((uint32_t)y << 8) | ((uint32_t)w << 16) | ((uint32_t)h << 24);
                rec.w = pop;  // <= 4096
                p.objects[out * (size_t)p.max_objects + n] = rec;
            }
            n += seeded ? 1u : 0u;
            rem = {rem.lo & ~f.lo, rem.hi & ~f.hi};
        }
    };
    // wave-uniform, outside the loops
    if (!CLIPPED && H == kLanes) run(std::true_type{});
    else run(std::false_type{});

    if (writer) p.counts[out] = n;
}

}  // namespace

hipError_t launch_batch_objects(const ObjectsParams& p, bool clipped, hipStream_t stream) {
    // every index the kernel forms stays inside the plane (p.boards, the range's end, is inside the batch: the
    // caller's to get right), the counts and the records
    if (!launch_geometry_ok(p.boards, p.width, p.height, p.boards_per_wave, clipped, p.vis_w, p.vis_h) || !p.plane ||
        !p.counts || !p.objects || p.first < 0 || p.boards <= p.first || (p.reach != 1 && p.reach != 2) ||
        p.max_objects < 1 || p.max_objects > kMaxBoardObjects || (!clipped && (p.width < 3 || p.height < 3)))
        return hipErrorInvalidValue;
    // the waves of the range's boards, not of the batch's
    const dim3 grid = launch_grid(p.height, (int64_t)p.boards - p.first), block(kLanes * kWavesPerWG);
    return clipped ? gol::launch_kernel(batch_objects_kernel<true>, grid, block, stream, p)
                   : gol::launch_kernel(batch_objects_kernel<false>, grid, block, stream, p);
}

}  // namespace golbatch
