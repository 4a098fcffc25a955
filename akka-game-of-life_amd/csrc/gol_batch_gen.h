// gol_batch_gen.h -- what the batch engine's kernels share on the device
// (gol_batch.hip: batch_step_kernel and batch_cycle_kernel; DESIGN.md sections
// 5f and 5g): one generation of a lane's row, from the rows above and below
// through to the masked new row, written once and instantiated from both
// kernels.  Everything is force-inlined and the per-lane constants are passed
// as references to the kernel's own locals, as the loop's lambda captured them
// when the generation was written out in it: batch_step_kernel's 16 instances
// keep their instruction streams (make asm-batch).  Device code only; not
// installed.  What is not the stencil -- the wave's prefix sum, the lane read,
// the per-board sum -- is gol_batch_wave.h's, which comes along from here.
#pragma once
#include "gol_batch.h"
#include "gol_batch_wave.h"
#include "gol_stencil.h"

namespace golbatch {

using namespace gol::dev;

struct Row {
    uint32_t lo, hi;
};
__device__ __forceinline__ Row row_of(uint32_t lo, uint32_t hi) { return Row{lo, hi}; }

// The per-lane constants of a generation: references to the kernel's locals.
struct GenConsts {
    const uint32_t &wm_lo, &wm_hi;  // the stored columns
    const uint32_t& wsh;  // torus: bit width - 1 inside its dword (the lower one iff width <= 32: the NARROW loops)
    // clipped: the lane's row as its neighbours see it, and whether it has a row above / below in its board
    const uint32_t &sm_lo, &sm_hi, &upm, &dnm;
    // torus, height < 64: the lanes holding the rows above and below, inside the lane's own board
    const int &up_addr, &dn_addr;
};

// A lane's place in its wave's boards and the values GenConsts refers to.
// batch_step_kernel keeps this arithmetic in its own body: taken from here its
// prologue was scheduled differently (two more SGPRs on the plain B3/S23
// torus instance), and its code is to stay what it was.
struct Lane {
    int H, bl, y;  // the board's height, the lane's board in the wave, its row
    int32_t board;
    bool active;   // the lane holds a row of a board of the batch
    size_t idx;    // active lanes: the row's word, < boards * height
    uint32_t wm_lo, wm_hi, wsh, sm_lo, sm_hi, upm, dnm;
    int up_addr, dn_addr;
    __device__ __forceinline__ GenConsts consts() const {
        return GenConsts{wm_lo, wm_hi, wsh, sm_lo, sm_hi, upm, dnm, up_addr, dn_addr};
    }
    // the board's lanes in a ballot (every lane for an idle one, which never votes)
    __device__ __forceinline__ unsigned long long board_lanes() const {
        const unsigned long long hm = H >= 64 ? ~0ull : (1ull << H) - 1ull;
        return active ? hm << (bl * H) : ~0ull;
    }
};

// P: a launch's parameters (boards, boards_per_wave, width, height, vis_w, vis_h)
template <bool CLIPPED, class P>
__device__ __forceinline__ Lane lane_of(const P& p, int lane, int32_t board0) {
    Lane c;
    c.H = p.height;
    const int H = c.H;
    c.bl = lane / H;
    c.y = lane - c.bl * H;
    const int bl = c.bl, y = c.y;
    c.board = board0 + bl;
    c.active = bl < p.boards_per_wave && c.board < p.boards;
    const bool active = c.active;
    c.idx = (size_t)c.board * (size_t)H + (size_t)y;
    const unsigned long long wmask = p.width >= 64 ? ~0ull : (1ull << p.width) - 1ull;
    c.wm_lo = (uint32_t)wmask;
    c.wm_hi = (uint32_t)(wmask >> 32);
    c.wsh = (uint32_t)(p.width - 1) & 31u;
    c.sm_lo = c.sm_hi = c.upm = c.dnm = 0xFFFFFFFFu;
    if constexpr (CLIPPED) {
        const unsigned long long vmask = p.vis_w >= 64 ? ~0ull : (1ull << p.vis_w) - 1ull;
        const bool seen = active && y < p.vis_h;
        c.sm_lo = seen ? (uint32_t)vmask : 0u;
        c.sm_hi = seen ? (uint32_t)(vmask >> 32) : 0u;
        c.upm = y > 0 ? 0xFFFFFFFFu : 0u;
        c.dnm = y < H - 1 ? 0xFFFFFFFFu : 0u;
    }
    c.up_addr = 4 * (active ? (y > 0 ? lane - 1 : lane + H - 1) : lane);
    c.dn_addr = 4 * (active ? (y < H - 1 ? lane + 1 : lane - (H - 1)) : lane);
    return c;
}

// One generation of the lane's row `cur`.  Every lane of the wave must be
// here: the rows above and below come through DPP or a permute.
// ROT: the wave is one torus board of 64 rows.  NARROW: width <= 32 -- a row's
// upper dword is zero and stays zero, so nothing is computed for it (the
// reference's 8 x 8 board: half the instructions).  P: birth, survive.
template <bool LIFE, bool CLIPPED, bool ROT, bool NARROW, class P>
__device__ __forceinline__ Row generation(const P& p, const GenConsts& c, const Row& cur) {
    // rows above (a) and below (b); s: the centre as a neighbour sees it
    Row a = {0u, 0u}, b = {0u, 0u}, s = cur;
    if constexpr (CLIPPED) {
        s = {cur.lo & c.sm_lo, NARROW ? 0u : cur.hi & c.sm_hi};
        a.lo = dpp_shr1_zero(s.lo) & c.upm;
        b.lo = dpp_shl1_zero(s.lo) & c.dnm;
        if constexpr (!NARROW) {
            a.hi = dpp_shr1_zero(s.hi) & c.upm;
            b.hi = dpp_shl1_zero(s.hi) & c.dnm;
        }
    } else if constexpr (ROT) {
        a.lo = dpp_ror1(cur.lo);
        b.lo = dpp_rol1(cur.lo);
        if constexpr (!NARROW) {
            a.hi = dpp_ror1(cur.hi);
            b.hi = dpp_rol1(cur.hi);
        }
    } else {
        a.lo = lane_read(c.up_addr, cur.lo);
        b.lo = lane_read(c.dn_addr, cur.lo);
        if constexpr (!NARROW) {
            a.hi = lane_read(c.up_addr, cur.hi);
            b.hi = lane_read(c.dn_addr, cur.hi);
        }
    }
    // column sums (v1 v0) = a + s + b, and their copies from the columns west and east
    const Row v0 = row_of(GOL_BITOP3(a.lo, s.lo, b.lo, kXor3), NARROW ? 0u : GOL_BITOP3(a.hi, s.hi, b.hi, kXor3));
    const Row v1 = row_of(GOL_BITOP3(a.lo, s.lo, b.lo, kMaj), NARROW ? 0u : GOL_BITOP3(a.hi, s.hi, b.hi, kMaj));
    const uint32_t wsh = c.wsh;
    auto west = [&](const Row& v) -> Row {  // column x - 1 at bit x
        Row w = row_of(v.lo << 1, NARROW ? 0u : __builtin_amdgcn_alignbit(v.hi, v.lo, 31));
        if constexpr (!CLIPPED) w.lo |= ((NARROW ? v.lo : v.hi) >> wsh) & 1u;
        return w;
    };
    auto east = [&](const Row& v) -> Row {  // column x + 1 at bit x
        Row e = row_of(NARROW ? v.lo >> 1 : __builtin_amdgcn_alignbit(v.hi, v.lo, 1), v.hi >> 1);
        if constexpr (!CLIPPED) {
            const uint32_t t = (v.lo & 1u) << wsh;
            if constexpr (NARROW) e.lo |= t;
            else e.hi |= t;
        }
        return e;
    };
    const Row w0 = west(v0), w1 = west(v1), e0 = east(v0), e1 = east(v1);
    Row nx = {0u, 0u};
    if constexpr (LIFE && !CLIPPED) {
        nx.lo = rule_b3s23_fullsum(w0.lo, w1.lo, v0.lo, v1.lo, e0.lo, e1.lo, cur.lo);
        if constexpr (!NARROW) nx.hi = rule_b3s23_fullsum(w0.hi, w1.hi, v0.hi, v1.hi, e0.hi, e1.hi, cur.hi);
    } else {
        auto half = [&](uint32_t aw, uint32_t bw, uint32_t ww0, uint32_t ww1, uint32_t ee0, uint32_t ee1,
                        uint32_t al) -> uint32_t {
            const uint32_t p0 = aw ^ bw, p1 = aw & bw;  // the column minus its centre
            const uint32_t nb0 = GOL_BITOP3(ww0, ee0, p0, kXor3);
            const uint32_t c0 = GOL_BITOP3(ww0, ee0, p0, kMaj);
            const uint32_t pp = GOL_BITOP3(ww1, ee1, p1, kXor3);
            const uint32_t qq = GOL_BITOP3(ww1, ee1, p1, kMaj);
            uint32_t o;
            GOL_RULE_FROM_COUNT(o, LIFE, p, nb0, c0, pp, qq, al);
            return o;
        };
        nx.lo = half(a.lo, b.lo, w0.lo, w1.lo, e0.lo, e1.lo, cur.lo);
        if constexpr (!NARROW) nx.hi = half(a.hi, b.hi, w0.hi, w1.hi, e0.hi, e1.hi, cur.hi);
    }
    nx.lo &= c.wm_lo;
    if constexpr (!NARROW) nx.hi &= c.wm_hi;
    return nx;
}

}  // namespace golbatch
