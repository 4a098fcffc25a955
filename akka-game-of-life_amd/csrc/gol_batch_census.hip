// gol_batch_census.hip -- the census of a batch's objects (gol_census_batch_*
// in gol_batch.cpp): a hash table in device memory that
// counts the objects of every key (hash, w, h, population) over as many calls
// as the caller likes and keeps each key's earliest place.  A unit of its own,
// without the stencil: of the batch's device headers it takes gol_batch_wave.h
// (the wave's prefix sum) alone.
//
// The table.  capacity slots (a power of two) of four qwords:
//   A      hash[47:0] << 1 | 1
//   B      hash[63:48] | w << 16 | h << 24 | population << 32 | 1 << 63
//   count  the objects with this key
//   place  the minimum of call << 38 | board << 16 | y << 8 | x over them
// A and B are never zero, and zero means "not yet set".  A word goes from zero
// to its value once, by a compare-and-swap, and never changes again.
//
// Insert (census_insert): from the key's home slot, at most
// min(capacity, kCensusProbeWindow) slots in turn.  At a slot: A is compared
// and swapped from zero; if it was neither zero nor the key's A, the slot is
// another key's -- on to the next.  Then the same for B.  With both words the
// key's, count is added to and place lowered, each with one atomic.  Nothing
// waits: a thread that loses a compare-and-swap has learnt the slot's word,
// which is final, and either matches it or moves on.  A slot that holds the
// key's A and another key's B (the two share hash[47:0] and met at this slot)
// is that other key's; the key's A under a B still zero will get its B from
// whoever set the A, in the next instruction it executes, and from anyone else
// who comes by with that A first.  So every thread with one key passes the
// same slots and stops at the same one, and a key occupies one slot at most.
// The words are read with an atomic load first and swapped only where zero:
// an established key costs one 16-byte read, an add, and a read of place.
//
// census_tally_kernel: one thread per record slot.  Before touching the table
// the wave aggregates: while a ballot of the lanes with a record left is not
// empty, the first of them is the leader; its key is read into scalars, every
// lane compares, a ballot gives the group; the group's lowest place is a wave
// reduction (a 32-bit minimum over DPP: within a wave the call is one and the
// boards are 64 apart at most, so board - the wave's first board, y and x fit
// one dword); the leader inserts the key once with the group's size.  At most
// 64 rounds; the loop's conditions are scalars and ballots, and no cross-lane
// operation sits under a lane branch.  The wave's sums go to the counters
// with one atomic each per wave.
//
// census_compact_kernel: one thread per slot; ballot and prefix inside the
// wave, one atomic add per wave for the output offset, plain 16-byte stores.
//
// No LDS, no scratch; vector atomics at device scope only.
#include "gol_batch.h"
#include "gol_batch_wave.h"
#include "gol_kernels.h"

namespace golbatch {

namespace {

using u64 = unsigned long long;

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_min(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xf, false);
    return o < v ? o : v;
}

// The sum / the minimum over the wave's 64 lanes, as a scalar.  Every lane of
// the wave must be here.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum(v), kLanes - 1);
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = dpp_min<kDppRowShr + 1, 0xf>(v);
    v = dpp_min<kDppRowShr + 2, 0xf>(v);
    v = dpp_min<kDppRowShr + 4, 0xf>(v);
    v = dpp_min<kDppRowShr + 8, 0xf>(v);
    v = dpp_min<kDppRowBcast15, 0xa>(v);
    v = dpp_min<kDppRowBcast31, 0xc>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, kLanes - 1);
}

__device__ __forceinline__ u64 load_word(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A key's home slot (before the mask): both words mixed, so that keys that
// differ in one word only, or in a few bits, do not share their window.
__device__ __forceinline__ uint32_t census_home(u64 a, u64 b) {
    u64 x = a ^ (b * 0x9E3779B97F4A7C15ull);
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 29;
    return (uint32_t)x;
}

// `n` objects of key (a, b), the earliest of them at `place`.  False: the key
// is not within its window and no slot there is free -- nothing was written.
__device__ __forceinline__ bool census_insert(const CensusTable& t, u64 a, u64 b, u64 n, u64 place) {
    const uint32_t mask = t.capacity - 1u;
    const uint32_t window = t.capacity < kCensusProbeWindow ? t.capacity : kCensusProbeWindow;
    uint32_t s = census_home(a, b) & mask;
    for (uint32_t k = 0; k < window; ++k, s = (s + 1u) & mask) {
        u64* slot = t.slots + 4 * (size_t)s;
        u64 sa = load_word(slot), sb = load_word(slot + 1);
        if (sa == 0ull) {
            sa = atomicCAS(slot, 0ull, a);
            if (sa == 0ull) sa = a;
        }
        if (sa != a) continue;
        if (sb == 0ull) {
            sb = atomicCAS(slot + 1, 0ull, b);
            if (sb == 0ull) {  // this thread completed the slot: one more distinct key
                atomicAdd(t.counters + kCensusDistinct, 1ull);
                sb = b;
            }
        }
        if (sb != b) continue;
        atomicAdd(slot + 2, n);
        if (load_word(slot + 3) > place) atomicMin(slot + 3, place);  // place only falls: a stale read is too high
        return true;
    }
    return false;
}

__global__ __launch_bounds__(kLanes* kWavesPerWG) void census_clear_kernel(const CensusTable t) {
    const uint32_t i = blockIdx.x * (uint32_t)(kLanes * kWavesPerWG) + threadIdx.x;  // capacity <= 2^21
    if (i < (uint32_t)kCensusCounters) t.counters[i] = 0ull;
    if (i >= t.capacity) return;
    uint4* slot = reinterpret_cast<uint4*>(t.slots + 4 * (size_t)i);
    slot[0] = make_uint4(0u, 0u, 0u, 0u);
    slot[1] = make_uint4(0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu);
}

__global__ __launch_bounds__(kLanes* kWavesPerWG) void census_tally_kernel(const CensusTallyParams p) {
    // total <= 2^32 and the grid is ceil(total / 256) blocks: no index wraps
    const uint32_t i = blockIdx.x * (uint32_t)(kLanes * kWavesPerWG) + threadIdx.x;
    const int lane = threadIdx.x & (kLanes - 1);
    const bool in = (u64)i < p.total;
    uint32_t board = p.board, j = 1u, count = 0xFFFFFFFFu;
    if (p.counts) {  // scalar
        board = i / p.max_objects;
        j = i - board * p.max_objects;
        count = in ? p.counts[board] : 0u;
    }
    const bool have = in && j < count;
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);  // gol_batch_object: hash, x y w h, population and the reserved word
    if (have) rec = p.records[i];
    const uint32_t pop = rec.w & 0xFFFFu;
    const bool live = have && pop != 0u;
    const u64 a = ((((u64)(rec.y & 0xFFFFu) << 32) | (u64)rec.x) << 1) | 1ull;
    const u64 b = (u64)(rec.y >> 16) | ((u64)(rec.z >> 16) << 16) | ((u64)pop << 32) | (1ull << 63);
    // a live lane's board is the wave's first board or one of the 63 after it
    const uint32_t board0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)board);
    const uint32_t rel = ((board - board0) << 16) | (rec.z & 0xFFFFu);  // board, y, x
    const u64 base = ((u64)p.call << 38) | ((u64)board0 << 16);

    // the board's first slot speaks for the board
    const bool first = p.counts && in && j == 0u;
    const uint32_t seen = wave_sum(p.counts ? (first ? count : 0u) : (live ? 1u : 0u));
    const uint32_t truncated = wave_sum(first && count > p.max_objects ? count - p.max_objects : 0u);
    uint32_t tallied = 0u, overflowed = 0u;  // scalars

#ifndef GOL_CENSUS_NO_AGGREGATE
    u64 pending = __builtin_amdgcn_ballot_w64(live);
    while (pending != 0ull) {
        const int leader = __builtin_ctzll(pending);
        const u64 ka = (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)a, leader) |
                       ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(a >> 32), leader) << 32);
        const u64 kb = (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, leader) |
                       ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), leader) << 32);
        const bool same = live && a == ka && b == kb;
        const u64 group = __builtin_amdgcn_ballot_w64(same);  // the leader and lanes still pending: a lane done has another key
        const uint32_t lowest = wave_min(same ? rel : 0xFFFFFFFFu);
        const uint32_t n = (uint32_t)__builtin_popcountll(group);
        bool ok = false;
        if (lane == leader) ok = census_insert(p.table, ka, kb, n, base + lowest);
        const bool kept = __builtin_amdgcn_ballot_w64(ok) != 0ull;
        tallied += kept ? n : 0u;
        overflowed += kept ? 0u : n;
        pending &= ~group;
    }
#else
    // the measurement's other side (scripts/batch_census_bench.py): every lane inserts its own record
    bool ok = false;
    if (live) ok = census_insert(p.table, a, b, 1ull, base + rel);
    tallied = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
    overflowed = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live && !ok));
#endif

    if (lane == 0) {
        if (seen) atomicAdd(p.table.counters + kCensusSeen, (u64)seen);
        if (tallied) atomicAdd(p.table.counters + kCensusTallied, (u64)tallied);
        if (truncated) atomicAdd(p.table.counters + kCensusTruncated, (u64)truncated);
        if (overflowed) atomicAdd(p.table.counters + kCensusOverflowed, (u64)overflowed);
    }
}

__global__ __launch_bounds__(kLanes* kWavesPerWG) void census_compact_kernel(const CensusTable t, uint4* out,
                                                                             const u64 out_capacity) {
    const uint32_t i = blockIdx.x * (uint32_t)(kLanes * kWavesPerWG) + threadIdx.x;  // capacity <= 2^21
    const int lane = threadIdx.x & (kLanes - 1);
    uint4 k = make_uint4(0u, 0u, 0u, 0u), v = k;  // A B, count place
    if (i < t.capacity) {
        const uint4* slot = reinterpret_cast<const uint4*>(t.slots + 4 * (size_t)i);
        k = slot[0];
        v = slot[1];
    }
    const bool occupied = (k.x | k.y) != 0u && (k.z | k.w) != 0u;
    const u64 votes = __builtin_amdgcn_ballot_w64(occupied);
    if (votes == 0ull) return;  // wave-uniform
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(votes >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)votes, 0u));
    u64 offset = 0ull;
    if (lane == 0) offset = atomicAdd(t.counters + kCensusCompacted, (u64)__builtin_popcountll(votes));
    offset = (u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)offset) |
             ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(offset >> 32)) << 32);
    const u64 at = offset + rank;
    if (!occupied || at >= out_capacity) return;
    const u64 a = (u64)k.x | ((u64)k.y << 32), b = (u64)k.z | ((u64)k.w << 32);
    const u64 hash = ((a >> 1) & 0xFFFFFFFFFFFFull) | (b << 48);
    const u64 place = (u64)v.z | ((u64)v.w << 32);
    // gol_census_entry: hash; w h population, first_call; count; first_board, first_x first_y and the reserved 0
    out[2 * at] = make_uint4((uint32_t)hash, (uint32_t)(hash >> 32), (uint32_t)((b >> 16) & 0xFFFFFFFFull),
                             (uint32_t)(place >> 38) & 0xFFFFFFu);
    out[2 * at + 1] = make_uint4(v.x, v.y, (uint32_t)(place >> 16) & 0x3FFFFFu, (uint32_t)place & 0xFFFFu);
}

bool table_ok(const CensusTable& t) {
    return t.slots && t.counters && t.capacity >= 2u && t.capacity <= 2u * (uint32_t)kMaxCensusKeys &&
           (t.capacity & (t.capacity - 1u)) == 0u;
}

dim3 blocks_for(uint64_t threads) {
    return dim3((unsigned)((threads + kLanes * kWavesPerWG - 1) / (kLanes * kWavesPerWG)));
}

}  // namespace

hipError_t launch_census_clear(const CensusTable& t, hipStream_t stream) {
    if (!table_ok(t)) return hipErrorInvalidValue;
    return gol::launch_kernel(census_clear_kernel, blocks_for(t.capacity), dim3(kLanes * kWavesPerWG), stream, t);
}

hipError_t launch_census_tally(const CensusTallyParams& p, hipStream_t stream) {
    // every index the kernel forms stays inside the records ([total]), the counts ([total / max_objects]: the
    // caller's to get right) and the table
    if (!table_ok(p.table) || !p.records || p.total < 1 || p.total > (1ull << 32) || p.board >= (uint32_t)kMaxBoards ||
        p.call >= kMaxCensusCalls)
        return hipErrorInvalidValue;
    if (p.counts && (p.max_objects < 1 || p.max_objects > (uint32_t)kMaxBoardObjects || p.total % p.max_objects != 0 ||
                     p.total / p.max_objects > (uint64_t)kMaxBoards))
        return hipErrorInvalidValue;
    if (!p.counts && p.total > kMaxCensusRecords) return hipErrorInvalidValue;
    return gol::launch_kernel(census_tally_kernel, blocks_for(p.total), dim3(kLanes * kWavesPerWG), stream, p);
}

hipError_t launch_census_compact(const CensusTable& t, uint4* out, uint64_t out_capacity, hipStream_t stream) {
    if (!table_ok(t) || !out || out_capacity < 1) return hipErrorInvalidValue;
    return gol::launch_kernel(census_compact_kernel, blocks_for(t.capacity), dim3(kLanes * kWavesPerWG), stream, t, out,
                              out_capacity);
}

}  // namespace golbatch
