// gol_batch.h -- internal interface between the batch engine's C-ABI unit
// (gol_batch.cpp) and its gfx950 kernels (gol_batch*.hip); DESIGN.md sections
// 5f to 5l: the lane mapping, the pure validators, the launch parameters and
// what every launcher checks of them.  A header of its own: the step kernels'
// units include none of it.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gol.h"
#include "gol_soup.h"

namespace golbatch {

constexpr int kLanes = 64;              // CDNA wavefront: one 64-bit row per lane
constexpr int kWavesPerWG = 4;          // 256-thread workgroups
constexpr int32_t kMaxBoards = 1 << 22;
constexpr uint32_t kAutoChunk = 1024;   // generations per launch (gol_batch_set_chunk 0): golc::kStepChunk

// The lane mapping, a function of the geometry alone: a wave holds
// k = 64 / height whole boards, lane l < k * height row l % height of the
// wave's board l / height (the other lanes are idle); the last wave may hold
// fewer boards.  What gol_batch_geometry_get reports and launch_batch_step
// launches.
struct Lanes {
    int32_t boards_per_wave;
    int64_t waves;
};
inline Lanes batch_lanes(int32_t height, int64_t boards) {
    const int32_t k = kLanes / height;
    return {k, (boards + k - 1) / k};
}

// What every per-board launcher checks of its parameters before its own: with
// it, the lane mapping's indices stay inside `boards` boards of `height` rows.
inline bool launch_geometry_ok(int32_t boards, int32_t width, int32_t height, int32_t boards_per_wave,
                               bool clipped = false, int32_t vis_w = 1, int32_t vis_h = 1) {
    return boards >= 1 && boards <= kMaxBoards && width >= 1 && width <= kLanes && height >= 1 && height <= kLanes &&
           boards_per_wave == batch_lanes(height, boards).boards_per_wave && (!clipped || (vis_w >= 1 && vis_h >= 1));
}
// ... and the grid it launches: workgroups of kWavesPerWG waves for `boards` boards.
inline dim3 launch_grid(int32_t height, int64_t boards) {
    return dim3((unsigned)((batch_lanes(height, boards).waves + kWavesPerWG - 1) / kWavesPerWG));
}

// The geometry a batch runs with, or the reason it is refused (null: fine).
struct Geometry {
    int32_t boards, width, height;
    int32_t vis_w, vis_h;  // clipped: visible extents; torus: the board
    bool clipped;
};
inline const char* batch_geometry(const gol_batch_config& c, Geometry* g) {
    if (c.topology != GOL_TORUS && c.topology != GOL_REF_CLIPPED) return "unknown topology";
    if (c.boards < 1 || c.boards > kMaxBoards) return "boards must be 1 .. 2^22";
    if (c.width < 1 || c.height < 1 || c.width > kLanes || c.height > kLanes)
        return "width and height must be 1 .. 64 stored cells";
    if ((c.birth_mask | c.survive_mask) & ~0x1FFu) return "rule masks must fit in 9 bits";
    const bool clipped = c.topology == GOL_REF_CLIPPED;
    int32_t vw = c.width, vh = c.height;
    if (clipped) {
        // gol_create's refusal: the reference never completes a generation
        // on a board where some cell has no visible neighbour
        vw = c.vis_width > 0 ? c.vis_width : c.width - 1;
        vh = c.vis_height > 0 ? c.vis_height : c.height - 1;
        // (extents beyond the stored board show no more than the board: a single visible cell stays one)
        if (vw < 1 || vh < 1 || (std::min(vw, c.width) == 1 && std::min(vh, c.height) == 1) || c.width > vw + 1 ||
            c.height > vh + 1)
            return "ref-clipped board on which a cell has no visible neighbour: the reference never completes a "
                   "generation on such a board (NextStateCellGathererActor.scala:26-27,39-58, "
                   "CellActor.scala:75-76,92-94)";
    } else if (c.width < 3 || c.height < 3) {
        return "torus width and height must be 3 .. 64";
    }
    *g = {c.boards, c.width, c.height, vw, vh, clipped};
    return nullptr;
}

// boards [first, first + count) inside the batch
inline bool window_ok(const Geometry& g, int64_t first, int64_t count) {
    return first >= 0 && count >= 1 && first < g.boards && count <= (int64_t)g.boards - first;
}

// Device memory of a batch: the plane, the plane of the generation before it
// (settle detection across launches) and one settle word per board.
inline uint64_t batch_device_bytes(const Geometry& g) {
    const uint64_t plane = (uint64_t)g.boards * (uint64_t)g.height * sizeof(uint64_t);
    return 2 * plane + (uint64_t)g.boards * sizeof(uint32_t);
}

// Pattern search on a batch (gol_find_batch).
constexpr int32_t kMaxFindPatterns = 256;
// Cared cells per launch (gol_find_batch_set_cut 0): the pattern list is cut
// into launches of at most this many, a pattern that has more alone in its
// own.  Section 5h derives it from the measured cost per cared cell.
constexpr uint32_t kAutoFindCut = 2048;

// The patterns a batch of geometry g can be searched for, or the reason they
// are refused (null: fine) and, in *which, the pattern it is about (-1: the
// list).  What gol_find_batch_check reports and gol_find_batch does first.
inline const char* batch_find_patterns(const Geometry& g, const gol_batch_pattern* patterns, int32_t npatterns,
                                       int32_t* which) {
    *which = -1;
    if (!patterns) return "patterns is null";
    if (npatterns < 1 || npatterns > kMaxFindPatterns) return "npatterns must be 1 .. 256";
    for (int32_t p = 0; p < npatterns; ++p) {
        const gol_batch_pattern& q = patterns[p];
        *which = p;
        if (q.pw < 1 || q.ph < 1 || q.pw > g.width || q.ph > g.height)
            return "pw and ph must be 1 .. the boards' width and height";
        if (!q.cells) return "cells is null";
        if (q.care) {
            const uint64_t kmask = q.pw >= 64 ? ~0ull : (1ull << q.pw) - 1ull;
            uint64_t any = 0;
            for (int32_t i = 0; i < q.ph; ++i) any |= q.care[i] & kmask;
            if (!any) return "the pattern cares for no cell";
        }
    }
    *which = -1;
    return nullptr;
}

// The device's pattern table: per pattern its extents and the first of its ph
// rows in the row array, a row being the qword pair (cells & care, care) with
// the bits at k >= pw cleared.
struct FindPattern {
    int32_t pw, ph;
    uint32_t row0, cared;  // cared: the pattern's cared cells (the launch cut counts them)
};

// One launch: patterns first .. first + count - 1 of the table against every board.
struct FindParams {
    const unsigned long long* plane;  // boards * height rows; read only
    uint32_t* counts;                 // [boards][npatterns]
    unsigned long long* matches;      // null, or [npatterns][boards][height]
    int32_t boards, width, height, boards_per_wave;
    int32_t npatterns, first, count;
};

// Per-board rules (gol_rules_batch_*): one word per
// board, the birth mask in bits 0..8 and the survive mask in bits 16..24
// (GOL_BATCH_RULE); no other bit may be set.
constexpr uint32_t kRuleWordBits = 0x01FF01FFu;
inline uint32_t rule_word(uint32_t birth, uint32_t survive) { return GOL_BATCH_RULE(birth, survive); }

// The rules boards first .. first + count - 1 of a batch of geometry g can be
// given, or the reason they are refused (null: fine) and, in *which, the index
// into `rules` of the word it is about (-1: the range).  rules == null (back
// to the configuration's rule) is for the whole batch only.  What
// gol_rules_batch_check reports and gol_rules_batch_set does first.
inline const char* batch_rules_args(const Geometry& g, int64_t first, int64_t count, const uint32_t* rules,
                                    int64_t* which) {
    *which = -1;
    if (!window_ok(g, first, count)) return "boards [first, first + count) outside the batch";
    if (!rules) return first == 0 && count == g.boards ? nullptr : "rules is null for a part of the batch";
    for (int64_t j = 0; j < count; ++j)
        if (rules[j] & ~kRuleWordBits) {
            *which = j;
            return "a rule word has a bit set outside the birth mask (bits 0..8) and the survive mask (bits 16..24)";
        }
    return nullptr;
}

// One launch: `gens` generations of every board, in place.
struct StepParams {
    unsigned long long* plane;  // boards * height rows
    unsigned long long* prev;   // settle: the plane one generation before `plane`; read when g0 > 0, always written
    uint32_t* pops;             // populations: [boards][pop_stride], this launch's generations from column 0
    uint32_t* settled;          // settle: [boards], 0 = not yet; read when g0 > 0, always written
    int32_t boards, width, height, boards_per_wave;
    int32_t vis_w, vis_h;
    uint32_t gens;              // generations of this launch
    uint32_t g0;                // generations of the call before this launch
    uint32_t pop_stride;
    uint32_t birth, survive;
    const uint32_t* rules;      // per-board rules (the RULES instances): [boards] rule words; null: birth / survive
};

// Cycle detection's schedule (gol_cycle_step): Brent's
// algorithm with snapshots at the generations t_k = 2^k - 1 of a call, a board
// after g generations compared with the snapshot t_k < g <= t_{k+1}.  The one
// place it is written: gol_cycle_snapshot_generation returns it, and the kernel
// replaces the snapshot where cycle_is_snapshot says so and takes a board's
// period from the generation its cycle was seen at.
// The t_k that generation g >= 1 is compared with; right for every uint32_t g.
__host__ __device__ inline uint32_t cycle_snapshot_generation(uint32_t g) {
    return (1u << (31 - __builtin_clz(g))) - 1u;
}
// g is a t_k, k >= 1: the board after generation g becomes the snapshot
// (2^32 - 1 is t_32: g + 1 wraps to 0).
__host__ __device__ inline bool cycle_is_snapshot(uint32_t g) { return (g & (g + 1u)) == 0u; }

// One launch of a cycle call: `gens` generations of every board, in place.
struct CycleParams {
    unsigned long long* plane;  // boards * height rows
    unsigned long long* snap;   // the snapshot plane (the batch's `prev`); read when g0 > 0
    uint32_t* period;           // [boards], 0 = no cycle seen yet; written with seen
    uint32_t* seen;             // [boards], 0 = not yet; read when g0 > 0
    uint32_t* counters;         // [0] boards that have a period, [1] the largest period
    int32_t boards, width, height, boards_per_wave;
    int32_t vis_w, vis_h;
    uint32_t gens;              // generations of this launch
    uint32_t g0;                // generations of the call before this launch
    uint32_t birth, survive;
    const uint32_t* rules;      // per-board rules (the RULES instances): [boards] rule words; null: birth / survive
};

// life: the B3/S23 instances; clipped: the topology; null pops / settled: the
// instance without that part; rules: the RULES instances, every board under
// its own word of p.rules (`life` means nothing then).  hipErrorInvalidValue
// for parameters outside what the kernels index safely, and for a p.rules
// that is null with `rules` or set without it.
hipError_t launch_batch_step(const StepParams& p, bool life, bool clipped, bool rules, hipStream_t stream);
hipError_t launch_batch_cycle(const CycleParams& p, bool life, bool clipped, bool rules, hipStream_t stream);
hipError_t launch_batch_seed(unsigned long long* plane, int64_t words, int32_t width, uint64_t seed,
                             hipStream_t stream);
// hashes[i] / pops[i] (either may be null) of boards first .. first + count - 1.
hipError_t launch_batch_hashes(const unsigned long long* plane, int32_t height, int64_t first, int64_t count,
                               unsigned long long* hashes, uint32_t* pops, hipStream_t stream);
// gol_batch_find.hip.  hipErrorInvalidValue for parameters outside what the
// kernel indexes safely; the table (`patterns`: [p.npatterns] headers, `rows`:
// the row array they index) is the caller's to get right.
hipError_t launch_batch_find(const FindParams& p, const FindPattern* patterns, const unsigned long long* rows,
                             bool clipped, hipStream_t stream);

// The objects of a batch's boards (gol_objects_batch).
// Two live cells of one 2 x 2 tile are always linked, so a board of at most
// 64 x 64 cells has at most 32 * 32 objects.
constexpr int32_t kMaxBoardObjects = 1024;

// The boards, reach and records per board that a batch of geometry g can be
// asked for, or the reason they are refused (null: fine).  What
// gol_objects_batch_check reports and gol_objects_batch does first.
inline const char* batch_objects_args(const Geometry& g, int64_t first, int64_t count, int32_t reach,
                                      int32_t max_objects) {
    if (reach != 1 && reach != 2) return "reach must be 1 or 2";
    if (max_objects < 1 || max_objects > kMaxBoardObjects) return "max_objects must be 1 .. 1024";
    if (!window_ok(g, first, count)) return "boards [first, first + count) outside the batch";
    return nullptr;
}

// One launch: the objects of boards first .. boards - 1.
struct ObjectsParams {
    const unsigned long long* plane;  // the batch's rows; read only
    uint32_t* counts;                 // [boards - first]
    uint4* objects;                   // [boards - first][max_objects] gol_batch_object records, zeroed by the caller
    int32_t boards;                   // the end of the range, <= the batch's boards
    int32_t width, height, boards_per_wave;
    int32_t vis_w, vis_h;
    int32_t first, reach, max_objects;
};

// gol_batch_objects.hip.  hipErrorInvalidValue for parameters outside what
// the kernel indexes safely.
hipError_t launch_batch_objects(const ObjectsParams& p, bool clipped, hipStream_t stream);

// The census of a batch's objects (gol_census_batch_*):
// a hash table of the handle's, filled on the device from the records the
// objects kernel leaves there and summed over as many calls as the caller
// likes.
constexpr int64_t kMaxCensusKeys = GOL_CENSUS_BATCH_MAX_KEYS;
// A key is stored only within this many linear probes of its home slot (or the
// whole table, if that is smaller): the longest any probe loop runs, and what
// makes "not found in the window" mean "absent".
constexpr uint32_t kCensusProbeWindow = 256;
constexpr uint64_t kMaxCensusRecords = 1ull << 22;  // gol_census_batch_add_records' n
constexpr uint64_t kMaxCensusCalls = 1ull << 24;    // ordinals 0 .. 2^24 - 1: 24 bits of the exemplar's place

// The table's slots for max_keys distinct keys: the power of two >= 2 * max_keys.
inline uint32_t census_capacity(int64_t max_keys) {
    uint32_t c = 2;
    while ((int64_t)c < 2 * max_keys) c <<= 1;
    return c;
}

// One census call as its validator sees it: the call, what the handle holds
// (ignored by kCheck and kBegin) and the call's own arguments (those of the
// other calls ignored).
struct CensusRequest {
    enum Call { kCheck, kBegin, kAdd, kAddRecords, kRead } call;
    bool begun;                  // the handle has a table
    uint64_t next_call;          // the ordinal kAdd / kAddRecords would take
    int32_t reach, max_objects;  // kCheck, kAdd
    int64_t max_keys;            // kCheck, kBegin
    bool records_null;           // kAddRecords
    uint64_t n;
    uint32_t board;
};

// Whether a census call is fine (null) or the reason it is refused.  What
// gol_census_batch_check reports and every gol_census_batch_* call does first.
inline const char* batch_census_args(const Geometry& g, const CensusRequest& r) {
    using R = CensusRequest;
    if (r.call == R::kCheck || r.call == R::kAdd)
        if (const char* why = batch_objects_args(g, 0, g.boards, r.reach, r.max_objects)) return why;
    if ((r.call == R::kCheck || r.call == R::kBegin) && (r.max_keys < 1 || r.max_keys > kMaxCensusKeys))
        return "max_keys must be 1 .. 2^20";
    if ((r.call == R::kAdd || r.call == R::kAddRecords || r.call == R::kRead) && !r.begun)
        return "no census has begun (gol_census_batch_begin)";
    if (r.call == R::kAddRecords) {
        if (r.n > kMaxCensusRecords) return "n must be at most 2^22";
        if (r.n > 0 && r.records_null) return "records is null";
        if (r.board >= (uint32_t)kMaxBoards) return "board must be below 2^22";
    }
    if ((r.call == R::kAdd || r.call == R::kAddRecords) && r.next_call >= kMaxCensusCalls)
        return "the census has had 2^24 calls: ordinals stop at 2^24 - 1 (begin again)";
    return nullptr;
}

// The table on the device.  A slot is four qwords: the key's two tagged words
// A and B (zero: not yet set), the count, and the exemplar's place (all-ones:
// none yet).  counters: kCensusCounters qwords.
enum CensusCounter {
    kCensusSeen, kCensusTallied, kCensusTruncated, kCensusOverflowed, kCensusDistinct,
    kCensusCompacted,  // the compaction's output offset
    kCensusCounters
};
struct CensusTable {
    unsigned long long* slots;     // [capacity][4]
    unsigned long long* counters;  // [kCensusCounters]
    uint32_t capacity;             // a power of two, 2 .. 2^21
};

// One tally launch: record slot i < total of `records`.  counts != null (the
// batch's objects): slot i is record i % max_objects of board i / max_objects,
// real iff that is below counts[board] and its population is not 0.  counts ==
// null (the caller's records): every slot is board `board`'s, real iff its
// population is not 0.
struct CensusTallyParams {
    const uint4* records;
    const uint32_t* counts;
    CensusTable table;
    uint64_t total;  // <= 2^32: a slot's index fits 32 bits
    uint32_t max_objects, board, call;
};

// gol_batch_census.hip.  hipErrorInvalidValue for parameters outside what the
// kernels index safely.  clear: an empty table and zero counters.  compact:
// the occupied slots as gol_census_entry records to `out` (room for
// out_capacity of them, at least the distinct keys; in any order), their
// number added to counters[kCensusCompacted] (zeroed by the caller).
hipError_t launch_census_clear(const CensusTable& t, hipStream_t stream);
hipError_t launch_census_tally(const CensusTallyParams& p, hipStream_t stream);
hipError_t launch_census_compact(const CensusTable& t, uint4* out, uint64_t out_capacity, hipStream_t stream);

// Soups (gol_soup_batch*).  The validator, the raw bits
// and the groups are gol_soup.h's, which needs no HIP.
inline const char* batch_soup_args(const Geometry& g, const gol_soup_spec* s, int64_t first, int64_t count) {
    return golsoup::soup_args(g.width, g.height, g.boards, s, first, count);
}

// One launch: boards first .. first + count - 1 become the soups of `spec`.
struct SoupParams {
    unsigned long long* plane;         // boards * height rows
    const unsigned long long* domain;  // [golsoup::kMaxSide]: the fundamental domain's row masks (golsoup::make_plan)
    gol_soup_spec spec;
    int32_t boards, width, height, boards_per_wave;
    int32_t first, count;
    uint32_t steps;  // golsoup::steps(spec.symmetry): the launcher's to fill in
};

// gol_batch_soup.hip.  hipErrorInvalidValue for parameters outside what the
// kernel indexes safely: everything batch_soup_args refuses among them.
hipError_t launch_batch_soup(const SoupParams& p, hipStream_t stream);

}  // namespace golbatch
