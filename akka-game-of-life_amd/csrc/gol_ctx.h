// gol_ctx.h -- libgol's host-side internals shared by the C-ABI units.  Not
// installed; the boundary is include/gol.h.
//
//   gol_capi.cpp       error state, context lifetime, seeding, stepping, hashes,
//                      tuning and the remaining small entry points
//   gol_plan.h         the schedule rules as pure functions of integers (no HIP,
//                      no context): band plan of a launch (band height,
//                      small-board cut, tail split, grid), XCD chunk, depth
//                      planner -- checked on the CPU (tests/schedule_probe.cpp)
//   gol_active.h       active-row stepping as pure functions (no HIP, no
//                      context): row runs that can hold a live cell, their
//                      growth per pass, what to clear, when to scan -- checked
//                      on the CPU (tests/active_probe.cpp)
//   gol_schedule.cpp   kernel instance and strip count of a pass, its kernel
//                      launches (whole shard, interior and boundary rows) and
//                      pass plan: gathers gol_plan.h's inputs from the context
//   gol_ring.cpp       the ring schedule: one_pass, the RCCL halo exchange and
//                      the RCCL gol_comm_* entry points
//   gol_loopback.cpp   the in-process loopback ring that stands in for RCCL in
//                      tests (gol_comm_init_loopback)
//   gol_active.cpp     the pass of a context stepped whole: one launch, or with
//                      active-row stepping one per run of live rows
//                      (gol_set_active_rows, gol_active_*)
//   gol_group.cpp      in-process shard groups (gol_group_*)
//   gol_checkpoint.cpp snapshots, checkpoints, restore and light-cone replay
//   gol_profile.h      the accounting of pass timing as pure functions (no HIP, no
//                      context) -- checked on the CPU (tests/profile_probe.cpp)
//   gol_profile.cpp    the Profiler: per-pass event records and their fold, the
//                      in-kernel clock probe's buffer, gol_profile_*
//   gol_region.cpp     census, windowed pattern I/O, the density map and the
//                      pattern search (gol_census, gol_read_region,
//                      gol_write_region, gol_density, gol_find; the search
//                      kernel is gol_find.hip)
//   gol_batch.cpp      the batch engine (gol_batch_*, gol_cycle_*): a handle type
//                      of its own behind gol_batch.h, kernels in gol_batch.hip
//                      (their shared generation: gol_batch_gen.h); it takes the
//                      error state and the HIP status discipline from here
//
// Reference correspondence (src/main/scala/gameoflife/ of the reference):
//   gol_create   <- BoardCreator.createAllInitialActors (BoardCreator.scala:79-89)
//   gol_seed     <- initialState = Random.nextBoolean() per cell (BoardCreator.scala:23)
//   gol_step     <- NextStep tick -> CurrentEpochMsg -> gatherer -> SetNewStateMsg
//                   (BoardCreator.scala:113-116, CellActor.scala:63-91,
//                    NextStateCellGathererActor.scala:25-48)
//   gol_snapshot <- CellStateMsg -> LoggerActor (CellActor.scala:89, LoggerActor.scala:30-46)
//   gol_comm_*   <- cross-backend GetStateFromEpoch/StateForEpoch over Akka remote
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gol.h"
#include "gol_active.h"
#include "gol_kernels.h"
#include "gol_profile.h"

struct LoopRing;  // gol_loopback.cpp

// In-process shard group: shards in row order, linked into a ring (torus) or
// a chain (clipped); each shard's comm stream pulls its neighbours' edge rows.
struct gol_group {
    std::vector<gol_ctx*> shards;
    bool torus = true;
    std::string err;
};

#pragma GCC visibility push(hidden)
namespace golc {

// Generations a step plans, accumulates and folds at a time (step_chunks): the
// hash accumulators are allocated for one chunk, 4 MiB.
constexpr uint32_t kStepChunk = 1024;

// A device buffer that kernels sum into and its owner: the device words, the
// mapped page-locked words their fold / export kernel leaves the result in
// (none for a device-only buffer), and how much of the device words is known
// to be in the reset state, left so by that kernel.  Each owner resets in its
// own way (a memset, launch_census_reset) and reports a failure with its own
// code.  `count` and `clean` are in the owner's unit (generations of hash
// slots, counts, words).
template <class T>
struct Accum {
    T* dev = nullptr;
    T* host = nullptr;      // coherent: the fold's stores reach host memory without a cache flush
    T* host_dev = nullptr;  // ... its device address (the fold stores there)
    size_t count = 0;       // capacity; set only once every buffer exists
    size_t clean = 0;       // leading units of `dev` known to be in the reset state

    // Forgets the buffers before freeing them, so a failure leaves nothing to
    // free twice.  The first failing status.
    hipError_t release() {
        T* const d = dev;
        T* const h = host;
        dev = host = host_dev = nullptr;
        count = clean = 0;
        const hipError_t ed = d ? hipFree(d) : hipSuccess;
        const hipError_t eh = h ? hipHostFree(h) : hipSuccess;
        return ed != hipSuccess ? ed : eh;
    }
    // Holds `n` units afterwards: dev_words device words and host_words mapped
    // ones (0: device only), none of them clean.  A buffer that is too small
    // is replaced (nothing may be in flight on it); on failure nothing is held.
    hipError_t grow(size_t n, size_t dev_words, size_t host_words) {
        if (n <= count) return hipSuccess;
        hipError_t e = release();
        if (e == hipSuccess) e = hipMalloc(&dev, dev_words * sizeof(T));
        if (e == hipSuccess && host_words)
            e = hipHostMalloc((void**)&host, host_words * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess && host_words) e = hipHostGetDevicePointer((void**)&host_dev, host, 0);
        if (e == hipSuccess) count = n;
        else (void)release();
        return e;
    }
};

// The rows of a plane that can hold a live cell: every
// word of the plane outside `runs` (local rows) is zero, or nothing is known.
struct LiveRows {
    bool known = true;  // false: any row may be non-zero (`runs` is empty then)
    golactive::Runs runs;
};

// The parts of a profiled pass (gol_profile_stats): its main launch (the whole
// shard, or a sharded shard's interior rows), its halo exchange, its boundary launch.
enum ProfKind { kProfNone = -1, kProfMain = 0, kProfExchange = 1, kProfBoundary = 2 };

// One pass in the profiler's window.  Each part is a HIP event pair, created
// the first time this record's part is used, and whether each event has been
// recorded since the record was begun: the fold counts a part only if both were.
struct PassRecord {
    struct Part {
        hipEvent_t start = nullptr, stop = nullptr;
        bool started = false, stopped = false;
    } part[3];          // by ProfKind
    int clk_slot = -1;  // the main launch's clock-probe slot, or -1
    uint32_t gens = 0;  // generations the main launch advances
};

// Pass timing of a context (gol_profile.cpp): the switch, the totals, the
// window of pass records not yet folded into them and the clock-probe buffer.
// A method's failure is its HIP status.
struct Profiler {
    static constexpr size_t kMaxPairs = 4096;      // event pairs of a window
    static constexpr uint32_t kClockSlots = 1024;  // probe slots of a window, golprof::kClockSlotWords each
    bool on = false;
    golprof::Totals totals;  // since the last reset; the halo bytes are counted with the switch off too
    std::vector<PassRecord> window;
    size_t used = 0, pairs = 0;     // records begun and parts started since the last fold
    Accum<unsigned long long> clk;  // in slots, zero when clean, device only; handed out in order,
    uint32_t clk_used = 0;          // ... this many since the last fold

    hipError_t alloc_clock(hipStream_t stream);  // the buffer exists and is zero; on failure nothing is held
    // A record for the pass about to be enqueued (null: switched off).  Folds first when fewer than three
    // pairs are left: the only fold besides the readers', so no pass straddles one.
    hipError_t begin(PassRecord** rec, hipStream_t stream);
    // Bracket part `kind` on the stream it runs on; stop() does nothing unless start() recorded.
    hipError_t start(PassRecord* rec, ProfKind kind, hipStream_t stream);
    hipError_t stop(PassRecord* rec, ProfKind kind, hipStream_t stream);
    // The main launch advances `gens` generations; its probe slot, or null (no buffer, or none left).
    unsigned long long* main_launch(PassRecord* rec, int gens);
    hipError_t fold(hipStream_t stream);  // completed parts into the totals, used slots cleared; synchronises
    void destroy_events();                // teardown: failures are logged
};

}  // namespace golc
#pragma GCC visibility pop

struct gol_ctx {
    // geometry
    int64_t width = 0, height = 0, row0 = 0, rows = 0;
    int32_t wwords = 0;
    int64_t pitch = 0;
    int32_t topology = GOL_TORUS;
    uint32_t birth = 0, survive = 0;
    int64_t vis_w = 0, vis_h = 0;
    int ilv = 1;         // device words per interleave group: 1 row-major, 2 pairs
    int device = 0;
    int vec_fixed = 0;  // words per lane forced by gol_set_tuning (0: per-pass automatic)
    // device state
    uint32_t* plane[2] = {nullptr, nullptr};
    int cur = 0;
    uint32_t* halo_top = nullptr;  // RCCL receive buffers (sharded)
    uint32_t* halo_bot = nullptr;
    uint32_t* zero_row = nullptr;
    // per-generation sums, in generations: dev [count][kHashGenStride], zero when clean; host [2][count], the
    // folded hashes and then (gol_step_series) the populations
    golc::Accum<unsigned long long> sums;
    uint64_t epoch = 0;
    hipStream_t compute = nullptr, comm = nullptr;
    hipStream_t edge = nullptr;  // boundary-row kernels of a sharded pass (concurrent with the interior)
    hipEvent_t ev_ready = nullptr, ev_halo = nullptr, ev_edge = nullptr;
    // asynchronous snapshot (gol_snapshot_async / gol_snapshot_wait): the
    // board at the snapshot epoch, row-major, copied to the host on `xfer`
    // while later passes run on `compute`
    uint32_t* snap = nullptr;
    hipStream_t xfer = nullptr;
    hipEvent_t ev_snap_ready = nullptr, ev_snap_done = nullptr;
    bool snap_pending = false;
    uint64_t snap_epoch = 0;
    // census, windows and density map (gol_region.cpp), allocated on first use
    // and grown on demand: the staged window rows this shard owns (packed,
    // ceil(w / 32) words per row; device only), the census accumulators
    // (kCensusSlots * kCensusSlotStride, the identity when clean; host:
    // kCensusValues) and the grid the density kernels count into (in counts,
    // zero when clean; exported to the host before it is added to the caller's)
    golc::Accum<uint32_t> region_stage;
    golc::Accum<unsigned long long> census;
    golc::Accum<uint32_t> density;
    // pattern search (gol_find): the cared cells (device and page-locked host
    // words, in cells), the match counters (kFindWords, zero when clean; host:
    // kFindValues) and the hit list (in (x, y) pairs, device only)
    golc::Accum<uint32_t> find_cells;
    golc::Accum<unsigned long long> find_count;
    golc::Accum<long long> find_hits;
    // active-row stepping (gol_active.h, gol_active.cpp):
    // live[p] is kept for plane p by every writer of a plane, mode on or off
    golc::LiveRows live[2];                // gol_create clears both planes: known, no runs
    bool active_on = false;                // gol_set_active_rows
    int64_t active_scan_rows = 0;          // rows of the current plane's runs after the last scan
    int active_backoff = 0;                // passes between scans while they keep finding the board dense
    int active_wait = 0;                   // ... of them still to go before the next scan
    gol_active_stats active_stats{};
    golc::Accum<uint32_t> active_bits;     // the scan's block bitmap, one bit per kActiveBlock rows (in words)
    // RCCL
    ncclComm_t nccl = nullptr;
    int rank = 0, nranks = 1;
    // loopback ring (gol_comm_init_loopback): the same halo exchange between
    // contexts of one process, for tests; exclusive with nccl
    std::shared_ptr<LoopRing> loop;
    // in-process shard group (gol_group_*): halos by device-to-device copies
    gol_group* group = nullptr;
    int gindex = 0;
    // tuning
    int32_t band_rows = 0;                                   // 0: automatic
    int32_t gens_per_pass = 0;                               // temporal blocking depth (0: automatic)
    golc::Profiler profile;  // pass timing and the halo byte counters (gol_profile.cpp)
    // occupancy
    int num_cus = 0;
    mutable std::map<int, int64_t> occupancy_cache;  // resident_waves (a cache: const callers may fill it)
    std::string err;
};

#pragma GCC visibility push(hidden)
namespace golc {

// ---- errors and HIP / RCCL status discipline (gol_capi.cpp) ----------------

int set_err(gol_ctx* ctx, int code, const char* fmt, ...);

// HIP status discipline: a failing HIP call also
// leaves its status pending on the calling thread (hipGetLastError).  A
// failure libgol reports through its own return code is taken off the
// thread here, so no later call -- ours or the caller's -- inherits it.
int hip_fail(gol_ctx* ctx, hipError_t e, const char* expr, const char* file, int line);

#define HIP_CHECK(ctx, expr)                                                   \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) return golc::hip_fail((ctx), e_, #expr, __FILE__, __LINE__); \
    } while (0)

// A status whose failure only gets logged (teardown, best-effort calls):
// reported on stderr and taken off the thread.
void hip_note(hipError_t e, const char* what);

// RCCL runs HIP calls of its own on the calling thread and does not take the
// statuses it discards off the thread: after every RCCL call libgol makes,
// such a leftover is taken, counted and logged once (gol_diag_absorbed).
void absorb_rccl_status(const char* call, hipError_t pending_before);

#define NCCL_CHECK(ctx, expr)                                                                       \
    do {                                                                                            \
        const hipError_t pre_ = hipPeekAtLastError();                                               \
        ncclResult_t r_ = (expr);                                                                   \
        golc::absorb_rccl_status(#expr, pre_);                                                      \
        if (r_ != ncclSuccess)                                                                      \
            return golc::set_err((ctx), GOL_ECOMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), \
                                 __FILE__, __LINE__);                                               \
    } while (0)

// ---- context state (gol_capi.cpp) ------------------------------------------

// Any attached communicator runs the ring schedule, a 1-rank one included.
bool sharded(const gol_ctx* c);
bool in_ring(const gol_ctx* c);
// The B3/S23 torus: the only boards the fast-path kernel instances serve.
bool life_torus(const gol_ctx* c);
int bind(gol_ctx* ctx);
int device_ilv(int32_t topology, int64_t wwords);
void destroy_impl(gol_ctx* c);

// ---- pass schedule (gol_schedule.cpp) --------------------------------------

// Before a chunk that sums: accumulators for `gens` generations exist and are
// zero (a memset unless read_sums left them so); marks them in use.
int prepare_sums(gol_ctx* ctx, uint32_t gens);
// After the chunk's passes on the compute stream: its `gens` generations'
// hashes and populations, each into its array unless null, folded on the
// device straight into mapped host memory (the populations only if asked
// for), the accumulators cleared again; synchronises.
int read_sums(gol_ctx* ctx, uint32_t gens, uint64_t* hashes_out, uint64_t* populations_out);
int lane_words(const gol_ctx* ctx, int gens);
// The kernel instance a pass of `gens` generations runs on this context: the
// one place that derives it (and so a pass's strip width, gol::strip_words).
gol::StepInstance step_instance(const gol_ctx* ctx, int gens, bool hashed, bool pop = false);
int64_t resident_waves(const gol_ctx* ctx, const gol::StepInstance& k);
// Load every step kernel instance the context can launch at its current
// tuning (the occupancy query of an instance loads its code object).
void preload_instances(gol_ctx* ctx);

// Rows of the plane a launch steps and the global row of its local row 0:
// the context's own (default), or gol_replay's extended block.
struct PlaneGeom {
    int32_t rows;
    int64_t grow0;
};

// The per-generation series a pass with accumulators (slots) sums into them:
// the state hash (gol_step), the population (gol_step_series), or both.
enum Series { kSeriesHash = 1, kSeriesPop = 2 };

// What a pass accumulates and where: the accumulators of its first generation
// (null: it sums nothing) and the series it sums into them.
struct PassSums {
    unsigned long long* slots = nullptr;
    int series = 0;  // Series bits
};
// ... for a pass that starts `g` generations into the chunk the context's
// accumulators were prepared for (series 0: a pass that sums nothing).
inline PassSums pass_sums(const gol_ctx* ctx, int series, uint32_t g) {
    return series ? PassSums{ctx->sums.dev + (size_t)g * gol::kHashGenStride, series} : PassSums{};
}

// One launch of a pass: `gens` generations over local row ranges
// [lo[0], hi[0]) (+ [lo[1], hi[1]) if n == 2).
struct PassLaunch {
    int gens = 1;
    const uint32_t* cur = nullptr;       // local row 0 of the current plane
    uint32_t* nxt = nullptr;             // ... of the next plane
    const uint32_t* halo_top = nullptr;  // rows -gens .. -1 and rows .. rows + gens - 1, halo_stride words apart
    const uint32_t* halo_bot = nullptr;  // (0: one row repeated)
    int64_t halo_stride = 0;
    bool wrap_y = false;                 // unsharded torus: rows wrap inside the plane, no halo read
    PassSums sums;
    int n = 1;
    int32_t lo[2] = {0, 0}, hi[2] = {0, 0};
    ProfKind prof_kind = kProfMain;  // the part of a profiled pass this launch is (kProfNone: untimed) ...
    PassRecord* rec = nullptr;       // ... of this record; null: of a record of its own
    hipStream_t stream = nullptr;    // null: the compute stream
    const PlaneGeom* geom = nullptr;  // null: the context's own plane
};

// Column strips of a row for instance `k`; `halo_lanes`: as if the pass ran
// halo-lane strips even where it runs whole-row waves (the planner's
// small-board test).
int strip_count(const gol_ctx* ctx, gol::StepInstance k, bool halo_lanes = false);
int launch_ranges(gol_ctx* ctx, const PassLaunch& launch);
// `rec`: the pass's profiling record (null: each launch opens its own).
int sharded_interior(gol_ctx* ctx, int G, PassSums sums, bool has_up, bool has_down, PassRecord* rec);
int sharded_boundary(gol_ctx* ctx, int G, PassSums sums, bool has_up, bool has_down, const hipEvent_t* halo_ready,
                     int nready, PassRecord* rec);
int sharded_pass_kernels(gol_ctx* ctx, int G, PassSums sums, bool has_up, bool has_down,
                         const hipEvent_t* halo_ready, int nready);
int depth_cap(const gol_ctx* ctx);
std::vector<int> plan_passes(const gol_ctx* ctx, uint32_t n, bool hashed);

// The one chunk loop of every step: `generations` in chunks of kStepChunk,
// each planned on `ctx` (any series is planned as a hashed step is, DESIGN.md
// section 5d).  Per chunk of n generations: prepare(n), then pass(G, g) for
// each planned depth G, g generations into the chunk, then read(g0, n) for
// the chunk that began at generation g0.  Not `summed`: passes only.
template <class Prepare, class Pass, class Read>
int step_chunks(const gol_ctx* ctx, uint32_t generations, bool summed, Prepare prepare, Pass pass, Read read) {
    for (uint32_t g0 = 0; g0 < generations; g0 += kStepChunk) {
        const uint32_t n = std::min(kStepChunk, generations - g0);
        if (summed)
            if (int rc = prepare(n)) return rc;
        uint32_t g = 0;
        for (const int G : plan_passes(ctx, n, summed)) {
            if (int rc = pass(G, g)) return rc;
            g += (uint32_t)G;
        }
        if (summed)
            if (int rc = read(g0, n)) return rc;
    }
    return GOL_OK;
}

// ---- ring schedule (gol_ring.cpp) ------------------------------------------

// One point-to-point operation of a pass's halo exchange: send `count`
// words from `buf` to rank `peer`, or receive them into `buf` from it.
struct HaloOp {
    bool send;
    uint32_t* buf;
    size_t count;
    int peer;
};

int one_pass(gol_ctx* ctx, int G, PassSums sums);

// ---- loopback ring (gol_loopback.cpp) --------------------------------------

int loop_exchange(gol_ctx* ctx, const HaloOp* ops, int n);
int loop_allreduce(gol_ctx* ctx, uint64_t* values, uint32_t count);
void loop_leave(gol_ctx* ctx);

// ---- a context stepped whole, active rows (gol_active.cpp) -----------------

// The launches of an unsharded pass (L: everything but the row ranges) and
// what they make of the live rows of both planes.
int whole_pass(gol_ctx* ctx, PassLaunch L);

// What the writers of a plane owe the active-row invariant (LiveRows):
// plane p may now hold anything ...
inline void live_unknown(gol_ctx* ctx, int p) { ctx->live[p] = LiveRows{false, {}}; }
// ... or may have gained live cells in local rows [lo, hi) only.
inline void live_add(gol_ctx* ctx, int p, int64_t lo, int64_t hi) {
    LiveRows& l = ctx->live[p];
    if (!l.known) return;
    l.runs.push_back({(int32_t)lo, (int32_t)hi});
    l.runs = golactive::normalize(std::move(l.runs), (int32_t)ctx->rows);
}

// ---- shard groups (gol_group.cpp) ------------------------------------------

size_t group_size(const gol_group* g);
// gol_group_step_partials, or with populations_out the series call (no partials).
int group_step(gol_group* g, uint32_t generations, uint64_t* hashes_out, uint64_t* partials_out,
               uint64_t* populations_out);
int64_t group_min_rows(const gol_group* g);

// ---- checkpoints (gol_checkpoint.cpp) --------------------------------------

struct CkptHeader {
    char magic[8];  // "GOLCKPT1"
    int64_t width, height, row0, rows;
    int64_t wwords;
    uint64_t epoch;
    int32_t topology;
    uint32_t birth, survive;
    int32_t pad;
};

}  // namespace golc
#pragma GCC visibility pop
