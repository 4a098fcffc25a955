// gol_schedule.cpp -- the pass schedule of a context: which kernel instance,
// lane width and strip count a pass of G generations launches with, the
// launches of a pass (whole shard, or the interior and boundary rows of a
// sharded one) and the pass plan.  The rules themselves -- band heights, the
// small-board cut, the tail split, the XCD block order and the depth planner
// -- are pure functions in gol_plan.h; this unit gathers their inputs from the
// context and the environment.  DESIGN.md section 4.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gol_ctx.h"
#include "gol_plan.h"

static_assert(golplan::kMaxGens == gol::kMaxGensPerPass, "the pass cost table covers every depth the kernels run");

namespace {

// GOL_XCD_CHUNK (golplan::xcd_chunk), read once per process.
int xcd_chunk_env() {  // 0: not set
    static const int c = [] {
        const char* e = getenv("GOL_XCD_CHUNK");
        if (!e) return 0;
        const int v = atoi(e);
        return v < 1 ? 1 : (v > 64 ? 64 : v);
    }();
    return c;
}

// GOL_TAIL="frac,div" (golplan::tail_split), read at every launch that
// considers a tail split: the sweep scripts change it inside one process.
golplan::TailOverride tail_env() {
    golplan::TailOverride t;
    const char* env = getenv("GOL_TAIL");
    t.present = env != nullptr;
    t.set = env && *env;
    if (t.set && sscanf(env, "%lf,%d", &t.frac, &t.div) != 2) t.frac = 0.0;
    return t;
}

// Words per lane for a single-generation pass: 16-byte lane loads where the
// row fills whole waves of them.
int default_vec(int64_t wwords) {
    return (wwords % 4 == 0 && wwords >= 256) ? 4 : (wwords % 2 == 0 && wwords >= 128) ? 2 : 1;
}

// Planned (not fixed) passes deeper than kMaxGensPlannedGeneric run only on
// the B3/S23 torus kernels: the generic-rule and clipped instances hold their
// rule masks / visibility planes in registers and drop to 2 waves per SIMD at
// G >= 10 (scripts/resource_usage.py), and the cost table is measured on the
// B3/S23 torus.
constexpr int kMaxGensPlannedGeneric = 8;

}  // namespace

namespace golc {

int prepare_sums(gol_ctx* ctx, uint32_t gens) {
    // one allocation for a whole chunk (kStepChunk generations, 4 MiB): a
    // hipFree + hipMalloc between two hashed calls would synchronise the
    // device inside the caller's step.  The mapped words hold the hash sums,
    // then the populations of a series call (read_sums).
    const size_t cap = std::max(gens, kStepChunk);
    HIP_CHECK(ctx, ctx->sums.grow(cap, cap * gol::kHashGenStride, 2 * cap));
    const bool clean = ctx->sums.clean >= gens;
    ctx->sums.clean = 0;  // in use until read_sums clears them again
    if (!clean)
        HIP_CHECK(ctx, hipMemsetAsync(ctx->sums.dev, 0, (size_t)gens * gol::kHashGenStride * sizeof(unsigned long long),
                                      ctx->compute));
    return GOL_OK;
}

// Per call (scripts/tick_cost.py): a hashed step(1) on the 7 x 7 default
// board went from 22.0 us (memset + pass + 4 KiB readback) to 20.4 (pass +
// fold into mapped memory); configs[1]'s hashed 1000 generations from 1.96 to
// 1.72 ms (8 bytes per generation cross PCIe instead of 4 KiB).
int read_sums(gol_ctx* ctx, uint32_t gens, uint64_t* hashes_out, uint64_t* populations_out) {
    const Accum<unsigned long long>& a = ctx->sums;
    const size_t pop0 = a.count;  // the populations' half of the mapped words
    HIP_CHECK(ctx, populations_out
                       ? gol::launch_fold_series(a.dev, gens, a.host_dev, a.host_dev + pop0, ctx->compute)
                       : gol::launch_fold(a.dev, gens, a.host_dev, ctx->compute));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
    if (hashes_out) std::memcpy(hashes_out, a.host, gens * sizeof(uint64_t));
    if (populations_out) std::memcpy(populations_out, a.host + pop0, gens * sizeof(uint64_t));
    ctx->sums.clean = gens;
    return GOL_OK;
}

// Words per lane for a pass of `gens` generations.  Multi-generation strips
// carry 62 output lanes, so a row of w words needs ceil(w / (62 v)) strips;
// prefer 16-byte lanes unless 8-byte lanes waste clearly fewer lanes.
int lane_words(const gol_ctx* ctx, int gens) {
    // the pair layout needs whole pairs per lane: 8- or 16-byte lanes
    if (ctx->vec_fixed > 0) return std::max(ctx->vec_fixed, ctx->ilv);
    const int64_t w = ctx->wwords;
    if (gens == 1) return ctx->ilv == 2 ? std::max(default_vec(w), 2) : default_vec(w);
    // the horizontal-first kernel keeps 3 planes per ring row: 8-byte lanes
    // (95 VGPRs at G = 6, 5 waves/SIMD) beat 16-byte lanes (183 VGPRs, 2 waves;
    // those run the vertical-first kernel, +9 % at 262144^2 and +24 % at
    // 65536^2 for 8-byte horizontal-first lanes, profiles/r01_variant_ab.txt)
    const bool ok2 = w % 2 == 0 && w >= 2 * 62;
    return ok2 || ctx->ilv == 2 ? 2 : 1;
}

gol::StepInstance step_instance(const gol_ctx* ctx, int gens, bool hashed, bool pop) {
    gol::StepInstance k{};
    k.vec = lane_words(ctx, gens);
    k.gens = gens;
    k.ilv = ctx->ilv;
    k.life = life_torus(ctx);
    k.hash = hashed;
    k.pop = pop;
    k.clipped = ctx->topology == GOL_REF_CLIPPED;
    k.whole_row =
        gol::whole_row_fits(k.vec, gens, k.life, k.clipped, k.ilv, ctx->topology == GOL_TORUS, ctx->wwords);
    return k;
}

// Resident waves on the whole GPU for a launch (cached occupancy query).
int64_t resident_waves(const gol_ctx* ctx, const gol::StepInstance& k) {
    const int key = ((((((k.vec * 16 + k.gens) * 2 + k.life) * 2 + k.hash) * 2 + k.clipped) * 2 + k.whole_row) * 8 +
                     k.ilv) * 2 + k.pop;
    auto it = ctx->occupancy_cache.find(key);
    if (it != ctx->occupancy_cache.end()) return it->second;
    const int64_t waves = (int64_t)gol::resident_blocks_per_cu(k) * gol::kWavesPerWG * ctx->num_cus;
    ctx->occupancy_cache[key] = waves;
    return waves;
}

void preload_instances(gol_ctx* ctx) {
    // unbuilt instances (16-byte generic / clipped lanes deeper than
    // kMaxGensVec4Generic, gol_stencil.h kBuilt) report 0 blocks without a load.
    // The population-series instances are left to their first use: their code
    // objects would lengthen every gol_create for the callers of one entry point.
    for (int G = 1; G <= gol::kMaxGensPerPass; ++G)
        for (int h = 0; h < 2; ++h) (void)resident_waves(ctx, step_instance(ctx, G, h != 0));
}

// Column strips of a row for instance `k`: the one place that divides the row
// by gol::strip_words (gol_occupancy reports that width).  `halo_lanes`: count
// strips of 62 output lanes even where the pass runs whole-row waves.
int strip_count(const gol_ctx* ctx, gol::StepInstance k, bool halo_lanes) {
    if (halo_lanes) k.whole_row = false;
    const int sw = gol::strip_words(k);
    return (int)((ctx->wwords + sw - 1) / sw);
}

// Launch one pass (PassLaunch, gol_ctx.h).  With profiling on, the launch is
// bracketed as the part L.prof_kind of the pass's record L.rec, or of a record
// of its own (a pass of one timed launch: stepped whole, or a group shard's).
int launch_ranges(gol_ctx* ctx, const PassLaunch& L) {
    const hipStream_t stream = L.stream ? L.stream : ctx->compute;
    const bool acc = L.sums.slots != nullptr;
    const gol::StepInstance k = step_instance(ctx, L.gens, acc && (L.sums.series & kSeriesHash) != 0,
                                              acc && (L.sums.series & kSeriesPop) != 0);
    const int strips = strip_count(ctx, k);
    const golplan::BandPlan bp = golplan::band_plan(L.n, L.lo, L.hi, strips, L.gens, resident_waves(ctx, k),
                                                    ctx->band_rows, tail_env, gol::kWavesPerWG);
    if (bp.waves == 0) return GOL_OK;
    gol::StepParams p{};
    p.cur = L.cur;
    p.nxt = L.nxt;
    p.halo_top = L.halo_top;
    p.halo_bot = L.halo_bot;
    p.halo_stride = L.halo_stride;
    p.wrap_y = L.wrap_y ? 1 : 0;
    p.hash_slots = L.sums.slots;
    p.pitch = ctx->pitch;
    p.grow0 = L.geom ? L.geom->grow0 : ctx->row0;
    p.vis_rows = ctx->topology == GOL_TORUS ? ctx->height : ctx->vis_h;
    p.vis_cols = ctx->topology == GOL_TORUS ? ctx->width : ctx->vis_w;
    p.width = ctx->width;
    p.wwords = ctx->wwords;
    p.rows = L.geom ? L.geom->rows : (int32_t)ctx->rows;
    p.strips = strips;
    for (int r = 0; r < 2; ++r) {
        p.row_lo[r] = bp.row_lo[r];
        p.row_hi[r] = bp.row_hi[r];
        p.band[r] = bp.band[r];
        p.nbands[r] = bp.nbands[r];
    }
    p.wrap_x = ctx->topology == GOL_TORUS ? 1 : 0;
    p.birth = ctx->birth;
    p.survive = ctx->survive;
    p.xcd_chunk = golplan::xcd_chunk(L.gens, strips, xcd_chunk_env(), gol::kWavesPerWG);
    PassRecord* rec = L.prof_kind != kProfNone ? L.rec : nullptr;
    if (!rec && L.prof_kind != kProfNone) HIP_CHECK(ctx, ctx->profile.begin(&rec, ctx->compute));
    p.clk = rec && L.prof_kind == kProfMain ? ctx->profile.main_launch(rec, L.gens) : nullptr;
    if (rec) HIP_CHECK(ctx, ctx->profile.start(rec, L.prof_kind, stream));
    HIP_CHECK(ctx, gol::launch_step(p, k, bp.grid, 1, stream));
    if (rec) HIP_CHECK(ctx, ctx->profile.stop(rec, L.prof_kind, stream));
    return GOL_OK;
}

// What every launch of a sharded pass shares: the planes, the received halos
// at the plane's pitch and the accumulators.  A missing neighbour (clipped board
// ends) reads dead rows: zero_row holds kMaxGensPerPass of them at the halo
// pitch.  The caller sets the ranges, the profiling part and the stream.
static PassLaunch sharded_launch(gol_ctx* ctx, int G, PassSums sums, bool has_up, bool has_down, PassRecord* rec) {
    PassLaunch L;
    L.gens = G;
    L.cur = ctx->plane[ctx->cur];
    L.nxt = ctx->plane[ctx->cur ^ 1];
    L.halo_top = has_up ? ctx->halo_top : ctx->zero_row;
    L.halo_bot = has_down ? ctx->halo_bot : ctx->zero_row;
    L.halo_stride = ctx->pitch;
    L.sums = sums;
    L.rec = rec;
    return L;
}

// The interior rows [G, rows - G) of a sharded pass on the compute stream:
// they read no halo, so they are enqueued before the exchange (one_pass) and
// run while it is in flight.  Shards of <= 2G rows have no interior.
int sharded_interior(gol_ctx* ctx, int G, PassSums sums, bool has_up, bool has_down, PassRecord* rec) {
    const int32_t rows = (int32_t)ctx->rows;
    if (rows <= 2 * G) return GOL_OK;
    PassLaunch L = sharded_launch(ctx, G, sums, has_up, has_down, rec);
    L.lo[0] = G;
    L.hi[0] = rows - G;
    return launch_ranges(ctx, L);
}

// The rest of a sharded pass once every event in `halo_ready` has fired: the
// two boundary row blocks on the edge stream, or the whole shard when it has
// no interior (the pass's main launch then).  The boundary launch runs
// concurrently with the tail of the interior one (its waves take the slots the
// interior's waves free) instead of after it; the compute stream then waits
// for it, so the next pass, a snapshot or a hash sees the whole plane.
int sharded_boundary(gol_ctx* ctx, int G, PassSums sums, bool has_up, bool has_down, const hipEvent_t* halo_ready,
                     int nready, PassRecord* rec) {
    const int32_t rows = (int32_t)ctx->rows;
    PassLaunch L = sharded_launch(ctx, G, sums, has_up, has_down, rec);
    if (rows > 2 * G) {
        // The exchange events follow this pass's ev_ready, recorded on the
        // compute stream after the previous pass's boundary rows: every
        // reader of the plane the boundary kernels overwrite has finished.
        for (int e = 0; e < nready; ++e) HIP_CHECK(ctx, hipStreamWaitEvent(ctx->edge, halo_ready[e], 0));
        L.n = 2;
        L.lo[0] = 0;
        L.hi[0] = G;
        L.lo[1] = rows - G;
        L.hi[1] = rows;
        L.prof_kind = kProfBoundary;
        L.stream = ctx->edge;
        if (int rc = launch_ranges(ctx, L)) return rc;
        HIP_CHECK(ctx, hipEventRecord(ctx->ev_edge, ctx->edge));
        HIP_CHECK(ctx, hipStreamWaitEvent(ctx->compute, ctx->ev_edge, 0));
        return GOL_OK;
    }
    for (int e = 0; e < nready; ++e) HIP_CHECK(ctx, hipStreamWaitEvent(ctx->compute, halo_ready[e], 0));
    L.lo[0] = 0;
    L.hi[0] = rows;
    return launch_ranges(ctx, L);
}

// Kernels of one sharded pass whose halos are already on their way (the
// in-process group): the interior rows, then the boundary rows after
// `halo_ready`, each timed as a record of its own (not tied to one another).
int sharded_pass_kernels(gol_ctx* ctx, int G, PassSums sums, bool has_up, bool has_down,
                         const hipEvent_t* halo_ready, int nready) {
    if (int rc = sharded_interior(ctx, G, sums, has_up, has_down, nullptr)) return rc;
    return sharded_boundary(ctx, G, sums, has_up, has_down, halo_ready, nready, nullptr);
}

// Deepest pass the context may run.  Every shard of a ring must pick the
// same depths (their halo messages must match), so a sharded pass is capped
// by the smallest shard of the decomposition, floor(H / N) (a 1-rank ring
// sends G of its own rows: G <= H).
int depth_cap(const gol_ctx* ctx) {
    int64_t G = ctx->gens_per_pass > 0 ? ctx->gens_per_pass
                                       : (life_torus(ctx) ? gol::kMaxGensPerPass : kMaxGensPlannedGeneric);
    G = std::min<int64_t>(G, gol::kMaxGensPerPass);
    // 16-byte lanes (forced by tuning): the generic-rule / clipped instances
    // deeper than this spill and are not built (gol_set_tuning refuses them
    // as fixed depths with words_per_lane = 4)
    if (ctx->vec_fixed == 4 && !life_torus(ctx)) G = std::min<int64_t>(G, gol::kMaxGensVec4Generic);
    if (in_ring(ctx)) G = std::min<int64_t>(G, ctx->height / ctx->nranks);
    if (ctx->group) G = std::min<int64_t>(G, group_min_rows(ctx->group));
    return (int)std::max<int64_t>(G, 1);
}

// A B3/S23 torus stepped whole (no ring, no group) whose 10-generation
// passes fall under the small-board cut (golplan::small_board_band).  There
// the hashed passes follow the unhashed cost row: the hashed narrow row
// (measured at 65536^2) ties G = 7 with G = 10, but on small boards a launch
// costs nearly the same at any depth and G = 7 runs 1.4 x the launches.
// Same-box sweep, 1000 generations, hashed, us per generation, G = 7 / 10
// (scripts/small_depth.py, profiles/r06_small_depth.txt): 1024^2 2.99 / 2.72,
// 4096^2 3.27 / 2.96, 8192^2 5.15 / 4.08, 16384^2 6.97 / 7.08, 32768^2 15.33 /
// 15.33.
static bool small_board(const gol_ctx* ctx) {
    if (sharded(ctx) || ctx->group || !life_torus(ctx) || depth_cap(ctx) < 10) return false;
    const int G = 10;
    const gol::StepInstance k = step_instance(ctx, G, true);
    // sized with halo-lane strips even where the pass runs whole-row waves:
    // whether that should change needs a measurement (small_board)
    const int strips = strip_count(ctx, k, /*halo_lanes=*/true);
    const int32_t lo[1] = {0}, hi[1] = {(int32_t)ctx->rows};
    const auto no_override = [] { return golplan::TailOverride{}; };  // the cut does not depend on GOL_TAIL
    return golplan::band_plan(1, lo, hi, strips, G, resident_waves(ctx, k), ctx->band_rows, no_override,
                              gol::kWavesPerWG)
        .small;
}

// Depths of the passes that advance `n` generations (golplan::plan_depths):
// a fixed gens_per_pass (tuning) is taken literally, otherwise the cost row is
// the board's -- wide or narrow by the strips of a 6-generation pass, hashed
// unless the board is a small one.
// Deterministic in (width, height, N, n), so all shards of a ring plan alike.
std::vector<int> plan_passes(const gol_ctx* ctx, uint32_t n, bool hashed) {
    const bool wide = strip_count(ctx, step_instance(ctx, 6, hashed)) >= 32;
    return golplan::plan_depths(n, depth_cap(ctx), ctx->gens_per_pass, hashed && !small_board(ctx), wide);
}

}  // namespace golc
