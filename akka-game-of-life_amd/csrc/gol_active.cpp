// gol_active.cpp -- the pass of a context stepped whole (no ring, no group):
// one launch over every row, or -- with active-row stepping on
// (gol_set_active_rows) -- one launch per run of rows
// that can hold a live cell.  The rules are pure functions in gol_active.h;
// this unit applies them to the context and keeps its LiveRows.
#include <algorithm>

#include "gol_ctx.h"

using namespace golc;

namespace {

static_assert(golactive::kActiveBlock == gol::kOccupancyBlock, "the scan's blocks are the runs' blocks");

golactive::Runs whole_plane(const gol_ctx* ctx) { return {{0, (int32_t)ctx->rows}}; }

// live[cur] from the device: the blocks of its runs (of the whole plane if
// nothing is known) that hold a non-zero word.  On the compute stream, after
// every queued pass; synchronises.
int scan_live(gol_ctx* ctx) {
    LiveRows& live = ctx->live[ctx->cur];
    const int32_t rows = (int32_t)ctx->rows;
    const golactive::Runs todo = live.known ? live.runs : whole_plane(ctx);
    ++ctx->active_stats.scans;
    if (!todo.empty()) {
        const int32_t nblocks = (rows + golactive::kActiveBlock - 1) / golactive::kActiveBlock;
        const int32_t nwords = (nblocks + 31) / 32;
        Accum<uint32_t>& bits = ctx->active_bits;
        HIP_CHECK(ctx, bits.grow((size_t)nwords, (size_t)nwords, (size_t)nwords));
        if (!bits.clean) HIP_CHECK(ctx, hipMemsetAsync(bits.dev, 0, (size_t)nwords * sizeof(uint32_t), ctx->compute));
        bits.clean = 0;  // in use until the export has left it zero
        for (const golactive::Run& r : todo) {
            HIP_CHECK(ctx, gol::launch_row_occupancy(ctx->plane[ctx->cur], ctx->pitch, ctx->wwords, r.lo, r.hi,
                                                     bits.dev, nwords, ctx->compute));
            ctx->active_stats.rows_scanned += (uint64_t)(r.hi - r.lo);
        }
        HIP_CHECK(ctx, gol::launch_density_export(bits.dev, bits.host_dev, nwords, ctx->compute));
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
        bits.clean = bits.count;
        live.runs = golactive::from_bitmap(bits.host, 0, nblocks, rows);
        live.known = true;
    }
    ctx->active_scan_rows = golactive::row_count(live.runs);
    return GOL_OK;
}

// The unsharded pass with the mode on (birth on 0 neighbours excluded by the
// caller): scan if due, grow the current plane's runs by the depth, and step
// them alone -- one launch per run, so the occupancy-based band rules and the
// small-board cut size each -- after clearing what the destination plane held
// outside them.  *stepped = false: the runs cover more than half the plane (or
// nothing is known and no scan is due yet), and the caller runs the pass as
// one launch over every row.
int active_pass(gol_ctx* ctx, PassLaunch L, bool* stepped) {
    using namespace golactive;
    const int32_t rows = (int32_t)ctx->rows;
    const int nxt = ctx->cur ^ 1;
    gol_active_stats& st = ctx->active_stats;
    *stepped = false;
    ++st.passes;
    bool scanned = false;
    {
        const LiveRows& live = ctx->live[ctx->cur];
        if (!live.known || scan_due(live.known ? row_count(live.runs) : rows, ctx->active_scan_rows)) {
            if (ctx->active_wait > 0) {
                --ctx->active_wait;
            } else {
                if (int rc = scan_live(ctx)) return rc;
                scanned = true;
            }
        }
    }
    const LiveRows& live = ctx->live[ctx->cur];
    Runs run = dilate(live.known ? live.runs : whole_plane(ctx), L.gens, rows, L.wrap_y);
    if (dense(row_count(run), rows) && !scanned && ctx->active_wait == 0 && live.known &&
        row_count(live.runs) < rows) {
        // runs that have grown past half the plane since their last scan: look before giving them up
        if (int rc = scan_live(ctx)) return rc;
        scanned = true;
        run = dilate(live.runs, L.gens, rows, L.wrap_y);
    }
    if (dense(row_count(run), rows)) {
        // a scan that leaves the pass dense lengthens the wait for the next one (next_backoff); without a
        // scan -- still waiting, or nothing known -- the wait just runs down
        if (scanned) ctx->active_wait = ctx->active_backoff = next_backoff(ctx->active_backoff);
        ctx->active_scan_rows = 0;  // whole-plane runs are due for a scan as soon as the wait is over
        ctx->live[nxt] = LiveRows{true, whole_plane(ctx)};
        st.rows_stepped += (uint64_t)rows;
        return GOL_OK;
    }
    ctx->active_backoff = ctx->active_wait = 0;
    uint32_t* const nplane = ctx->plane[nxt];
    for (const Run& r : subtract(ctx->live[nxt].known ? ctx->live[nxt].runs : whole_plane(ctx), run)) {
        HIP_CHECK(ctx, hipMemsetAsync(nplane + (int64_t)r.lo * ctx->pitch, 0,
                                      (size_t)(r.hi - r.lo) * ctx->pitch * sizeof(uint32_t), ctx->compute));
        st.rows_cleared += (uint64_t)(r.hi - r.lo);
    }
    // whatever happens to the launches below, the destination plane is zero outside the runs
    ctx->live[nxt] = LiveRows{true, run};
    size_t largest = 0;
    for (size_t k = 1; k < run.size(); ++k)
        if (run[k].hi - run[k].lo > run[largest].hi - run[largest].lo) largest = k;
    for (size_t k = 0; k < run.size(); ++k) {
        L.n = 1;
        L.lo[0] = run[k].lo;
        L.hi[0] = run[k].hi;
        L.prof_kind = k == largest ? kProfMain : kProfNone;
        if (int rc = launch_ranges(ctx, L)) return rc;
    }
    ++st.sparse_passes;
    st.rows_stepped += (uint64_t)row_count(run);
    *stepped = true;
    return GOL_OK;
}

}  // namespace

// Active-row stepping.  Without birth on 0 neighbours a
// dead cell with no live neighbour stays dead on both topologies, so the live
// cells of every generation of the pass lie within the current plane's runs
// grown by G rows: stepping those rows alone gives the same plane and, summed
// over them, the same hashes and populations (a row that is not launched is
// dead and adds 0).
int golc::whole_pass(gol_ctx* ctx, PassLaunch L) {
    const int32_t rows = (int32_t)ctx->rows;
    const bool quiet = (ctx->birth & 1u) == 0;  // nothing is born in empty space
    bool stepped = false;
    if (ctx->active_on && quiet) {
        if (int rc = active_pass(ctx, L, &stepped)) return rc;
    } else {
        // mode off: one launch over every row writes the whole next plane;
        // its live rows follow from the current plane's where those are known
        const LiveRows& live = ctx->live[ctx->cur];
        ctx->live[ctx->cur ^ 1] = live.known && quiet
                                      ? LiveRows{true, golactive::dilate(live.runs, L.gens, rows, L.wrap_y)}
                                      : LiveRows{false, {}};
        if (ctx->active_on) {
            ++ctx->active_stats.passes;
            ctx->active_stats.rows_stepped += (uint64_t)rows;
        }
    }
    if (stepped) return GOL_OK;
    L.hi[0] = rows;
    return launch_ranges(ctx, L);
}

extern "C" {

int gol_set_active_rows(gol_ctx* ctx, int32_t enable) {
    if (!ctx) return set_err(nullptr, GOL_EINVAL, "null context");
    if (enable != 0 && enable != 1) return set_err(ctx, GOL_EINVAL, "gol_set_active_rows: enable must be 0 or 1");
    if (enable && !ctx->active_on) ctx->active_backoff = ctx->active_wait = 0;  // the first pass may scan
    ctx->active_on = enable != 0;
    return GOL_OK;
}

int gol_active_stats_read(gol_ctx* ctx, gol_active_stats* out, int32_t reset) {
    if (!ctx || !out) return set_err(ctx, GOL_EINVAL, "gol_active_stats_read: null argument");
    *out = ctx->active_stats;
    if (reset) ctx->active_stats = gol_active_stats{};
    return GOL_OK;
}

int gol_active_rows(gol_ctx* ctx, int64_t* lo_hi_pairs, int32_t max_runs, int32_t* count) {
    if (!ctx || !count || (max_runs > 0 && !lo_hi_pairs))
        return set_err(ctx, GOL_EINVAL, "gol_active_rows: null argument");
    const LiveRows& live = ctx->live[ctx->cur];
    if (!live.known) {
        *count = -1;
        return GOL_OK;
    }
    for (size_t k = 0; k < live.runs.size() && (int32_t)k < max_runs; ++k) {
        lo_hi_pairs[2 * k] = ctx->row0 + live.runs[k].lo;
        lo_hi_pairs[2 * k + 1] = ctx->row0 + live.runs[k].hi;
    }
    *count = (int32_t)live.runs.size();
    return GOL_OK;
}

}  // extern "C"
