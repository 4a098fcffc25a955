// gol_region.cpp -- the board from the user's side without moving a plane:
// gol_census (population and bounding box, one pass on the device),
// gol_read_region and gol_write_region (a window of the torus or of the
// clipped board, gathered from / scattered into the device layout) and
// gol_density (the live cells per tile of a window: the zoomed-out view) and
// gol_find (every occurrence of a pattern among a window of anchors).  They
// stand for what the reference offered at 7 x 7: the per-cell initialState of
// BoardCreator.scala:65-70, the CellStateMsg stream a LoggerActor prints
// (CellActor.scala:89, LoggerActor.scala:30-46) and the counting a reader of
// that log does by eye.
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "gol_ctx.h"

using namespace golc;

namespace {

// A contiguous run of window rows this shard owns: window rows
// [win_row, win_row + count) are the shard's local rows from local_row on.
struct RowRun {
    int64_t win_row, count, local_row;
};

// The window rows y0 .. y0 + h - 1 (modulo the height) that fall into the
// shard: at most two runs, one on each side of the y seam.
int owned_runs(const gol_ctx* ctx, int64_t y0, int64_t h, RowRun runs[2]) {
    int n = 0;
    const int64_t first = std::min(h, ctx->height - y0);  // window rows before the seam
    const int64_t seg[2][3] = {{0, first, y0}, {first, h, y0 - ctx->height}};  // [lo, hi) and board row - window row
    for (const auto& s : seg) {
        const int64_t lo = std::max(s[0], ctx->row0 - s[2]);
        const int64_t hi = std::min(s[1], ctx->row0 + ctx->rows - s[2]);
        if (lo < hi) runs[n++] = {lo, hi - lo, lo + s[2] - ctx->row0};
    }
    return n;
}

// The window rules every windowed call shares (include/gol.h "The window").
int check_window(gol_ctx* ctx, const char* what, int64_t x0, int64_t y0, int64_t w, int64_t h, const void* buf) {
    if (!ctx) return set_err(nullptr, GOL_EINVAL, "%s: null context", what);
    if (!buf) return set_err(ctx, GOL_EINVAL, "%s: null buffer", what);
    if (w < 1 || w > ctx->width || h < 1 || h > ctx->height || x0 < 0 || x0 >= ctx->width || y0 < 0 ||
        y0 >= ctx->height)
        return set_err(ctx, GOL_EINVAL, "%s: window %lld x %lld at (%lld, %lld) does not fit a %lld x %lld board", what,
                       (long long)w, (long long)h, (long long)x0, (long long)y0, (long long)ctx->width,
                       (long long)ctx->height);
    if (ctx->topology == GOL_REF_CLIPPED && (x0 + w > ctx->width || y0 + h > ctx->height))
        return set_err(ctx, GOL_EINVAL, "%s: window %lld x %lld at (%lld, %lld) leaves the clipped %lld x %lld board",
                       what, (long long)w, (long long)h, (long long)x0, (long long)y0, (long long)ctx->width,
                       (long long)ctx->height);
    return GOL_OK;
}

// ... and a packed window buffer's pitch.
int check_window(gol_ctx* ctx, const char* what, int64_t x0, int64_t y0, int64_t w, int64_t h, const void* buf,
                 int64_t host_pitch_words) {
    if (int rc = check_window(ctx, what, x0, y0, w, h, buf)) return rc;
    if (host_pitch_words < (w + 31) / 32)
        return set_err(ctx, GOL_EINVAL, "%s: host pitch %lld < %lld words per window row", what,
                       (long long)host_pitch_words, (long long)((w + 31) / 32));
    return GOL_OK;
}

// The staging buffer holds `words` words.  Nothing is in flight on it between
// calls: both region calls synchronise before they return.
int ensure_stage(gol_ctx* ctx, size_t words) {
    if (ctx->region_stage.grow(words, words, 0) == hipSuccess) return GOL_OK;
    (void)hipGetLastError();
    return set_err(ctx, GOL_ENOMEM, "hipMalloc of %zu bytes for the window staging buffer failed",
                   words * sizeof(uint32_t));
}

// The density grid and the mapped page-locked words it is exported to hold
// `words` counts.  Nothing is in flight on them between calls: gol_density
// synchronises before it adds.
int ensure_density(gol_ctx* ctx, size_t words) {
    if (ctx->density.grow(words, words, words) == hipSuccess) return GOL_OK;
    (void)hipGetLastError();
    return set_err(ctx, GOL_ENOMEM, "allocating %zu bytes for the density map on the device and the host failed",
                   words * sizeof(uint32_t));
}

// gol_find's device buffers: `cells` cared cells (device and page-locked host
// words), the counters, and a hit list of `pairs` (x, y) pairs.  Nothing is in
// flight on them between calls: gol_find synchronises before it returns.
int ensure_find(gol_ctx* ctx, size_t cells, size_t pairs) {
    hipError_t e = ctx->find_cells.grow(cells, cells, cells);
    if (e == hipSuccess) e = ctx->find_count.grow(1, gol::kFindWords, gol::kFindValues);
    if (e == hipSuccess && pairs) e = ctx->find_hits.grow(pairs, 2 * pairs, 0);
    if (e == hipSuccess) return GOL_OK;
    (void)hipGetLastError();
    return set_err(ctx, GOL_ENOMEM, "allocating the pattern (%zu cells) and a hit list of %zu matches on the device failed",
                   cells, pairs);
}

}  // namespace

extern "C" {

int gol_census(gol_ctx* ctx, gol_census_result* out) {
    if (!ctx || !out) return set_err(ctx, GOL_EINVAL, "gol_census: null argument");
    if (int rc = bind(ctx)) return rc;
    Accum<unsigned long long>& acc = ctx->census;
    HIP_CHECK(ctx, acc.grow(1, (size_t)gol::kCensusSlots * gol::kCensusSlotStride, gol::kCensusValues));
    if (!acc.clean) HIP_CHECK(ctx, gol::launch_census_reset(acc.dev, ctx->compute));
    acc.clean = 0;  // in use until the fold has left the identity behind
    HIP_CHECK(ctx, gol::launch_census(ctx->plane[ctx->cur], ctx->pitch, ctx->wwords, ctx->row0, (int32_t)ctx->rows,
                                      ctx->ilv, acc.dev, ctx->compute));
    HIP_CHECK(ctx, gol::launch_census_fold(acc.dev, acc.host_dev, ctx->compute));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
    acc.clean = 1;
    const unsigned long long* v = acc.host;
    out->population = v[0];
    out->min_x = (int64_t)v[1];
    out->max_x = (int64_t)v[2];
    out->min_y = (int64_t)v[3];
    out->max_y = (int64_t)v[4];
    return GOL_OK;
}

int gol_read_region(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h, uint32_t* packed_out,
                    int64_t host_pitch_words) {
    if (int rc = check_window(ctx, "gol_read_region", x0, y0, w, h, packed_out, host_pitch_words)) return rc;
    RowRun runs[2];
    const int nruns = owned_runs(ctx, y0, h, runs);
    if (nruns == 0) return GOL_OK;  // the window misses this shard
    if (int rc = bind(ctx)) return rc;
    const int64_t sw = (w + 31) / 32;
    int64_t owned = 0;
    for (int k = 0; k < nruns; ++k) owned += runs[k].count;
    if (int rc = ensure_stage(ctx, (size_t)(owned * sw))) return rc;
    // gathered on the compute stream: after every queued pass, straight from
    // the current plane (the pair layout is undone per word, no spare plane)
    uint32_t* stage = ctx->region_stage.dev;
    for (int k = 0; k < nruns; ++k) {
        const RowRun& r = runs[k];
        HIP_CHECK(ctx, gol::launch_region_gather(ctx->plane[ctx->cur] + r.local_row * ctx->pitch, ctx->pitch,
                                                 ctx->wwords, ctx->ilv, (int32_t)r.count, x0, w, stage, ctx->compute));
        HIP_CHECK(ctx, hipMemcpy2DAsync(packed_out + r.win_row * host_pitch_words, (size_t)host_pitch_words * 4, stage,
                                        (size_t)sw * 4, (size_t)sw * 4, (size_t)r.count, hipMemcpyDeviceToHost,
                                        ctx->compute));
        stage += r.count * sw;
    }
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
    return GOL_OK;
}

int gol_write_region(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h, const uint32_t* packed,
                     int64_t host_pitch_words, int32_t mode) {
    if (int rc = check_window(ctx, "gol_write_region", x0, y0, w, h, packed, host_pitch_words)) return rc;
    if (mode != GOL_REGION_COPY && mode != GOL_REGION_OR && mode != GOL_REGION_XOR && mode != GOL_REGION_CLEAR)
        return set_err(ctx, GOL_EINVAL, "gol_write_region: unknown mode %d", mode);
    RowRun runs[2];
    const int nruns = owned_runs(ctx, y0, h, runs);
    if (nruns == 0) return GOL_OK;  // the window misses this shard
    if (int rc = bind(ctx)) return rc;
    const int64_t sw = (w + 31) / 32;
    int64_t owned = 0;
    for (int k = 0; k < nruns; ++k) owned += runs[k].count;
    if (int rc = ensure_stage(ctx, (size_t)(owned * sw))) return rc;
    // On the compute stream: after every queued pass and after the device
    // copy of a snapshot in flight (gol_snapshot_async copies the board there
    // first).  The epoch stays: neighbours pull this plane's edge rows again
    // at the start of the next pass, after this stream's work.
    uint32_t* stage = ctx->region_stage.dev;
    for (int k = 0; k < nruns; ++k) {
        const RowRun& r = runs[k];
        HIP_CHECK(ctx, hipMemcpy2DAsync(stage, (size_t)sw * 4, packed + r.win_row * host_pitch_words,
                                        (size_t)host_pitch_words * 4, (size_t)sw * 4, (size_t)r.count,
                                        hipMemcpyHostToDevice, ctx->compute));
        HIP_CHECK(ctx, gol::launch_region_scatter(ctx->plane[ctx->cur] + r.local_row * ctx->pitch, ctx->pitch,
                                                  ctx->wwords, ctx->width, ctx->ilv, (int32_t)r.count, x0, w, stage,
                                                  mode, ctx->topology == GOL_TORUS, ctx->compute));
        live_add(ctx, ctx->cur, r.local_row, r.local_row + r.count);  // no scan: place() then step() stays O(pattern)
        stage += r.count * sw;
    }
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
    return GOL_OK;
}

int gol_density(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h, int32_t log2_tile, uint32_t* counts,
                int64_t pitch) {
    if (int rc = check_window(ctx, "gol_density", x0, y0, w, h, counts)) return rc;
    if (log2_tile < 0 || log2_tile > 15)
        return set_err(ctx, GOL_EINVAL, "gol_density: log2_tile %d is not in 0 .. 15", log2_tile);
    const int lg = log2_tile;
    const int64_t tw = ((w - 1) >> lg) + 1;
    if (pitch < tw)
        return set_err(ctx, GOL_EINVAL, "gol_density: pitch %lld < %lld counts per map row", (long long)pitch,
                       (long long)tw);
    RowRun runs[2];
    const int nruns = owned_runs(ctx, y0, h, runs);
    if (nruns == 0) return GOL_OK;  // the window misses this shard
    if (int rc = bind(ctx)) return rc;
    // Each run counts into its own rows of the grid -- the tile rows its
    // window rows meet -- so two runs (or two shards) that share a tile row
    // each add their part of it to the caller's buffer.
    int64_t map_row[2], map_rows[2];
    size_t words = 0;
    for (int k = 0; k < nruns; ++k) {
        map_row[k] = runs[k].win_row >> lg;
        map_rows[k] = ((runs[k].win_row + runs[k].count - 1) >> lg) - map_row[k] + 1;
        words += (size_t)(map_rows[k] * tw);
    }
    if (int rc = ensure_density(ctx, words)) return rc;
    // the window's columns as board columns that do not wrap: [xa, xb), xa being window column koff
    const int64_t first = std::min(w, ctx->width - x0);
    const int64_t piece[2][3] = {{x0, x0 + first, 0}, {0, w - first, first}};
    // On the compute stream: after every queued pass and after the device
    // copy of a snapshot in flight; the board, the epoch and the hash stay.
    Accum<uint32_t>& acc = ctx->density;
    if (!acc.clean) HIP_CHECK(ctx, hipMemsetAsync(acc.dev, 0, acc.count * sizeof(uint32_t), ctx->compute));
    acc.clean = 0;  // in use until the export has left it zero
    uint32_t* grid = acc.dev;
    for (int k = 0; k < nruns; ++k) {
        const RowRun& r = runs[k];
        const uint32_t* src = ctx->plane[ctx->cur] + r.local_row * ctx->pitch;
        if (lg >= gol::kDensityCoarseLog2) {
            for (const auto& p : piece)
                if (p[0] < p[1])
                    HIP_CHECK(ctx, gol::launch_density_coarse(src, ctx->pitch, ctx->wwords, ctx->ilv, (int32_t)r.count,
                                                              r.win_row, p[0], p[1], p[2], lg, grid, tw, map_rows[k],
                                                              ctx->compute));
        } else {
            HIP_CHECK(ctx, gol::launch_density_fine(src, ctx->pitch, ctx->wwords, ctx->ilv, (int32_t)r.count, r.win_row,
                                                    x0, w, lg, grid, tw, map_rows[k], ctx->compute));
        }
        grid += map_rows[k] * tw;
    }
    HIP_CHECK(ctx, gol::launch_density_export(acc.dev, acc.host_dev, (int64_t)words, ctx->compute));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
    acc.clean = acc.count;
    const uint32_t* got = acc.host;
    for (int k = 0; k < nruns; ++k)
        for (int64_t i = 0; i < map_rows[k]; ++i, got += tw) {
            uint32_t* __restrict__ out = counts + (map_row[k] + i) * pitch;
            const uint32_t* __restrict__ in = got;
            for (int64_t j = 0; j < tw; ++j) out[j] += in[j];
        }
    return GOL_OK;
}

int gol_find(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h, const uint32_t* pattern, const uint32_t* care,
             int64_t pattern_pitch_words, int32_t pw, int32_t ph, int64_t* xy_out, int64_t max_matches,
             gol_find_result* out) {
    if (!ctx) return set_err(nullptr, GOL_EINVAL, "gol_find: null context");
    if (!pattern || !out) return set_err(ctx, GOL_EINVAL, "gol_find: null pattern or result");
    if (max_matches < 0 || (max_matches > 0 && !xy_out))
        return set_err(ctx, GOL_EINVAL, "gol_find: max_matches %lld %s", (long long)max_matches,
                       max_matches < 0 ? "is negative" : "with a null xy_out");
    if (pw < 1 || pw > 64 || ph < 1 || ph > 64 || pw > ctx->width || ph > ctx->height)
        return set_err(ctx, GOL_EINVAL, "gol_find: a %d x %d pattern is not within 1 .. 64 each way and a %lld x %lld board",
                       pw, ph, (long long)ctx->width, (long long)ctx->height);
    if (pattern_pitch_words < (pw + 31) / 32)
        return set_err(ctx, GOL_EINVAL, "gol_find: pattern pitch %lld < %d words per pattern row",
                       (long long)pattern_pitch_words, (pw + 31) / 32);
    if (int rc = check_window(ctx, "gol_find", x0, y0, w, h, pattern)) return rc;
    // the cared cells, live ones first, each group row by row: the kernel loads a pattern row when the
    // list reaches it
    std::vector<uint32_t> cells[2];  // [dead, live]
    for (int i = 0; i < ph; ++i)
        for (int k = 0; k < pw; ++k) {
            const int64_t word = i * pattern_pitch_words + k / 32;
            if (care && !((care[word] >> (k % 32)) & 1u)) continue;
            const bool alive = (pattern[word] >> (k % 32)) & 1u;
            cells[alive].push_back(gol::find_cell(i, k, alive));
        }
    const size_t ncells = cells[0].size() + cells[1].size();
    if (ncells == 0) return set_err(ctx, GOL_EINVAL, "gol_find: the care mask cares for no cell of the pattern");
    const bool has_live = !cells[1].empty();

    gol_find_result res{0, 0, 0};
    // The anchor rows this shard examines: the window's rows it owns whose pattern rows are all its own
    // (a whole torus wraps) or off the end of a clipped board.
    const bool wrap_y = ctx->topology == GOL_TORUS && ctx->rows == ctx->height;
    const bool open_end = wrap_y || (ctx->topology == GOL_REF_CLIPPED && ctx->row0 + ctx->rows == ctx->height);
    const int64_t a_end = open_end ? ctx->rows : ctx->rows - (ph - 1);  // anchors: local rows [0, a_end)
    RowRun runs[2];
    const int nruns = owned_runs(ctx, y0, h, runs);
    // ... of them, where the live rows are known and the pattern has a live cared cell, those with a
    // pattern row in a run
    const LiveRows& live = ctx->live[ctx->cur];
    const bool narrowed = live.known && has_live;
    const golactive::Runs can_match =
        narrowed ? golactive::anchor_rows(live.runs, ph, (int32_t)ctx->rows, wrap_y) : golactive::Runs{};
    golactive::Runs todo;
    for (int k = 0; k < nruns; ++k) {
        const int64_t lo = runs[k].local_row, hi = std::min(runs[k].local_row + runs[k].count, a_end);
        if (lo >= hi) continue;
        if (narrowed)
            for (const golactive::Run& r : golactive::clip(can_match, lo, hi)) todo.push_back(r);
        else
            todo.push_back({(int32_t)lo, (int32_t)hi});
    }
    res.rows_searched = (uint64_t)golactive::row_count(todo);
    if (todo.empty()) {  // the window misses the shard, or no row of it can hold a match
        *out = res;
        return GOL_OK;
    }
    if (int rc = bind(ctx)) return rc;
    if (int rc = ensure_find(ctx, ncells, (size_t)max_matches)) return rc;
    std::copy(cells[1].begin(), cells[1].end(), ctx->find_cells.host);
    std::copy(cells[0].begin(), cells[0].end(), ctx->find_cells.host + cells[1].size());
    // On the compute stream: after every queued pass and after the device copy of a snapshot in flight;
    // the board, the epoch, the hash and the live-row lists stay.
    Accum<unsigned long long>& acc = ctx->find_count;
    HIP_CHECK(ctx, hipMemcpyAsync(ctx->find_cells.dev, ctx->find_cells.host, ncells * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, ctx->compute));
    if (!acc.clean) HIP_CHECK(ctx, hipMemsetAsync(acc.dev, 0, gol::kFindWords * sizeof(unsigned long long), ctx->compute));
    acc.clean = 0;  // in use until the fold has left the counters zero
    gol::FindParams p{};
    p.plane = ctx->plane[ctx->cur];
    p.cells = ctx->find_cells.dev;
    p.slots = acc.dev;
    p.hits = max_matches ? ctx->find_hits.dev : nullptr;
    p.pitch = ctx->pitch;
    p.max_hits = max_matches;
    p.grow0 = ctx->row0;
    p.x0 = x0;
    p.width = ctx->width;
    p.wwords = ctx->wwords;
    p.rows = (int32_t)ctx->rows;
    p.sw = (int32_t)((w + 31) / 32);
    p.last_mask = w % 32 ? (uint32_t)((1ull << (w % 32)) - 1ull) : 0xFFFFFFFFu;
    p.c_first = (int32_t)(x0 / 32);
    p.sh = (int32_t)(x0 % 32);
    p.nw = ((p.sh + pw + 30) >> 5) + 1;  // anchor bit 31's column pw - 1 is bit sh + 31 + pw - 1 of the lane's words
    p.ncells = (int32_t)ncells;
    p.prefilter = has_live && gol::find_prefilter_fits(ctx->topology == GOL_TORUS, ctx->wwords);
    p.wrap_x = ctx->topology == GOL_TORUS;
    p.wrap_y = wrap_y;
    for (const golactive::Run& r : todo) {
        p.a_lo = r.lo;
        p.a_hi = r.hi;
        HIP_CHECK(ctx, gol::launch_find(p, ctx->ilv, ctx->compute));
    }
    HIP_CHECK(ctx, gol::launch_find_fold(acc.dev, acc.host_dev, ctx->compute));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
    acc.clean = 1;
    res.count = acc.host[0];
    res.returned = std::min<uint64_t>(res.count, (uint64_t)max_matches);
    if (res.returned) {
        HIP_CHECK(ctx, hipMemcpyAsync(xy_out, ctx->find_hits.dev, (size_t)res.returned * 2 * sizeof(int64_t),
                                      hipMemcpyDeviceToHost, ctx->compute));
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->compute));
        std::vector<std::pair<int64_t, int64_t>> yx((size_t)res.returned);  // the host sorts: by (y, x)
        for (size_t k = 0; k < yx.size(); ++k) yx[k] = {xy_out[2 * k + 1], xy_out[2 * k]};
        std::sort(yx.begin(), yx.end());
        for (size_t k = 0; k < yx.size(); ++k) xy_out[2 * k] = yx[k].second, xy_out[2 * k + 1] = yx[k].first;
    }
    *out = res;
    return GOL_OK;
}

}  // extern "C"
