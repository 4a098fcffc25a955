// gol_region.cpp -- the board from the user's side without moving a plane:
// gol_census (population and bounding box, one pass on the device),
// gol_read_region and gol_write_region (a window of the torus or of the
// clipped board, gathered from / scattered into the device layout) and
// gol_density (the live cells per tile of a window: the zoomed-out view).  They
// stand for what the reference offered at 7 x 7: the per-cell initialState of
// BoardCreator.scala:65-70, the CellStateMsg stream a LoggerActor prints
// (CellActor.scala:89, LoggerActor.scala:30-46) and the counting a reader of
// that log does by eye.
#include <algorithm>
#include <cstring>

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

}  // extern "C"
