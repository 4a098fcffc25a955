// gol_batch.cpp -- C ABI of the batch engine (include/gol.h gol_batch_*,
// gol_cycle_*, gol_find_batch*, gol_objects_batch*, gol_census_batch* and
// gol_rules_batch_*; DESIGN.md sections 5f to 5k): many independent boards of at most 64 x 64
// stored cells stepped by one launch (kernels: gol_batch.hip), searched by one
// (gol_batch_find.hip), cut into their objects by one (gol_batch_objects.hip)
// and those tallied by one (gol_batch_census.hip).  A
// handle type of its own: it shares the error conventions and the HIP status
// discipline with the contexts (gol_ctx.h), and nothing else -- no planner, no
// step kernel.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "gol_batch.h"
#include "gol_ctx.h"

struct gol_batch {
    golbatch::Geometry geo{};
    golbatch::Lanes lanes{};
    uint32_t birth = 0, survive = 0;
    int device = 0;
    uint32_t chunk = 0;  // gol_batch_set_chunk (0: automatic)
    uint64_t epoch = 0;
    hipStream_t stream = nullptr;
    unsigned long long* plane = nullptr;  // boards * height rows
    // the plane one generation before (settle detection across launches), or a cycle call's snapshot plane: a call
    // is one or the other, and neither reads what an earlier call left in it
    unsigned long long* prev = nullptr;
    uint32_t* settled = nullptr;          // [boards]
    // gol_cycle_step's words, allocated by its first call: period [boards], seen [boards], then the two counters
    // (boards that have a period, the largest period)
    uint32_t* cycle_words = nullptr;
    uint64_t cycle_launches = 0, cycle_boards = 0;  // gol_cycle_stats: the last gol_cycle_step call
    uint32_t cycle_max_period = 0;
    // the series of one launch, [boards][series_gens] (grown on demand), and gol_batch_hashes' results
    uint32_t* series = nullptr;
    size_t series_gens = 0;
    unsigned long long* hashes = nullptr;
    uint32_t* hash_pops = nullptr;
    size_t hashes_count = 0;
    // gol_find_batch's buffers, grown on demand: the pattern table (headers, then the row pairs), the counts
    // [boards][npatterns] and the match planes [npatterns][boards][height]
    void* find_table = nullptr;
    size_t find_table_bytes = 0;
    uint32_t* find_counts = nullptr;
    size_t find_counts_n = 0;
    unsigned long long* find_matches = nullptr;
    size_t find_matches_n = 0;
    uint32_t find_cut = 0;  // gol_find_batch_set_cut (0: automatic)
    uint64_t find_launches = 0, find_cared = 0;  // gol_find_batch_stats: the last gol_find_batch call
    // gol_objects_batch's buffers, grown on demand: the counts [count] and the records [count][max_objects]
    uint32_t* obj_counts = nullptr;
    size_t obj_counts_n = 0;
    gol_batch_object* obj_records = nullptr;
    size_t obj_records_n = 0;
    // gol_objects_batch_stats: the last gol_objects_batch call
    uint64_t obj_launches = 0, obj_total = 0, obj_truncated = 0;
    // gol_census_batch_*'s table (census_capacity slots, 0: no census has begun) and counters, the calls since
    // begin, and the buffers, grown on demand, add_records' records and read's entries pass through
    unsigned long long* census_slots = nullptr;
    unsigned long long* census_counters = nullptr;
    uint32_t census_capacity = 0;
    uint64_t census_calls = 0;
    gol_batch_object* census_in = nullptr;
    size_t census_in_n = 0;
    gol_census_entry* census_out = nullptr;
    size_t census_out_n = 0;
    // gol_rules_batch_*: the device's rule words [boards], allocated by the first set; their host copy, the rules
    // in force (empty before the first set: the configuration's rule everywhere); and whether the steps launch the
    // RULES instances
    uint32_t* rules = nullptr;
    std::vector<uint32_t> rules_host;
    bool rules_on = false;
    std::string err;
};

namespace {

using golc::hip_note;

int batch_err(gol_batch* b, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (b) {
        b->err = buf;
        return code;
    }
    return golc::set_err(nullptr, code, "%s", buf);
}

// A failing HIP call's status is reported through the return code and taken
// off the thread.
int batch_hip_fail(gol_batch* b, hipError_t e, const char* expr, int line) {
    (void)hipGetLastError();
    return batch_err(b, GOL_EHIP, "%s failed: %s (gol_batch.cpp:%d)", expr, hipGetErrorString(e), line);
}

#define BATCH_HIP(b, expr)                                                        \
    do {                                                                          \
        const hipError_t e_ = (expr);                                             \
        if (e_ != hipSuccess) return batch_hip_fail((b), e_, #expr, __LINE__);    \
    } while (0)

bool life_rule(const gol_batch* b) {
    return b->birth == GOL_RULE_LIFE_BIRTH && b->survive == GOL_RULE_LIFE_SURVIVE;
}

size_t plane_words(const gol_batch* b) { return (size_t)b->geo.boards * (size_t)b->geo.height; }

// boards [first, first + count) inside the batch
bool window_ok(const gol_batch* b, int64_t first, int64_t count) {
    return first >= 0 && count >= 1 && first < b->geo.boards && count <= (int64_t)b->geo.boards - first;
}

void destroy_impl(gol_batch* b) {
    hip_note(hipSetDevice(b->device), "batch destroy: hipSetDevice");
    if (b->stream) hip_note(hipStreamSynchronize(b->stream), "batch destroy: hipStreamSynchronize");
    for (void* p : {(void*)b->plane, (void*)b->prev, (void*)b->settled, (void*)b->series, (void*)b->hashes,
                    (void*)b->hash_pops, (void*)b->cycle_words, b->find_table, (void*)b->find_counts,
                    (void*)b->find_matches, (void*)b->obj_counts, (void*)b->obj_records, (void*)b->census_slots,
                    (void*)b->census_counters, (void*)b->census_in, (void*)b->census_out, (void*)b->rules})
        if (p) hip_note(hipFree(p), "batch destroy: hipFree");
    if (b->stream) hip_note(hipStreamDestroy(b->stream), "batch destroy: hipStreamDestroy");
    delete b;
}

// A buffer of the handle that holds at least `want` elements of `elem` bytes (nothing is in flight on the old one:
// every call synchronises).  False, with the buffer gone, if it cannot be had.
template <class T>
bool grow(T*& buf, size_t& have, size_t want, size_t elem) {
    if (have >= want) return true;
    if (buf) hip_note(hipFree(buf), "gol_find_batch: hipFree");
    buf = nullptr;
    have = 0;
    void* p = nullptr;
    if (hipMalloc(&p, want * elem) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    buf = static_cast<T*>(p);
    have = want;
    return true;
}

// "pattern 3: ..." or "...": batch_find_patterns' refusal as a message
int find_refusal(gol_batch* b, const char* fn, const char* why, int32_t which) {
    if (which >= 0) return batch_err(b, GOL_EINVAL, "%s: pattern %d: %s", fn, which, why);
    return batch_err(b, GOL_EINVAL, "%s: %s", fn, why);
}

// The objects launch of every board into the handle's buffers, as gol_objects_batch issues it (no copy back, no
// synchronisation).  GOL_ENOMEM if the buffers cannot be had.
int launch_objects(gol_batch* batch, const char* fn, int64_t first, int64_t count, int32_t reach,
                   int32_t max_objects) {
    const size_t n = (size_t)count, records_n = n * (size_t)max_objects;  // <= 2^22 * 2^10
    if (!grow(batch->obj_counts, batch->obj_counts_n, n, sizeof(uint32_t)) ||
        !grow(batch->obj_records, batch->obj_records_n, records_n, sizeof(gol_batch_object)))
        return batch_err(batch, GOL_ENOMEM, "%s: hipMalloc of the counts (%zu entries) or the records "
                         "(%zu entries) failed; nothing written", fn, n, records_n);
    // the records past a board's count are zero: one memset before the launch, the kernel stores the real ones only
    BATCH_HIP(batch, hipMemsetAsync(batch->obj_records, 0, records_n * sizeof(gol_batch_object), batch->stream));
    golbatch::ObjectsParams p{};
    p.plane = batch->plane;
    p.counts = batch->obj_counts;
    p.objects = reinterpret_cast<uint4*>(batch->obj_records);
    p.boards = (int32_t)(first + count);
    p.width = batch->geo.width;
    p.height = batch->geo.height;
    p.boards_per_wave = batch->lanes.boards_per_wave;
    p.vis_w = batch->geo.vis_w;
    p.vis_h = batch->geo.vis_h;
    p.first = (int32_t)first;
    p.reach = reach;
    p.max_objects = max_objects;
    BATCH_HIP(batch, golbatch::launch_batch_objects(p, batch->geo.clipped, batch->stream));
    return GOL_OK;
}

// batch_rules_args' refusal as a message: "rules[5] (board 7) = 0x...: ..." or the range
int rules_refusal(gol_batch* b, const char* fn, const char* why, const golbatch::Geometry& g, int64_t first,
                  int64_t count, const uint32_t* rules, int64_t which) {
    if (which >= 0)
        return batch_err(b, GOL_EINVAL, "%s: rules[%lld] (board %lld) = 0x%08X: %s", fn, (long long)which,
                         (long long)(first + which), rules[which], why);
    return batch_err(b, GOL_EINVAL, "%s: %s (first %lld, count %lld, batch of %d)", fn, why, (long long)first,
                     (long long)count, g.boards);
}

golbatch::CensusTable census_table(const gol_batch* b) {
    return {b->census_slots, b->census_counters, b->census_capacity};
}

// batch_census_args for a call of this handle: the request's handle fields filled in
const char* census_refusal(const gol_batch* b, golbatch::CensusRequest r) {
    r.begun = b->census_capacity != 0;
    r.next_call = b->census_calls;
    return golbatch::batch_census_args(b->geo, r);
}

}  // namespace

extern "C" {

int gol_batch_geometry_get(const gol_batch_config* cfg, gol_batch_geometry* out) {
    if (!cfg || !out) return batch_err(nullptr, GOL_EINVAL, "gol_batch_geometry_get: null argument");
    golbatch::Geometry g;
    if (const char* why = golbatch::batch_geometry(*cfg, &g))
        return batch_err(nullptr, GOL_EINVAL, "batch of %d boards %d x %d: %s", cfg->boards, cfg->width, cfg->height,
                         why);
    const golbatch::Lanes l = golbatch::batch_lanes(g.height, g.boards);
    out->boards_per_wave = l.boards_per_wave;
    out->waves = l.waves;
    out->device_bytes = golbatch::batch_device_bytes(g);
    return GOL_OK;
}

int gol_batch_create(gol_batch** out, const gol_batch_config* cfg) {
    if (!out || !cfg) return batch_err(nullptr, GOL_EINVAL, "gol_batch_create: null argument");
    *out = nullptr;
    golbatch::Geometry g;
    if (const char* why = golbatch::batch_geometry(*cfg, &g))
        return batch_err(nullptr, GOL_EINVAL, "batch of %d boards %d x %d: %s", cfg->boards, cfg->width, cfg->height,
                         why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return batch_err(nullptr, GOL_ENODEV, "no HIP device available (libgol has no CPU fallback)");
    }
    if (cfg->device < 0 || cfg->device >= ndev)
        return batch_err(nullptr, GOL_EINVAL, "device %d out of range (%d devices)", cfg->device, ndev);

    gol_batch* b = new gol_batch();
    b->geo = g;
    b->lanes = golbatch::batch_lanes(g.height, g.boards);
    b->birth = cfg->birth_mask;
    b->survive = cfg->survive_mask;
    b->device = cfg->device;
    auto fail = [&](int rc, const char* what) {
        (void)hipGetLastError();  // the failed call's status: reported through rc
        destroy_impl(b);
        return batch_err(nullptr, rc, "gol_batch_create: %s failed", what);
    };
    if (hipSetDevice(b->device) != hipSuccess) return fail(GOL_EHIP, "hipSetDevice");
    const size_t bytes = plane_words(b) * sizeof(unsigned long long);
    const size_t settle_bytes = (size_t)g.boards * sizeof(uint32_t);
    if (hipMalloc(&b->plane, bytes) != hipSuccess || hipMalloc(&b->prev, bytes) != hipSuccess ||
        hipMalloc(&b->settled, settle_bytes) != hipSuccess)
        return fail(GOL_ENOMEM, "hipMalloc of the planes");
    if (hipMemset(b->plane, 0, bytes) != hipSuccess || hipMemset(b->prev, 0, bytes) != hipSuccess ||
        hipMemset(b->settled, 0, settle_bytes) != hipSuccess)
        return fail(GOL_EHIP, "hipMemset");
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess)
        return fail(GOL_EHIP, "hipStreamCreateWithFlags");
    if (hipDeviceSynchronize() != hipSuccess) return fail(GOL_EHIP, "hipDeviceSynchronize");
    *out = b;
    return GOL_OK;
}

void gol_batch_destroy(gol_batch* batch) {
    if (batch) destroy_impl(batch);
}

const char* gol_batch_last_error(const gol_batch* batch) {
    return batch ? batch->err.c_str() : gol_last_error(nullptr);
}

int gol_batch_seed(gol_batch* batch, uint64_t seed) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_seed: null handle");
    BATCH_HIP(batch, hipSetDevice(batch->device));
    BATCH_HIP(batch, golbatch::launch_batch_seed(batch->plane, (int64_t)plane_words(batch), batch->geo.width, seed,
                                                 batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->epoch = 0;
    return GOL_OK;
}

int gol_batch_load(gol_batch* batch, int64_t first, int64_t count, const uint64_t* rows) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_load: null handle");
    if (!rows) return batch_err(batch, GOL_EINVAL, "gol_batch_load: rows is null");
    if (!window_ok(batch, first, count))
        return batch_err(batch, GOL_EINVAL, "gol_batch_load: boards [%lld, %lld + %lld) outside the batch of %d",
                         (long long)first, (long long)first, (long long)count, batch->geo.boards);
    const size_t H = (size_t)batch->geo.height, n = (size_t)count * H;
    const uint64_t wmask = batch->geo.width >= 64 ? ~0ull : (1ull << batch->geo.width) - 1ull;
    std::vector<uint64_t> masked(n);  // bits at x >= width are ignored
    for (size_t i = 0; i < n; ++i) masked[i] = rows[i] & wmask;
    BATCH_HIP(batch, hipSetDevice(batch->device));
    BATCH_HIP(batch, hipMemcpyAsync(batch->plane + (size_t)first * H, masked.data(), n * sizeof(uint64_t),
                                    hipMemcpyHostToDevice, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->epoch = 0;
    return GOL_OK;
}

int gol_batch_snapshot(gol_batch* batch, int64_t first, int64_t count, uint64_t* rows) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_snapshot: null handle");
    if (!rows) return batch_err(batch, GOL_EINVAL, "gol_batch_snapshot: rows is null");
    if (!window_ok(batch, first, count))
        return batch_err(batch, GOL_EINVAL, "gol_batch_snapshot: boards [%lld, %lld + %lld) outside the batch of %d",
                         (long long)first, (long long)first, (long long)count, batch->geo.boards);
    const size_t H = (size_t)batch->geo.height;
    BATCH_HIP(batch, hipSetDevice(batch->device));
    // the plane never holds a bit at x >= width: every writer masks
    BATCH_HIP(batch, hipMemcpyAsync(rows, batch->plane + (size_t)first * H, (size_t)count * H * sizeof(uint64_t),
                                    hipMemcpyDeviceToHost, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_batch_step(gol_batch* batch, uint32_t generations, uint32_t* populations_out, size_t capacity,
                   uint32_t* settled_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_step: null handle");
    const size_t boards = (size_t)batch->geo.boards;
    if (populations_out && capacity / boards < generations)  // boards * generations may pass 2^32: compare by division
        return batch_err(batch, GOL_EINVAL, "gol_batch_step: populations_out holds %zu entries, %zu boards x %u "
                         "generations need %zu", capacity, boards, generations, boards * (size_t)generations);
    if (generations == 0) return GOL_OK;
    const uint32_t chunk = std::min(batch->chunk ? batch->chunk : golbatch::kAutoChunk, generations);
    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (populations_out && batch->series_gens < chunk) {
        // nothing is in flight on the old buffer: every call synchronises
        if (batch->series) BATCH_HIP(batch, hipFree(batch->series));
        batch->series = nullptr;
        batch->series_gens = 0;
        const size_t bytes = boards * (size_t)chunk * sizeof(uint32_t);
        if (hipMalloc(&batch->series, bytes) != hipSuccess) {
            (void)hipGetLastError();
            batch->series = nullptr;
            return batch_err(batch, GOL_ENOMEM, "gol_batch_step: hipMalloc of %zu bytes for the population series "
                             "failed; nothing advanced", bytes);
        }
        batch->series_gens = chunk;
    }
    golbatch::StepParams p{};
    p.plane = batch->plane;
    p.prev = batch->prev;
    p.pops = populations_out ? batch->series : nullptr;
    p.settled = settled_out ? batch->settled : nullptr;
    p.boards = batch->geo.boards;
    p.width = batch->geo.width;
    p.height = batch->geo.height;
    p.boards_per_wave = batch->lanes.boards_per_wave;
    p.vis_w = batch->geo.vis_w;
    p.vis_h = batch->geo.vis_h;
    p.pop_stride = (uint32_t)batch->series_gens;
    p.birth = batch->birth;
    p.survive = batch->survive;
    p.rules = batch->rules_on ? batch->rules : nullptr;
    for (uint32_t g0 = 0; g0 < generations; g0 += chunk) {
        p.gens = std::min(chunk, generations - g0);
        p.g0 = g0;
        BATCH_HIP(batch, golbatch::launch_batch_step(p, life_rule(batch), batch->geo.clipped, batch->rules_on,
                                                     batch->stream));
        batch->epoch += p.gens;
        if (populations_out)  // this launch's columns of the caller's [boards][generations]; waits for the launch
            BATCH_HIP(batch, hipMemcpy2DAsync(populations_out + g0, (size_t)generations * sizeof(uint32_t), batch->series,
                                              batch->series_gens * sizeof(uint32_t), (size_t)p.gens * sizeof(uint32_t),
                                              boards, hipMemcpyDeviceToHost, batch->stream));
    }
    if (settled_out)
        BATCH_HIP(batch, hipMemcpyAsync(settled_out, batch->settled, boards * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                        batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_cycle_snapshot_generation(uint32_t generation, uint32_t* snapshot_out) {
    if (generation == 0 || !snapshot_out)
        return batch_err(nullptr, GOL_EINVAL, "gol_cycle_snapshot_generation: generation 0 is compared with nothing, "
                         "and snapshot_out must not be null");
    *snapshot_out = golbatch::cycle_snapshot_generation(generation);
    return GOL_OK;
}

int gol_cycle_step(gol_batch* batch, uint32_t generations, uint32_t* period_out, uint32_t* seen_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_cycle_step: null handle");
    if (generations == 0) return GOL_OK;
    const size_t boards = (size_t)batch->geo.boards;
    const uint32_t chunk = batch->chunk ? batch->chunk : golbatch::kAutoChunk;
    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (!batch->cycle_words) {
        const size_t bytes = (2 * boards + 2) * sizeof(uint32_t);
        if (hipMalloc(&batch->cycle_words, bytes) != hipSuccess) {
            (void)hipGetLastError();
            batch->cycle_words = nullptr;
            return batch_err(batch, GOL_ENOMEM, "gol_cycle_step: hipMalloc of %zu bytes for the period and seen words "
                             "failed; nothing advanced", bytes);
        }
    }
    golbatch::CycleParams p{};
    p.plane = batch->plane;
    p.snap = batch->prev;
    p.period = batch->cycle_words;
    p.seen = batch->cycle_words + boards;
    p.counters = batch->cycle_words + 2 * boards;
    p.boards = batch->geo.boards;
    p.width = batch->geo.width;
    p.height = batch->geo.height;
    p.boards_per_wave = batch->lanes.boards_per_wave;
    p.vis_w = batch->geo.vis_w;
    p.vis_h = batch->geo.vis_h;
    p.birth = batch->birth;
    p.survive = batch->survive;
    p.rules = batch->rules_on ? batch->rules : nullptr;
    // the first launch of a call reads neither the words nor the snapshot plane; the counters start at zero
    BATCH_HIP(batch, hipMemsetAsync(p.counters, 0, 2 * sizeof(uint32_t), batch->stream));
    batch->cycle_launches = 0;
    uint32_t counters[2] = {0u, 0u};
    for (uint32_t g0 = 0; g0 < generations; g0 += p.gens) {
        // every board cycled: a launch fast-forwards, at most max_period - 1 generations per board whatever it is
        // asked for, so the remainder goes as one launch unless a chunk launch is the shorter
        const bool all = counters[0] == boards && counters[1] - 1u <= chunk;
        p.gens = all ? generations - g0 : std::min(chunk, generations - g0);
        p.g0 = g0;
        BATCH_HIP(batch, golbatch::launch_batch_cycle(p, life_rule(batch), batch->geo.clipped, batch->rules_on,
                                                      batch->stream));
        batch->epoch += p.gens;
        ++batch->cycle_launches;
        BATCH_HIP(batch, hipMemcpyAsync(counters, p.counters, sizeof counters, hipMemcpyDeviceToHost, batch->stream));
        BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
        batch->cycle_boards = counters[0];
        batch->cycle_max_period = counters[1];
    }
    if (period_out)
        BATCH_HIP(batch, hipMemcpyAsync(period_out, p.period, boards * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                        batch->stream));
    if (seen_out)
        BATCH_HIP(batch, hipMemcpyAsync(seen_out, p.seen, boards * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                        batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_cycle_stats(gol_batch* batch, uint64_t* launches, uint64_t* boards_cycled, uint32_t* max_period) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_cycle_stats: null handle");
    if (launches) *launches = batch->cycle_launches;
    if (boards_cycled) *boards_cycled = batch->cycle_boards;
    if (max_period) *max_period = batch->cycle_max_period;
    return GOL_OK;
}

int gol_batch_hashes(gol_batch* batch, int64_t first, int64_t count, uint64_t* hashes_out,
                     uint32_t* populations_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_hashes: null handle");
    if (!hashes_out && !populations_out) return batch_err(batch, GOL_EINVAL, "gol_batch_hashes: both arrays are null");
    if (!window_ok(batch, first, count))
        return batch_err(batch, GOL_EINVAL, "gol_batch_hashes: boards [%lld, %lld + %lld) outside the batch of %d",
                         (long long)first, (long long)first, (long long)count, batch->geo.boards);
    BATCH_HIP(batch, hipSetDevice(batch->device));
    const size_t n = (size_t)count;
    if (batch->hashes_count < n) {
        if (batch->hashes) BATCH_HIP(batch, hipFree(batch->hashes));
        batch->hashes = nullptr;
        if (batch->hash_pops) BATCH_HIP(batch, hipFree(batch->hash_pops));
        batch->hash_pops = nullptr;
        batch->hashes_count = 0;
        if (hipMalloc(&batch->hashes, n * sizeof(unsigned long long)) != hipSuccess ||
            hipMalloc(&batch->hash_pops, n * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            if (batch->hashes) hip_note(hipFree(batch->hashes), "gol_batch_hashes: hipFree");
            batch->hashes = nullptr;
            batch->hash_pops = nullptr;
            return batch_err(batch, GOL_ENOMEM, "gol_batch_hashes: hipMalloc for %zu boards failed", n);
        }
        batch->hashes_count = n;
    }
    BATCH_HIP(batch, golbatch::launch_batch_hashes(batch->plane, batch->geo.height, first, count,
                                                   hashes_out ? batch->hashes : nullptr,
                                                   populations_out ? batch->hash_pops : nullptr, batch->stream));
    if (hashes_out)
        BATCH_HIP(batch, hipMemcpyAsync(hashes_out, batch->hashes, n * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                        batch->stream));
    if (populations_out)
        BATCH_HIP(batch, hipMemcpyAsync(populations_out, batch->hash_pops, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                        batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_find_batch_check(const gol_batch_config* cfg, const gol_batch_pattern* patterns, int32_t npatterns) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_find_batch_check: null configuration");
    golbatch::Geometry g;
    if (const char* why = golbatch::batch_geometry(*cfg, &g))
        return batch_err(nullptr, GOL_EINVAL, "batch of %d boards %d x %d: %s", cfg->boards, cfg->width, cfg->height,
                         why);
    int32_t which = -1;
    if (const char* why = golbatch::batch_find_patterns(g, patterns, npatterns, &which))
        return find_refusal(nullptr, "gol_find_batch_check", why, which);
    return GOL_OK;
}

int gol_find_batch(gol_batch* batch, const gol_batch_pattern* patterns, int32_t npatterns, uint32_t* counts_out,
                   size_t counts_capacity, uint64_t* matches_out, size_t matches_capacity) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_find_batch: null handle");
    int32_t which = -1;
    if (const char* why = golbatch::batch_find_patterns(batch->geo, patterns, npatterns, &which))
        return find_refusal(batch, "gol_find_batch", why, which);
    if (!counts_out) return batch_err(batch, GOL_EINVAL, "gol_find_batch: counts_out is null");
    const size_t boards = (size_t)batch->geo.boards, H = (size_t)batch->geo.height, np = (size_t)npatterns;
    const size_t counts_n = boards * np, matches_n = np * boards * H;  // <= 2^8 * 2^22 * 2^6
    if (counts_capacity < counts_n)
        return batch_err(batch, GOL_EINVAL, "gol_find_batch: counts_out holds %zu entries, %zu boards x %d patterns "
                         "need %zu", counts_capacity, boards, npatterns, counts_n);
    if (matches_out && matches_capacity < matches_n)
        return batch_err(batch, GOL_EINVAL, "gol_find_batch: matches_out holds %zu entries, %d patterns x %zu boards "
                         "x %zu rows need %zu", matches_capacity, npatterns, boards, H, matches_n);

    // the table: the headers, then per pattern row the pair (cells & care, care), bits at k >= pw cleared
    size_t nrows = 0;
    for (int32_t p = 0; p < npatterns; ++p) nrows += (size_t)patterns[p].ph;
    const size_t head_bytes = np * sizeof(golbatch::FindPattern);  // a multiple of 16: the rows stay 8-byte aligned
    const size_t table_bytes = head_bytes + nrows * 2 * sizeof(uint64_t);
    std::vector<unsigned char> table(table_bytes);
    auto* heads = reinterpret_cast<golbatch::FindPattern*>(table.data());
    auto* rows = reinterpret_cast<uint64_t*>(table.data() + head_bytes);
    uint32_t row0 = 0;
    uint64_t cared_all = 0;
    for (int32_t p = 0; p < npatterns; ++p) {
        const gol_batch_pattern& q = patterns[p];
        const uint64_t kmask = q.pw >= 64 ? ~0ull : (1ull << q.pw) - 1ull;
        uint32_t cared = 0;
        for (int32_t i = 0; i < q.ph; ++i) {
            const uint64_t care = (q.care ? q.care[i] : ~0ull) & kmask;
            rows[2 * ((size_t)row0 + (size_t)i)] = q.cells[i] & care;
            rows[2 * ((size_t)row0 + (size_t)i) + 1] = care;
            cared += (uint32_t)__builtin_popcountll(care);
        }
        heads[p] = {q.pw, q.ph, row0, cared};
        row0 += (uint32_t)q.ph;
        cared_all += cared;
    }

    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (!grow(batch->find_table, batch->find_table_bytes, table_bytes, 1) ||
        !grow(batch->find_counts, batch->find_counts_n, counts_n, sizeof(uint32_t)) ||
        (matches_out && !grow(batch->find_matches, batch->find_matches_n, matches_n, sizeof(unsigned long long))))
        return batch_err(batch, GOL_ENOMEM, "gol_find_batch: hipMalloc of the pattern table (%zu bytes), the counts "
                         "(%zu entries) or the match planes (%zu entries) failed; nothing written", table_bytes,
                         counts_n, matches_out ? matches_n : (size_t)0);
    // `table` outlives the copy: the call synchronises before it returns
    BATCH_HIP(batch, hipMemcpyAsync(batch->find_table, table.data(), table_bytes, hipMemcpyHostToDevice, batch->stream));
    golbatch::FindParams fp{};
    fp.plane = batch->plane;
    fp.counts = batch->find_counts;
    fp.matches = matches_out ? batch->find_matches : nullptr;
    fp.boards = batch->geo.boards;
    fp.width = batch->geo.width;
    fp.height = batch->geo.height;
    fp.boards_per_wave = batch->lanes.boards_per_wave;
    fp.npatterns = npatterns;
    const auto* dev_heads = static_cast<const golbatch::FindPattern*>(batch->find_table);
    const auto* dev_rows = reinterpret_cast<const unsigned long long*>(
        static_cast<const unsigned char*>(batch->find_table) + head_bytes);
    // the cut: as many patterns per launch as stay within the bound, one at least
    const uint64_t cut = batch->find_cut ? batch->find_cut : golbatch::kAutoFindCut;
    batch->find_launches = 0;
    batch->find_cared = cared_all;
    for (int32_t first = 0; first < npatterns; first += fp.count) {
        uint64_t cared = heads[first].cared;
        int32_t n = 1;
        while (first + n < npatterns && cared + heads[first + n].cared <= cut) cared += heads[first + n++].cared;
        fp.first = first;
        fp.count = n;
        BATCH_HIP(batch, golbatch::launch_batch_find(fp, dev_heads, dev_rows, batch->geo.clipped, batch->stream));
        ++batch->find_launches;
    }
    BATCH_HIP(batch, hipMemcpyAsync(counts_out, batch->find_counts, counts_n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                    batch->stream));
    if (matches_out)
        BATCH_HIP(batch, hipMemcpyAsync(matches_out, batch->find_matches, matches_n * sizeof(uint64_t),
                                        hipMemcpyDeviceToHost, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_find_batch_set_cut(gol_batch* batch, uint32_t cared_cells_per_launch) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_find_batch_set_cut: null handle");
    batch->find_cut = cared_cells_per_launch;
    return GOL_OK;
}

int gol_find_batch_stats(gol_batch* batch, uint64_t* launches, uint64_t* cared_cells) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_find_batch_stats: null handle");
    if (launches) *launches = batch->find_launches;
    if (cared_cells) *cared_cells = batch->find_cared;
    return GOL_OK;
}

int gol_objects_batch_check(const gol_batch_config* cfg, int64_t first, int64_t count, int32_t reach,
                            int32_t max_objects) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_objects_batch_check: null configuration");
    golbatch::Geometry g;
    if (const char* why = golbatch::batch_geometry(*cfg, &g))
        return batch_err(nullptr, GOL_EINVAL, "batch of %d boards %d x %d: %s", cfg->boards, cfg->width, cfg->height,
                         why);
    if (const char* why = golbatch::batch_objects_args(g, first, count, reach, max_objects))
        return batch_err(nullptr, GOL_EINVAL, "gol_objects_batch_check: %s (first %lld, count %lld, reach %d, "
                         "max_objects %d, batch of %d)", why, (long long)first, (long long)count, reach, max_objects,
                         g.boards);
    return GOL_OK;
}

int gol_objects_batch(gol_batch* batch, int64_t first, int64_t count, int32_t reach, int32_t max_objects,
                      uint32_t* counts_out, size_t counts_capacity, gol_batch_object* objects_out,
                      size_t objects_capacity) {
    static_assert(sizeof(gol_batch_object) == sizeof(uint4), "a record is one 16-byte store");
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_objects_batch: null handle");
    if (const char* why = golbatch::batch_objects_args(batch->geo, first, count, reach, max_objects))
        return batch_err(batch, GOL_EINVAL, "gol_objects_batch: %s (first %lld, count %lld, reach %d, max_objects %d, "
                         "batch of %d)", why, (long long)first, (long long)count, reach, max_objects,
                         batch->geo.boards);
    if (!counts_out || !objects_out)
        return batch_err(batch, GOL_EINVAL, "gol_objects_batch: counts_out or objects_out is null");
    const size_t n = (size_t)count, records_n = n * (size_t)max_objects;  // <= 2^22 * 2^10
    if (counts_capacity < n)
        return batch_err(batch, GOL_EINVAL, "gol_objects_batch: counts_out holds %zu entries, %zu boards need %zu",
                         counts_capacity, n, n);
    if (objects_capacity < records_n)
        return batch_err(batch, GOL_EINVAL, "gol_objects_batch: objects_out holds %zu entries, %zu boards x %d "
                         "objects need %zu", objects_capacity, n, max_objects, records_n);

    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (const int rc = launch_objects(batch, "gol_objects_batch", first, count, reach, max_objects)) return rc;
    BATCH_HIP(batch, hipMemcpyAsync(counts_out, batch->obj_counts, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                    batch->stream));
    BATCH_HIP(batch, hipMemcpyAsync(objects_out, batch->obj_records, records_n * sizeof(gol_batch_object),
                                    hipMemcpyDeviceToHost, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->obj_launches = 1;
    batch->obj_total = batch->obj_truncated = 0;
    for (size_t i = 0; i < n; ++i) {
        batch->obj_total += counts_out[i];
        batch->obj_truncated += counts_out[i] > (uint32_t)max_objects ? 1u : 0u;
    }
    return GOL_OK;
}

int gol_objects_batch_stats(gol_batch* batch, uint64_t* launches, uint64_t* objects, uint64_t* boards_truncated) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_objects_batch_stats: null handle");
    if (launches) *launches = batch->obj_launches;
    if (objects) *objects = batch->obj_total;
    if (boards_truncated) *boards_truncated = batch->obj_truncated;
    return GOL_OK;
}

int gol_census_batch_check(const gol_batch_config* cfg, int32_t reach, int32_t max_objects, int64_t max_keys) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_check: null configuration");
    golbatch::Geometry g;
    if (const char* why = golbatch::batch_geometry(*cfg, &g))
        return batch_err(nullptr, GOL_EINVAL, "batch of %d boards %d x %d: %s", cfg->boards, cfg->width, cfg->height,
                         why);
    golbatch::CensusRequest r{};
    r.call = golbatch::CensusRequest::kCheck;
    r.reach = reach;
    r.max_objects = max_objects;
    r.max_keys = max_keys;
    if (const char* why = golbatch::batch_census_args(g, r))
        return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_check: %s (reach %d, max_objects %d, max_keys %lld)",
                         why, reach, max_objects, (long long)max_keys);
    return GOL_OK;
}

int gol_census_batch_begin(gol_batch* batch, int64_t max_keys) {
    static_assert(sizeof(gol_census_entry) == 2 * sizeof(uint4), "an entry is two 16-byte stores, and a slot's size");
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_begin: null handle");
    golbatch::CensusRequest r{};
    r.call = golbatch::CensusRequest::kBegin;
    r.max_keys = max_keys;
    if (const char* why = census_refusal(batch, r))
        return batch_err(batch, GOL_EINVAL, "gol_census_batch_begin: %s (max_keys %lld)", why, (long long)max_keys);
    const uint32_t capacity = golbatch::census_capacity(max_keys);
    BATCH_HIP(batch, hipSetDevice(batch->device));
    // what is missing is allocated before anything of the handle changes
    void* slots = nullptr;
    void* counters = nullptr;
    const size_t bytes = (size_t)capacity * sizeof(gol_census_entry);
    if ((capacity != batch->census_capacity && hipMalloc(&slots, bytes) != hipSuccess) ||
        (!batch->census_counters &&
         hipMalloc(&counters, golbatch::kCensusCounters * sizeof(unsigned long long)) != hipSuccess)) {
        (void)hipGetLastError();
        if (slots) hip_note(hipFree(slots), "gol_census_batch_begin: hipFree");
        return batch_err(batch, GOL_ENOMEM, "gol_census_batch_begin: hipMalloc of %zu bytes for a table of %u slots "
                         "failed; nothing changed", bytes, capacity);
    }
    if (counters) batch->census_counters = static_cast<unsigned long long*>(counters);
    if (slots) {  // nothing is in flight on the old table: every call synchronises
        if (batch->census_slots) hip_note(hipFree(batch->census_slots), "gol_census_batch_begin: hipFree");
        batch->census_slots = static_cast<unsigned long long*>(slots);
        batch->census_capacity = capacity;
    }
    batch->census_calls = 0;
    BATCH_HIP(batch, golbatch::launch_census_clear(census_table(batch), batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_census_batch_add(gol_batch* batch, int32_t reach, int32_t max_objects, uint32_t* call_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_add: null handle");
    golbatch::CensusRequest r{};
    r.call = golbatch::CensusRequest::kAdd;
    r.reach = reach;
    r.max_objects = max_objects;
    if (const char* why = census_refusal(batch, r))
        return batch_err(batch, GOL_EINVAL, "gol_census_batch_add: %s (reach %d, max_objects %d)", why, reach,
                         max_objects);
    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (const int rc = launch_objects(batch, "gol_census_batch_add", 0, batch->geo.boards, reach, max_objects))
        return rc;
    golbatch::CensusTallyParams p{};
    p.records = reinterpret_cast<const uint4*>(batch->obj_records);
    p.counts = batch->obj_counts;
    p.table = census_table(batch);
    p.total = (uint64_t)batch->geo.boards * (uint64_t)max_objects;
    p.max_objects = (uint32_t)max_objects;
    p.call = (uint32_t)batch->census_calls;
    BATCH_HIP(batch, golbatch::launch_census_tally(p, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    if (call_out) *call_out = p.call;
    ++batch->census_calls;
    return GOL_OK;
}

int gol_census_batch_add_records(gol_batch* batch, const gol_batch_object* records, size_t n, uint32_t board,
                                 uint32_t* call_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_add_records: null handle");
    golbatch::CensusRequest r{};
    r.call = golbatch::CensusRequest::kAddRecords;
    r.records_null = records == nullptr;
    r.n = n;
    r.board = board;
    if (const char* why = census_refusal(batch, r))
        return batch_err(batch, GOL_EINVAL, "gol_census_batch_add_records: %s (n %zu, board %u)", why, n, board);
    const uint32_t call = (uint32_t)batch->census_calls;
    if (n > 0) {
        BATCH_HIP(batch, hipSetDevice(batch->device));
        if (!grow(batch->census_in, batch->census_in_n, n, sizeof(gol_batch_object)))
            return batch_err(batch, GOL_ENOMEM, "gol_census_batch_add_records: hipMalloc for %zu records failed; "
                             "nothing tallied", n);
        // `records` outlives the copy: the call synchronises before it returns
        BATCH_HIP(batch, hipMemcpyAsync(batch->census_in, records, n * sizeof(gol_batch_object), hipMemcpyHostToDevice,
                                        batch->stream));
        golbatch::CensusTallyParams p{};
        p.records = reinterpret_cast<const uint4*>(batch->census_in);
        p.table = census_table(batch);
        p.total = n;
        p.board = board;
        p.call = call;
        BATCH_HIP(batch, golbatch::launch_census_tally(p, batch->stream));
        BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    }
    if (call_out) *call_out = call;
    ++batch->census_calls;
    return GOL_OK;
}

int gol_census_batch_read(gol_batch* batch, gol_census_entry* entries_out, size_t capacity, size_t* n_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_read: null handle");
    golbatch::CensusRequest r{};
    r.call = golbatch::CensusRequest::kRead;
    if (const char* why = census_refusal(batch, r)) return batch_err(batch, GOL_EINVAL, "gol_census_batch_read: %s", why);
    if (!n_out) return batch_err(batch, GOL_EINVAL, "gol_census_batch_read: n_out is null");
    BATCH_HIP(batch, hipSetDevice(batch->device));
    unsigned long long counters[golbatch::kCensusCounters];
    BATCH_HIP(batch, hipMemcpyAsync(counters, batch->census_counters, sizeof counters, hipMemcpyDeviceToHost,
                                    batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    const size_t n = (size_t)counters[golbatch::kCensusDistinct];
    *n_out = n;
    if (capacity < n || (n > 0 && !entries_out))
        return batch_err(batch, GOL_EINVAL, "gol_census_batch_read: entries_out holds %zu entries, the census has %zu "
                         "distinct keys", entries_out ? capacity : (size_t)0, n);
    if (n == 0) return GOL_OK;
    if (!grow(batch->census_out, batch->census_out_n, n, sizeof(gol_census_entry)))
        return batch_err(batch, GOL_ENOMEM, "gol_census_batch_read: hipMalloc for %zu entries failed; nothing written",
                         n);
    BATCH_HIP(batch, hipMemsetAsync(batch->census_counters + golbatch::kCensusCompacted, 0, sizeof(unsigned long long),
                                    batch->stream));
    BATCH_HIP(batch, golbatch::launch_census_compact(census_table(batch), reinterpret_cast<uint4*>(batch->census_out),
                                                     n, batch->stream));
    std::vector<gol_census_entry> got(n);
    unsigned long long compacted = 0;
    BATCH_HIP(batch, hipMemcpyAsync(got.data(), batch->census_out, n * sizeof(gol_census_entry), hipMemcpyDeviceToHost,
                                    batch->stream));
    BATCH_HIP(batch, hipMemcpyAsync(&compacted, batch->census_counters + golbatch::kCensusCompacted, sizeof compacted,
                                    hipMemcpyDeviceToHost, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    if (compacted != n)
        return batch_err(batch, GOL_ESTATE, "gol_census_batch_read: the table holds %llu occupied slots, its counter "
                         "says %zu distinct keys; nothing written", compacted, n);
    std::sort(got.begin(), got.end(), [](const gol_census_entry& a, const gol_census_entry& b) {
        if (a.count != b.count) return a.count > b.count;
        if (a.hash != b.hash) return a.hash < b.hash;
        if (a.w != b.w) return a.w < b.w;
        if (a.h != b.h) return a.h < b.h;
        return a.population < b.population;
    });
    std::copy(got.begin(), got.end(), entries_out);
    return GOL_OK;
}

int gol_census_batch_stats(gol_batch* batch, uint64_t* calls, uint64_t* seen, uint64_t* tallied, uint64_t* truncated,
                           uint64_t* overflowed, uint64_t* distinct) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_stats: null handle");
    unsigned long long counters[golbatch::kCensusCounters] = {};
    if (batch->census_capacity != 0) {
        BATCH_HIP(batch, hipSetDevice(batch->device));
        BATCH_HIP(batch, hipMemcpyAsync(counters, batch->census_counters, sizeof counters, hipMemcpyDeviceToHost,
                                        batch->stream));
        BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    }
    if (calls) *calls = batch->census_calls;
    if (seen) *seen = counters[golbatch::kCensusSeen];
    if (tallied) *tallied = counters[golbatch::kCensusTallied];
    if (truncated) *truncated = counters[golbatch::kCensusTruncated];
    if (overflowed) *overflowed = counters[golbatch::kCensusOverflowed];
    if (distinct) *distinct = counters[golbatch::kCensusDistinct];
    return GOL_OK;
}

int gol_rules_batch_check(const gol_batch_config* cfg, int64_t first, int64_t count, const uint32_t* rules) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_rules_batch_check: null configuration");
    golbatch::Geometry g;
    if (const char* why = golbatch::batch_geometry(*cfg, &g))
        return batch_err(nullptr, GOL_EINVAL, "batch of %d boards %d x %d: %s", cfg->boards, cfg->width, cfg->height,
                         why);
    int64_t which = -1;
    if (const char* why = golbatch::batch_rules_args(g, first, count, rules, &which))
        return rules_refusal(nullptr, "gol_rules_batch_check", why, g, first, count, rules, which);
    return GOL_OK;
}

int gol_rules_batch_set(gol_batch* batch, int64_t first, int64_t count, const uint32_t* rules) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_rules_batch_set: null handle");
    int64_t which = -1;
    if (const char* why = golbatch::batch_rules_args(batch->geo, first, count, rules, &which))
        return rules_refusal(batch, "gol_rules_batch_set", why, batch->geo, first, count, rules, which);
    const size_t boards = (size_t)batch->geo.boards;
    const uint32_t config_word = golbatch::rule_word(batch->birth, batch->survive);
    if (!rules) {  // the whole batch back to its configuration's rule; the device words stay for a later set
        batch->rules_on = false;
        std::fill(batch->rules_host.begin(), batch->rules_host.end(), config_word);
        return GOL_OK;
    }
    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (!batch->rules) {
        void* words = nullptr;
        if (hipMalloc(&words, boards * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            return batch_err(batch, GOL_ENOMEM, "gol_rules_batch_set: hipMalloc of %zu bytes for the rule words failed; "
                             "nothing changed", boards * sizeof(uint32_t));
        }
        batch->rules = static_cast<uint32_t*>(words);
    }
    // the device takes a copy of what the rules will be; the handle changes once it has arrived
    std::vector<uint32_t> next = batch->rules_host;
    if (next.empty()) next.assign(boards, config_word);
    std::copy(rules, rules + count, next.begin() + first);
    // while the configuration's rule is in force the device words are stale (or new): all of them go
    const size_t lo = batch->rules_on ? (size_t)first : 0, n = batch->rules_on ? (size_t)count : boards;
    BATCH_HIP(batch, hipMemcpyAsync(batch->rules + lo, next.data() + lo, n * sizeof(uint32_t), hipMemcpyHostToDevice,
                                    batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->rules_host.swap(next);
    batch->rules_on = true;
    return GOL_OK;
}

int gol_rules_batch_get(gol_batch* batch, int64_t first, int64_t count, uint32_t* rules_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_rules_batch_get: null handle");
    if (!rules_out) return batch_err(batch, GOL_EINVAL, "gol_rules_batch_get: rules_out is null");
    if (!window_ok(batch, first, count))
        return batch_err(batch, GOL_EINVAL, "gol_rules_batch_get: boards [%lld, %lld + %lld) outside the batch of %d",
                         (long long)first, (long long)first, (long long)count, batch->geo.boards);
    if (batch->rules_host.empty())
        std::fill(rules_out, rules_out + count, golbatch::rule_word(batch->birth, batch->survive));
    else
        std::copy(batch->rules_host.begin() + first, batch->rules_host.begin() + first + count, rules_out);
    return GOL_OK;
}

int gol_batch_epoch(const gol_batch* batch, uint64_t* epoch) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_epoch: null handle");
    if (!epoch) return batch_err(const_cast<gol_batch*>(batch), GOL_EINVAL, "gol_batch_epoch: epoch is null");
    *epoch = batch->epoch;
    return GOL_OK;
}

int gol_batch_set_chunk(gol_batch* batch, uint32_t generations_per_launch) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_set_chunk: null handle");
    batch->chunk = generations_per_launch;
    return GOL_OK;
}

}  // extern "C"
