// gol_batch.cpp -- C ABI of the batch engine (include/gol.h gol_batch_*,
// gol_cycle_*, gol_find_batch*, gol_objects_batch*, gol_census_batch*,
// gol_rules_batch_* and gol_soup_batch*; DESIGN.md sections 5f to 5l): many independent boards of at most 64 x 64
// stored cells stepped by one launch (kernels: gol_batch.hip), searched by one
// (gol_batch_find.hip), cut into their objects by one (gol_batch_objects.hip),
// those tallied by one (gol_batch_census.hip) and filled with soups by one (gol_batch_soup.hip).  A
// handle type of its own: it shares the error conventions and the HIP status
// discipline with the contexts (gol_ctx.h), and nothing else -- no planner, no
// step kernel.  Every device buffer of the handle has one owner (DevBuf), the
// handle's fields are grouped by the calls they serve, and a refusal that more
// than one entry point gives is formatted in one place.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "gol_batch.h"
#include "gol_ctx.h"

namespace {

using golc::hip_note;

// A device buffer of the handle and its owner (golc::Accum's idiom, as small
// as the batch needs): the pointer and how many elements it holds.  Whoever
// destroys it has set the device and synchronised the stream.
template <class T>
struct DevBuf {
    T* dev = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release("batch destroy: hipFree"); }
    // Forgets the buffer before freeing it; a failing hipFree is noted under the caller's label.
    void release(const char* label) {
        T* const d = dev;
        dev = nullptr;
        count = 0;
        if (d) hip_note(hipFree(d), label);
    }
    // Holds at least n elements afterwards.  A buffer that is too small is replaced (nothing is in flight on it:
    // every call synchronises); false, with nothing held and the HIP status taken off the thread, if it cannot be.
    bool grow(size_t n, const char* label) {
        if (n <= count) return true;
        release(label);
        void* p = nullptr;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        dev = static_cast<T*>(p);
        count = n;
        return true;
    }
    void swap(DevBuf& o) {
        std::swap(dev, o.dev);
        std::swap(count, o.count);
    }
};

}  // namespace

struct gol_batch {
    golbatch::Geometry geo{};
    golbatch::Lanes lanes{};
    uint32_t birth = 0, survive = 0;
    int device = 0;
    uint32_t chunk = 0;  // gol_batch_set_chunk (0: automatic)
    uint64_t epoch = 0;
    hipStream_t stream = nullptr;
    DevBuf<unsigned long long> plane;  // boards * height rows
    // the plane one generation before (settle detection across launches), or a cycle call's snapshot plane: a call
    // is one or the other, and neither reads what an earlier call left in it
    DevBuf<unsigned long long> prev;
    DevBuf<uint32_t> settled;  // [boards]
    DevBuf<uint32_t> series;   // the series of one launch, [boards][count / boards], grown on demand
    // gol_cycle_step's words, allocated by its first call: period [boards], seen [boards], then the two counters
    // (boards that have a period, the largest period); gol_cycle_stats: the last gol_cycle_step call
    struct {
        DevBuf<uint32_t> words;
        uint64_t launches = 0, boards = 0;
        uint32_t max_period = 0;
    } cycle;
    // gol_batch_hashes' results, grown on demand and together
    struct {
        DevBuf<unsigned long long> values;
        DevBuf<uint32_t> pops;
    } hashes;
    // gol_find_batch's buffers, grown on demand: the pattern table (headers, then the row pairs), the counts
    // [boards][npatterns] and the match planes [npatterns][boards][height]
    struct {
        DevBuf<unsigned char> table;
        DevBuf<uint32_t> counts;
        DevBuf<unsigned long long> matches;
        uint32_t cut = 0;                  // gol_find_batch_set_cut (0: automatic)
        uint64_t launches = 0, cared = 0;  // gol_find_batch_stats: the last gol_find_batch call
    } find;
    // gol_objects_batch's buffers, grown on demand: the counts [count] and the records [count][max_objects]
    struct {
        DevBuf<uint32_t> counts;
        DevBuf<gol_batch_object> records;
        uint64_t launches = 0, total = 0, truncated = 0;  // gol_objects_batch_stats: the last gol_objects_batch call
    } objects;
    // gol_census_batch_*'s table (four qwords a slot; none: no census has begun) and counters, the calls since
    // begin, and the buffers, grown on demand, add_records' records and read's entries pass through
    struct {
        DevBuf<unsigned long long> slots, counters;
        uint64_t calls = 0;
        DevBuf<gol_batch_object> in;
        DevBuf<gol_census_entry> out;
        uint32_t capacity() const { return (uint32_t)(slots.count / 4); }
        golbatch::CensusTable table() const { return {slots.dev, counters.dev, capacity()}; }
    } census;
    // gol_rules_batch_*: the device's rule words [boards], allocated by the first set; their host copy, the rules
    // in force (empty before the first set: the configuration's rule everywhere); and whether the steps launch the
    // RULES instances
    struct {
        DevBuf<uint32_t> words;
        std::vector<uint32_t> host;
        bool on = false;
    } rules;
    // gol_soup_batch: the fundamental domain's row masks of the call's spec, allocated by the first call
    struct {
        DevBuf<unsigned long long> domain;  // [golsoup::kMaxSide]
    } soup;
    std::string err;
};

namespace {

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

// The buffers release themselves with the handle, after the stream has drained and before it goes.
void destroy_impl(gol_batch* b) {
    hip_note(hipSetDevice(b->device), "batch destroy: hipSetDevice");
    const hipStream_t stream = b->stream;
    if (stream) hip_note(hipStreamSynchronize(stream), "batch destroy: hipStreamSynchronize");
    delete b;
    if (stream) hip_note(hipStreamDestroy(stream), "batch destroy: hipStreamDestroy");
}

// The geometry of a configuration, or its refusal as a message
int config_geometry(const gol_batch_config* cfg, golbatch::Geometry* g) {
    if (const char* why = golbatch::batch_geometry(*cfg, g))
        return batch_err(nullptr, GOL_EINVAL, "batch of %d boards %d x %d: %s", cfg->boards, cfg->width, cfg->height,
                         why);
    return GOL_OK;
}

// window_ok's refusal as a message
int window_refusal(gol_batch* b, const char* fn, int64_t first, int64_t count) {
    return batch_err(b, GOL_EINVAL, "%s: boards [%lld, %lld + %lld) outside the batch of %d", fn, (long long)first,
                     (long long)first, (long long)count, b->geo.boards);
}

// A launch's parameters with what they take from the handle's geometry: boards, width, height, boards_per_wave
// and, where P has them, vis_w and vis_h
template <class P>
auto set_visible(P& p, const golbatch::Geometry& g, int) -> decltype((void)p.vis_w) {
    p.vis_w = g.vis_w;
    p.vis_h = g.vis_h;
}
template <class P>
void set_visible(P&, const golbatch::Geometry&, long) {}
template <class P>
P launch_params(const gol_batch* b) {
    P p{};
    p.boards = b->geo.boards;
    p.width = b->geo.width;
    p.height = b->geo.height;
    p.boards_per_wave = b->lanes.boards_per_wave;
    set_visible(p, b->geo, 0);
    return p;
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
    if (!batch->objects.counts.grow(n, "gol_objects_batch: hipFree") ||
        !batch->objects.records.grow(records_n, "gol_objects_batch: hipFree"))
        return batch_err(batch, GOL_ENOMEM, "%s: hipMalloc of the counts (%zu entries) or the records "
                         "(%zu entries) failed; nothing written", fn, n, records_n);
    // the records past a board's count are zero: one memset before the launch, the kernel stores the real ones only
    BATCH_HIP(batch, hipMemsetAsync(batch->objects.records.dev, 0, records_n * sizeof(gol_batch_object), batch->stream));
    auto p = launch_params<golbatch::ObjectsParams>(batch);
    p.plane = batch->plane.dev;
    p.counts = batch->objects.counts.dev;
    p.objects = reinterpret_cast<uint4*>(batch->objects.records.dev);
    p.boards = (int32_t)(first + count);  // the end of the range
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

// batch_soup_args' refusal as a message, with the window and the range it is about
int soup_refusal(gol_batch* b, const char* fn, const char* why, const golbatch::Geometry& g, const gol_soup_spec* s,
                 int64_t first, int64_t count) {
    if (!s) return batch_err(b, GOL_EINVAL, "%s: %s", fn, why);
    return batch_err(b, GOL_EINVAL, "%s: %s (window %d x %d at (%d, %d), density %d, symmetry %d, first %lld, count "
                     "%lld, batch of %d boards %d x %d)", fn, why, s->w, s->h, s->x, s->y, s->density, s->symmetry,
                     (long long)first, (long long)count, g.boards, g.width, g.height);
}

// batch_census_args for a call of this handle: the request's handle fields filled in
const char* census_refusal(const gol_batch* b, golbatch::CensusRequest r) {
    r.begun = b->census.capacity() != 0;
    r.next_call = b->census.calls;
    return golbatch::batch_census_args(b->geo, r);
}

// The census's counters as the device has them now
int census_counters(gol_batch* batch, unsigned long long (&counters)[golbatch::kCensusCounters]) {
    BATCH_HIP(batch, hipSetDevice(batch->device));
    BATCH_HIP(batch, hipMemcpyAsync(counters, batch->census.counters.dev, sizeof counters, hipMemcpyDeviceToHost,
                                    batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

}  // namespace

extern "C" {

int gol_batch_geometry_get(const gol_batch_config* cfg, gol_batch_geometry* out) {
    if (!cfg || !out) return batch_err(nullptr, GOL_EINVAL, "gol_batch_geometry_get: null argument");
    golbatch::Geometry g;
    if (const int rc = config_geometry(cfg, &g)) return rc;
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
    if (const int rc = config_geometry(cfg, &g)) return rc;
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
    const char* const label = "gol_batch_create: hipFree";
    if (!b->plane.grow(plane_words(b), label) || !b->prev.grow(plane_words(b), label) ||
        !b->settled.grow((size_t)g.boards, label))
        return fail(GOL_ENOMEM, "hipMalloc of the planes");
    if (hipMemset(b->plane.dev, 0, bytes) != hipSuccess || hipMemset(b->prev.dev, 0, bytes) != hipSuccess ||
        hipMemset(b->settled.dev, 0, settle_bytes) != hipSuccess)
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
    BATCH_HIP(batch, golbatch::launch_batch_seed(batch->plane.dev, (int64_t)plane_words(batch), batch->geo.width, seed,
                                                 batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->epoch = 0;
    return GOL_OK;
}

int gol_batch_load(gol_batch* batch, int64_t first, int64_t count, const uint64_t* rows) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_load: null handle");
    if (!rows) return batch_err(batch, GOL_EINVAL, "gol_batch_load: rows is null");
    if (!golbatch::window_ok(batch->geo, first, count)) return window_refusal(batch, "gol_batch_load", first, count);
    const size_t H = (size_t)batch->geo.height, n = (size_t)count * H;
    const uint64_t wmask = batch->geo.width >= 64 ? ~0ull : (1ull << batch->geo.width) - 1ull;
    std::vector<uint64_t> masked(n);  // bits at x >= width are ignored
    for (size_t i = 0; i < n; ++i) masked[i] = rows[i] & wmask;
    BATCH_HIP(batch, hipSetDevice(batch->device));
    BATCH_HIP(batch, hipMemcpyAsync(batch->plane.dev + (size_t)first * H, masked.data(), n * sizeof(uint64_t),
                                    hipMemcpyHostToDevice, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->epoch = 0;
    return GOL_OK;
}

int gol_batch_snapshot(gol_batch* batch, int64_t first, int64_t count, uint64_t* rows) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_snapshot: null handle");
    if (!rows) return batch_err(batch, GOL_EINVAL, "gol_batch_snapshot: rows is null");
    if (!golbatch::window_ok(batch->geo, first, count)) return window_refusal(batch, "gol_batch_snapshot", first, count);
    const size_t H = (size_t)batch->geo.height;
    BATCH_HIP(batch, hipSetDevice(batch->device));
    // the plane never holds a bit at x >= width: every writer masks
    BATCH_HIP(batch, hipMemcpyAsync(rows, batch->plane.dev + (size_t)first * H, (size_t)count * H * sizeof(uint64_t),
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
    if (populations_out && !batch->series.grow(boards * (size_t)chunk, "gol_batch_step: hipFree"))
        return batch_err(batch, GOL_ENOMEM, "gol_batch_step: hipMalloc of %zu bytes for the population series "
                         "failed; nothing advanced", boards * (size_t)chunk * sizeof(uint32_t));
    const size_t series_gens = batch->series.count / boards;  // >= chunk with populations_out
    auto p = launch_params<golbatch::StepParams>(batch);
    p.plane = batch->plane.dev;
    p.prev = batch->prev.dev;
    p.pops = populations_out ? batch->series.dev : nullptr;
    p.settled = settled_out ? batch->settled.dev : nullptr;
    p.pop_stride = (uint32_t)series_gens;
    p.birth = batch->birth;
    p.survive = batch->survive;
    p.rules = batch->rules.on ? batch->rules.words.dev : nullptr;
    for (uint32_t g0 = 0; g0 < generations; g0 += chunk) {
        p.gens = std::min(chunk, generations - g0);
        p.g0 = g0;
        BATCH_HIP(batch, golbatch::launch_batch_step(p, life_rule(batch), batch->geo.clipped, batch->rules.on,
                                                     batch->stream));
        batch->epoch += p.gens;
        if (populations_out)  // this launch's columns of the caller's [boards][generations]; waits for the launch
            BATCH_HIP(batch, hipMemcpy2DAsync(populations_out + g0, (size_t)generations * sizeof(uint32_t),
                                              batch->series.dev, series_gens * sizeof(uint32_t), (size_t)p.gens * sizeof(uint32_t),
                                              boards, hipMemcpyDeviceToHost, batch->stream));
    }
    if (settled_out)
        BATCH_HIP(batch, hipMemcpyAsync(settled_out, batch->settled.dev, boards * sizeof(uint32_t), hipMemcpyDeviceToHost,
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
    if (!batch->cycle.words.grow(2 * boards + 2, "gol_cycle_step: hipFree"))
        return batch_err(batch, GOL_ENOMEM, "gol_cycle_step: hipMalloc of %zu bytes for the period and seen words "
                         "failed; nothing advanced", (2 * boards + 2) * sizeof(uint32_t));
    auto p = launch_params<golbatch::CycleParams>(batch);
    p.plane = batch->plane.dev;
    p.snap = batch->prev.dev;
    p.period = batch->cycle.words.dev;
    p.seen = batch->cycle.words.dev + boards;
    p.counters = batch->cycle.words.dev + 2 * boards;
    p.birth = batch->birth;
    p.survive = batch->survive;
    p.rules = batch->rules.on ? batch->rules.words.dev : nullptr;
    // the first launch of a call reads neither the words nor the snapshot plane; the counters start at zero
    BATCH_HIP(batch, hipMemsetAsync(p.counters, 0, 2 * sizeof(uint32_t), batch->stream));
    batch->cycle.launches = 0;
    uint32_t counters[2] = {0u, 0u};
    for (uint32_t g0 = 0; g0 < generations; g0 += p.gens) {
        // every board cycled: a launch fast-forwards, at most max_period - 1 generations per board whatever it is
        // asked for, so the remainder goes as one launch unless a chunk launch is the shorter
        const bool all = counters[0] == boards && counters[1] - 1u <= chunk;
        p.gens = all ? generations - g0 : std::min(chunk, generations - g0);
        p.g0 = g0;
        BATCH_HIP(batch, golbatch::launch_batch_cycle(p, life_rule(batch), batch->geo.clipped, batch->rules.on,
                                                      batch->stream));
        batch->epoch += p.gens;
        ++batch->cycle.launches;
        BATCH_HIP(batch, hipMemcpyAsync(counters, p.counters, sizeof counters, hipMemcpyDeviceToHost, batch->stream));
        BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
        batch->cycle.boards = counters[0];
        batch->cycle.max_period = counters[1];
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
    if (launches) *launches = batch->cycle.launches;
    if (boards_cycled) *boards_cycled = batch->cycle.boards;
    if (max_period) *max_period = batch->cycle.max_period;
    return GOL_OK;
}

int gol_batch_hashes(gol_batch* batch, int64_t first, int64_t count, uint64_t* hashes_out,
                     uint32_t* populations_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_batch_hashes: null handle");
    if (!hashes_out && !populations_out) return batch_err(batch, GOL_EINVAL, "gol_batch_hashes: both arrays are null");
    if (!golbatch::window_ok(batch->geo, first, count)) return window_refusal(batch, "gol_batch_hashes", first, count);
    BATCH_HIP(batch, hipSetDevice(batch->device));
    const size_t n = (size_t)count;
    const char* const label = "gol_batch_hashes: hipFree";
    if (!batch->hashes.values.grow(n, label) || !batch->hashes.pops.grow(n, label)) {
        batch->hashes.values.release(label);  // both or neither
        batch->hashes.pops.release(label);
        return batch_err(batch, GOL_ENOMEM, "gol_batch_hashes: hipMalloc for %zu boards failed", n);
    }
    BATCH_HIP(batch, golbatch::launch_batch_hashes(batch->plane.dev, batch->geo.height, first, count,
                                                   hashes_out ? batch->hashes.values.dev : nullptr,
                                                   populations_out ? batch->hashes.pops.dev : nullptr, batch->stream));
    if (hashes_out)
        BATCH_HIP(batch, hipMemcpyAsync(hashes_out, batch->hashes.values.dev, n * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                        batch->stream));
    if (populations_out)
        BATCH_HIP(batch, hipMemcpyAsync(populations_out, batch->hashes.pops.dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                        batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_find_batch_check(const gol_batch_config* cfg, const gol_batch_pattern* patterns, int32_t npatterns) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_find_batch_check: null configuration");
    golbatch::Geometry g;
    if (const int rc = config_geometry(cfg, &g)) return rc;
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
    const char* const label = "gol_find_batch: hipFree";
    if (!batch->find.table.grow(table_bytes, label) || !batch->find.counts.grow(counts_n, label) ||
        (matches_out && !batch->find.matches.grow(matches_n, label)))
        return batch_err(batch, GOL_ENOMEM, "gol_find_batch: hipMalloc of the pattern table (%zu bytes), the counts "
                         "(%zu entries) or the match planes (%zu entries) failed; nothing written", table_bytes,
                         counts_n, matches_out ? matches_n : (size_t)0);
    // `table` outlives the copy: the call synchronises before it returns
    BATCH_HIP(batch, hipMemcpyAsync(batch->find.table.dev, table.data(), table_bytes, hipMemcpyHostToDevice, batch->stream));
    auto fp = launch_params<golbatch::FindParams>(batch);
    fp.plane = batch->plane.dev;
    fp.counts = batch->find.counts.dev;
    fp.matches = matches_out ? batch->find.matches.dev : nullptr;
    fp.npatterns = npatterns;
    const auto* dev_heads = reinterpret_cast<const golbatch::FindPattern*>(batch->find.table.dev);
    const auto* dev_rows = reinterpret_cast<const unsigned long long*>(batch->find.table.dev + head_bytes);
    // the cut: as many patterns per launch as stay within the bound, one at least
    const uint64_t cut = batch->find.cut ? batch->find.cut : golbatch::kAutoFindCut;
    batch->find.launches = 0;
    batch->find.cared = cared_all;
    for (int32_t first = 0; first < npatterns; first += fp.count) {
        uint64_t cared = heads[first].cared;
        int32_t n = 1;
        while (first + n < npatterns && cared + heads[first + n].cared <= cut) cared += heads[first + n++].cared;
        fp.first = first;
        fp.count = n;
        BATCH_HIP(batch, golbatch::launch_batch_find(fp, dev_heads, dev_rows, batch->geo.clipped, batch->stream));
        ++batch->find.launches;
    }
    BATCH_HIP(batch, hipMemcpyAsync(counts_out, batch->find.counts.dev, counts_n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                    batch->stream));
    if (matches_out)
        BATCH_HIP(batch, hipMemcpyAsync(matches_out, batch->find.matches.dev, matches_n * sizeof(uint64_t),
                                        hipMemcpyDeviceToHost, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    return GOL_OK;
}

int gol_find_batch_set_cut(gol_batch* batch, uint32_t cared_cells_per_launch) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_find_batch_set_cut: null handle");
    batch->find.cut = cared_cells_per_launch;
    return GOL_OK;
}

int gol_find_batch_stats(gol_batch* batch, uint64_t* launches, uint64_t* cared_cells) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_find_batch_stats: null handle");
    if (launches) *launches = batch->find.launches;
    if (cared_cells) *cared_cells = batch->find.cared;
    return GOL_OK;
}

int gol_objects_batch_check(const gol_batch_config* cfg, int64_t first, int64_t count, int32_t reach,
                            int32_t max_objects) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_objects_batch_check: null configuration");
    golbatch::Geometry g;
    if (const int rc = config_geometry(cfg, &g)) return rc;
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
    BATCH_HIP(batch, hipMemcpyAsync(counts_out, batch->objects.counts.dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                    batch->stream));
    BATCH_HIP(batch, hipMemcpyAsync(objects_out, batch->objects.records.dev, records_n * sizeof(gol_batch_object),
                                    hipMemcpyDeviceToHost, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->objects.launches = 1;
    batch->objects.total = batch->objects.truncated = 0;
    for (size_t i = 0; i < n; ++i) {
        batch->objects.total += counts_out[i];
        batch->objects.truncated += counts_out[i] > (uint32_t)max_objects ? 1u : 0u;
    }
    return GOL_OK;
}

int gol_objects_batch_stats(gol_batch* batch, uint64_t* launches, uint64_t* objects, uint64_t* boards_truncated) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_objects_batch_stats: null handle");
    if (launches) *launches = batch->objects.launches;
    if (objects) *objects = batch->objects.total;
    if (boards_truncated) *boards_truncated = batch->objects.truncated;
    return GOL_OK;
}

int gol_census_batch_check(const gol_batch_config* cfg, int32_t reach, int32_t max_objects, int64_t max_keys) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_check: null configuration");
    golbatch::Geometry g;
    if (const int rc = config_geometry(cfg, &g)) return rc;
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
    // what is missing (a table of another size, smaller ones too: the capacity is the probe mask) is allocated
    // before anything of the handle changes, and swapped in once all of it is there
    const char* const label = "gol_census_batch_begin: hipFree";
    DevBuf<unsigned long long> slots, counters;
    if ((capacity != batch->census.capacity() && !slots.grow(4 * (size_t)capacity, label)) ||
        (!batch->census.counters.dev && !counters.grow(golbatch::kCensusCounters, label))) {
        slots.release(label);
        return batch_err(batch, GOL_ENOMEM, "gol_census_batch_begin: hipMalloc of %zu bytes for a table of %u slots "
                         "failed; nothing changed", (size_t)capacity * sizeof(gol_census_entry), capacity);
    }
    if (counters.dev) batch->census.counters.swap(counters);
    if (slots.dev) {  // nothing is in flight on the old table: every call synchronises
        batch->census.slots.swap(slots);
        slots.release(label);
    }
    batch->census.calls = 0;
    BATCH_HIP(batch, golbatch::launch_census_clear(batch->census.table(), batch->stream));
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
    p.records = reinterpret_cast<const uint4*>(batch->objects.records.dev);
    p.counts = batch->objects.counts.dev;
    p.table = batch->census.table();
    p.total = (uint64_t)batch->geo.boards * (uint64_t)max_objects;
    p.max_objects = (uint32_t)max_objects;
    p.call = (uint32_t)batch->census.calls;
    BATCH_HIP(batch, golbatch::launch_census_tally(p, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    if (call_out) *call_out = p.call;
    ++batch->census.calls;
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
    const uint32_t call = (uint32_t)batch->census.calls;
    if (n > 0) {
        BATCH_HIP(batch, hipSetDevice(batch->device));
        if (!batch->census.in.grow(n, "gol_census_batch_add_records: hipFree"))
            return batch_err(batch, GOL_ENOMEM, "gol_census_batch_add_records: hipMalloc for %zu records failed; "
                             "nothing tallied", n);
        // `records` outlives the copy: the call synchronises before it returns
        BATCH_HIP(batch, hipMemcpyAsync(batch->census.in.dev, records, n * sizeof(gol_batch_object), hipMemcpyHostToDevice,
                                        batch->stream));
        golbatch::CensusTallyParams p{};
        p.records = reinterpret_cast<const uint4*>(batch->census.in.dev);
        p.table = batch->census.table();
        p.total = n;
        p.board = board;
        p.call = call;
        BATCH_HIP(batch, golbatch::launch_census_tally(p, batch->stream));
        BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    }
    if (call_out) *call_out = call;
    ++batch->census.calls;
    return GOL_OK;
}

int gol_census_batch_read(gol_batch* batch, gol_census_entry* entries_out, size_t capacity, size_t* n_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_census_batch_read: null handle");
    golbatch::CensusRequest r{};
    r.call = golbatch::CensusRequest::kRead;
    if (const char* why = census_refusal(batch, r)) return batch_err(batch, GOL_EINVAL, "gol_census_batch_read: %s", why);
    if (!n_out) return batch_err(batch, GOL_EINVAL, "gol_census_batch_read: n_out is null");
    unsigned long long counters[golbatch::kCensusCounters];
    if (const int rc = census_counters(batch, counters)) return rc;
    const size_t n = (size_t)counters[golbatch::kCensusDistinct];
    *n_out = n;
    if (capacity < n || (n > 0 && !entries_out))
        return batch_err(batch, GOL_EINVAL, "gol_census_batch_read: entries_out holds %zu entries, the census has %zu "
                         "distinct keys", entries_out ? capacity : (size_t)0, n);
    if (n == 0) return GOL_OK;
    if (!batch->census.out.grow(n, "gol_census_batch_read: hipFree"))
        return batch_err(batch, GOL_ENOMEM, "gol_census_batch_read: hipMalloc for %zu entries failed; nothing written",
                         n);
    BATCH_HIP(batch, hipMemsetAsync(batch->census.counters.dev + golbatch::kCensusCompacted, 0, sizeof(unsigned long long),
                                    batch->stream));
    BATCH_HIP(batch, golbatch::launch_census_compact(batch->census.table(), reinterpret_cast<uint4*>(batch->census.out.dev),
                                                     n, batch->stream));
    std::vector<gol_census_entry> got(n);
    unsigned long long compacted = 0;
    BATCH_HIP(batch, hipMemcpyAsync(got.data(), batch->census.out.dev, n * sizeof(gol_census_entry), hipMemcpyDeviceToHost,
                                    batch->stream));
    BATCH_HIP(batch, hipMemcpyAsync(&compacted, batch->census.counters.dev + golbatch::kCensusCompacted, sizeof compacted,
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
    if (batch->census.capacity() != 0)
        if (const int rc = census_counters(batch, counters)) return rc;
    if (calls) *calls = batch->census.calls;
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
    if (const int rc = config_geometry(cfg, &g)) return rc;
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
        batch->rules.on = false;
        std::fill(batch->rules.host.begin(), batch->rules.host.end(), config_word);
        return GOL_OK;
    }
    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (!batch->rules.words.grow(boards, "gol_rules_batch_set: hipFree"))
        return batch_err(batch, GOL_ENOMEM, "gol_rules_batch_set: hipMalloc of %zu bytes for the rule words failed; "
                         "nothing changed", boards * sizeof(uint32_t));
    // the device takes a copy of what the rules will be; the handle changes once it has arrived
    std::vector<uint32_t> next = batch->rules.host;
    if (next.empty()) next.assign(boards, config_word);
    std::copy(rules, rules + count, next.begin() + first);
    // while the configuration's rule is in force the device words are stale (or new): all of them go
    const size_t lo = batch->rules.on ? (size_t)first : 0, n = batch->rules.on ? (size_t)count : boards;
    BATCH_HIP(batch, hipMemcpyAsync(batch->rules.words.dev + lo, next.data() + lo, n * sizeof(uint32_t), hipMemcpyHostToDevice,
                                    batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->rules.host.swap(next);
    batch->rules.on = true;
    return GOL_OK;
}

int gol_rules_batch_get(gol_batch* batch, int64_t first, int64_t count, uint32_t* rules_out) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_rules_batch_get: null handle");
    if (!rules_out) return batch_err(batch, GOL_EINVAL, "gol_rules_batch_get: rules_out is null");
    if (!golbatch::window_ok(batch->geo, first, count)) return window_refusal(batch, "gol_rules_batch_get", first, count);
    if (batch->rules.host.empty())
        std::fill(rules_out, rules_out + count, golbatch::rule_word(batch->birth, batch->survive));
    else
        std::copy(batch->rules.host.begin() + first, batch->rules.host.begin() + first + count, rules_out);
    return GOL_OK;
}

int gol_soup_batch_check(const gol_batch_config* cfg, const gol_soup_spec* spec, int64_t first, int64_t count) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_soup_batch_check: null configuration");
    golbatch::Geometry g;
    if (const int rc = config_geometry(cfg, &g)) return rc;
    if (const char* why = golbatch::batch_soup_args(g, spec, first, count))
        return soup_refusal(nullptr, "gol_soup_batch_check", why, g, spec, first, count);
    return GOL_OK;
}

int gol_soup_batch(gol_batch* batch, const gol_soup_spec* spec, int64_t first, int64_t count) {
    if (!batch) return batch_err(nullptr, GOL_EINVAL, "gol_soup_batch: null handle");
    if (const char* why = golbatch::batch_soup_args(batch->geo, spec, first, count))
        return soup_refusal(batch, "gol_soup_batch", why, batch->geo, spec, first, count);
    golsoup::Plan plan;  // the domain's row masks are the spec's alone: computed here, read by every wave
    golsoup::make_plan(*spec, &plan);
    BATCH_HIP(batch, hipSetDevice(batch->device));
    if (!batch->soup.domain.grow(golsoup::kMaxSide, "gol_soup_batch: hipFree"))
        return batch_err(batch, GOL_ENOMEM, "gol_soup_batch: hipMalloc of %zu bytes for the domain words failed; "
                         "nothing changed", (size_t)golsoup::kMaxSide * sizeof(uint64_t));
    // `plan` outlives the copy: the call synchronises before it returns
    BATCH_HIP(batch, hipMemcpyAsync(batch->soup.domain.dev, plan.domain, sizeof plan.domain, hipMemcpyHostToDevice,
                                    batch->stream));
    auto p = launch_params<golbatch::SoupParams>(batch);
    p.plane = batch->plane.dev;
    p.domain = batch->soup.domain.dev;
    p.spec = *spec;
    p.first = (int32_t)first;  // inside the batch: both fit
    p.count = (int32_t)count;
    BATCH_HIP(batch, golbatch::launch_batch_soup(p, batch->stream));
    BATCH_HIP(batch, hipStreamSynchronize(batch->stream));
    batch->epoch = 0;
    return GOL_OK;
}

int gol_soup_batch_rows(const gol_batch_config* cfg, const gol_soup_spec* spec, int64_t first, int64_t count,
                        uint64_t* rows_out, size_t capacity) {
    if (!cfg) return batch_err(nullptr, GOL_EINVAL, "gol_soup_batch_rows: null configuration");
    golbatch::Geometry g;
    if (const int rc = config_geometry(cfg, &g)) return rc;
    if (const char* why = golbatch::batch_soup_args(g, spec, first, count))
        return soup_refusal(nullptr, "gol_soup_batch_rows", why, g, spec, first, count);
    if (!rows_out) return batch_err(nullptr, GOL_EINVAL, "gol_soup_batch_rows: rows_out is null");
    const size_t need = (size_t)count * (size_t)g.height;  // <= 2^22 * 2^6
    if (capacity < need)
        return batch_err(nullptr, GOL_EINVAL, "gol_soup_batch_rows: rows_out holds %zu entries, %lld boards x %d rows "
                         "need %zu", capacity, (long long)count, g.height, need);
    golsoup::batch_rows(*spec, g.height, first, count, rows_out);
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
