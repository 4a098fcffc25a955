// gol_profile.cpp -- pass timing of a context (gol_profile_*): the Profiler
// keeps one record per profiled pass -- HIP event pairs around its main launch
// and, on a ring, its halo exchange and boundary launch, plus the main
// launch's clock-probe slot (gol_stencil.h clock_probe_*) -- and folds them
// into running totals by the rules of gol_profile.h.
#include <cstdlib>
#include <vector>

#include "gol_ctx.h"

static_assert(golprof::kClockSubSlots == gol::kClockSubSlots && golprof::kClockSubWords == gol::kClockSubWords &&
                  golprof::kClockSlotWords == gol::kClockSlotWords,
              "the fold reads a probe slot as the kernels write it");

namespace golc {

// Zeroes the first `slots` slots; a buffer that cannot be cleared is given up, not summed into again.
static hipError_t clear_clock(Accum<unsigned long long>& clk, size_t slots, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(clk.dev, 0, slots * golprof::kClockSlotWords * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) clk.clean = clk.count;
    else (void)clk.release();
    return e;
}

hipError_t Profiler::alloc_clock(hipStream_t stream) {
    const hipError_t e = clk.grow(kClockSlots, (size_t)kClockSlots * golprof::kClockSlotWords, 0);
    return e == hipSuccess && clk.clean < clk.count ? clear_clock(clk, clk.count, stream) : e;
}

hipError_t Profiler::begin(PassRecord** rec, hipStream_t stream) {
    *rec = nullptr;
    if (!on) return hipSuccess;
    if (kMaxPairs - pairs < 3 || used == kMaxPairs)  // (a record whose pass failed may hold no pair)
        if (hipError_t e = fold(stream)) return e;
    if (used == window.size()) window.emplace_back();
    PassRecord& r = window[used++];
    for (PassRecord::Part& p : r.part) p.started = p.stopped = false;
    r.clk_slot = -1;
    r.gens = 0;
    *rec = &r;
    return hipSuccess;
}

hipError_t Profiler::start(PassRecord* rec, ProfKind kind, hipStream_t stream) {
    PassRecord::Part& p = rec->part[kind];
    for (hipEvent_t* ev : {&p.start, &p.stop})
        if (!*ev)
            if (hipError_t e = hipEventCreate(ev)) return e;
    if (hipError_t e = hipEventRecord(p.start, stream)) return e;
    p.started = true;
    ++pairs;
    return hipSuccess;
}

hipError_t Profiler::stop(PassRecord* rec, ProfKind kind, hipStream_t stream) {
    PassRecord::Part& p = rec->part[kind];
    if (!p.started) return hipSuccess;
    if (hipError_t e = hipEventRecord(p.stop, stream)) return e;
    p.stopped = true;
    return hipSuccess;
}

unsigned long long* Profiler::main_launch(PassRecord* rec, int gens) {
    rec->gens = (uint32_t)gens;
    if (!clk.count || clk_used >= kClockSlots) return nullptr;
    clk.clean = 0;
    rec->clk_slot = (int)clk_used++;
    return clk.dev + (size_t)rec->clk_slot * golprof::kClockSlotWords;
}

hipError_t Profiler::fold(hipStream_t stream) {
    // the HIP half: every part with both events recorded, into its pass's sample.  The exchange and the
    // boundary launch are tied to the record's main launch (one that ran after them, a ring shard
    // without interior rows, ended after them: they add 0)
    std::vector<golprof::Sample> samples(used);
    for (size_t i = 0; i < used; ++i) {
        const PassRecord& r = window[i];
        const PassRecord::Part& m = r.part[kProfMain];
        golprof::Part* const out[3] = {&samples[i].main, &samples[i].exchange, &samples[i].boundary};
        for (int k = 0; k < 3; ++k) {
            const PassRecord::Part& p = r.part[k];
            if (!(p.started && p.stopped)) continue;
            const bool tied = k != kProfMain && m.started && m.stopped;
            float ms = 0.f, after = 0.f;
            if (hipError_t e = hipEventSynchronize(p.stop)) return e;
            if (hipError_t e = hipEventElapsedTime(&ms, p.start, p.stop)) return e;
            if (tied)
                if (hipError_t e = hipEventElapsedTime(&after, m.stop, p.stop)) return e;
            *out[k] = golprof::Part{true, tied, ms, after};
        }
        samples[i].generations = r.gens;
    }
    // every probed launch that counts has finished (its stop event fired): read the slots
    if (clk_used > 0) {
        std::vector<unsigned long long> words((size_t)clk_used * golprof::kClockSlotWords);
        if (hipError_t e = hipMemcpy(words.data(), clk.dev, words.size() * sizeof(words[0]), hipMemcpyDeviceToHost))
            return e;
        for (size_t i = 0; i < used; ++i)
            if (window[i].clk_slot >= 0)
                samples[i].main_ghz =
                    golprof::slot_clock_ghz(words.data() + (size_t)window[i].clk_slot * golprof::kClockSlotWords);
    }
    for (const golprof::Sample& s : samples) golprof::add(totals, s);  // the pure half
    used = pairs = 0;
    const size_t slots = clk_used;
    clk_used = 0;
    return slots ? clear_clock(clk, slots, stream) : hipSuccess;
}

void Profiler::destroy_events() {
    for (PassRecord& r : window)
        for (PassRecord::Part& p : r.part)
            for (hipEvent_t ev : {p.start, p.stop})
                if (ev) hip_note(hipEventDestroy(ev), "destroy: hipEventDestroy");
    window.clear();
    used = pairs = 0;
}

}  // namespace golc

using namespace golc;

namespace {

// What every reader does first: the context's device, then the window into the totals.
int folded(gol_ctx* ctx) {
    if (int rc = bind(ctx)) return rc;
    HIP_CHECK(ctx, ctx->profile.fold(ctx->compute));
    return GOL_OK;
}

}  // namespace

extern "C" {

int gol_profile_enable(gol_ctx* ctx, int enable) {
    if (!ctx) return set_err(nullptr, GOL_EINVAL, "null context");
    const char* probe = getenv("GOL_CLOCK_PROBE");  // "0": no in-kernel clock probe (A/B)
    if (enable && !ctx->profile.clk.count && !(probe && probe[0] == '0')) {
        if (int rc = bind(ctx)) return rc;
        const hipError_t e = ctx->profile.alloc_clock(ctx->compute);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return set_err(ctx, GOL_ENOMEM, "clock-probe buffer allocation failed");
        }
        HIP_CHECK(ctx, e);
    }
    ctx->profile.on = enable != 0;
    return GOL_OK;
}

int gol_profile_clock(gol_ctx* ctx, double* ghz) {
    if (!ctx || !ghz) return set_err(ctx, GOL_EINVAL, "null argument");
    if (int rc = folded(ctx)) return rc;
    *ghz = golprof::clock_ghz(ctx->profile.totals);
    return GOL_OK;
}

int gol_profile_read(gol_ctx* ctx, double* total_ms, uint64_t* launches, uint64_t* generations) {
    if (!ctx) return set_err(nullptr, GOL_EINVAL, "null context");
    if (int rc = folded(ctx)) return rc;
    const gol_profile_stats& st = ctx->profile.totals.stats;
    if (total_ms) *total_ms = st.kernel_ms;
    if (launches) *launches = st.launches;
    if (generations) *generations = st.generations;
    return GOL_OK;
}

int gol_profile_reset(gol_ctx* ctx) {
    if (!ctx) return set_err(nullptr, GOL_EINVAL, "null context");
    if (int rc = folded(ctx)) return rc;
    ctx->profile.totals = golprof::Totals{};
    return GOL_OK;
}

int gol_profile_stats_read(gol_ctx* ctx, gol_profile_stats* out) {
    if (!ctx || !out) return set_err(ctx, GOL_EINVAL, "null argument");
    if (int rc = folded(ctx)) return rc;
    *out = ctx->profile.totals.stats;
    out->clock_ghz = golprof::clock_ghz(ctx->profile.totals);
    return GOL_OK;
}

}  // extern "C"
