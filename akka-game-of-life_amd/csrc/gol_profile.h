// gol_profile.h -- the accounting of pass timing as pure functions of plain
// numbers: a probe slot's clock, and what one profiled pass adds to the totals
// of gol_profile_stats (include/gol.h).  No HIP, no context: checked with a
// plain host compiler (tests/profile_probe.cpp); gol_profile.cpp fills Samples.
#pragma once
#include <algorithm>

#include "../../include/gol.h"

namespace golprof {

// A launch's clock-probe slot (gol_stencil.h clock_probe_*): kClockSubSlots
// sub-slots one 64-byte line apart, each summing the core-clock ticks (word 0)
// and 100 MHz reference ticks (word 1) of the workgroups that report into it.
constexpr int kClockSubSlots = 64;
constexpr int kClockSubWords = 8;
constexpr int kClockSlotWords = kClockSubSlots * kClockSubWords;

// Clock (GHz) one launch ran at, from its slot; 0.0: no workgroup reported.
inline double slot_clock_ghz(const unsigned long long* w) {
    unsigned long long mt = 0, rt = 0;
    for (int k = 0; k < kClockSubSlots; ++k) {
        mt += w[k * kClockSubWords + 0];
        rt += w[k * kClockSubWords + 1];
    }
    return rt ? (double)mt / (double)rt * 0.1 : 0.0;
}

// A part of a pass, if timed: its duration and, for an exchange or a boundary
// launch tied to the pass's main launch, how long after that launch's end it
// ended (negative: before).
struct Part {
    bool timed = false, tied = false;
    double ms = 0.0, after_ms = 0.0;
};

// One profiled pass: its main launch (the whole shard, or the interior rows), the generations that
// advances and the clock its slot gave (0.0: none), its halo exchange and its boundary launch.
struct Sample {
    Part main, exchange, boundary;
    double main_ghz = 0.0;
    unsigned generations = 0;
};

// gol_profile_stats as summed (its clock_ghz stays 0: clock_ghz() below) and
// the two sums over the main launches whose slot gave a clock.
struct Totals {
    gol_profile_stats stats{};
    double clk_ms_ghz = 0.0, clk_ms = 0.0;
};

// How far a tied part ended after the main launch; 0 if before, or not tied.
inline double exposed_ms(const Part& p) { return p.tied ? std::max(p.after_ms, 0.0) : 0.0; }

inline void add(Totals& t, const Sample& s) {
    gol_profile_stats& st = t.stats;
    if (s.main.timed) {
        st.kernel_ms += s.main.ms;
        st.launches += 1;
        st.generations += s.generations;
        t.clk_ms_ghz += s.main_ghz > 0.0 ? s.main_ghz * s.main.ms : 0.0;
        t.clk_ms += s.main_ghz > 0.0 ? s.main.ms : 0.0;
    }
    if (s.exchange.timed) {
        st.exchange_ms += s.exchange.ms;
        st.exchanges += 1;
        // the part the interior did not hide: never more than the exchange itself.  On a short shard the
        // interior launch can end before the exchange's first event fires; that gap belongs to neither.
        st.exchange_exposed_ms += std::min(exposed_ms(s.exchange), s.exchange.ms);
    }
    if (s.boundary.timed) {
        st.boundary_ms += s.boundary.ms;
        st.boundary_launches += 1;
        st.pass_tail_ms += exposed_ms(s.boundary);
    }
}

// The clock the main launches held, weighted by their durations; 0.0: none of them has one.
inline double clock_ghz(const Totals& t) { return t.clk_ms > 0.0 ? t.clk_ms_ghz / t.clk_ms : 0.0; }

}  // namespace golprof
