// profile_probe -- the pass-timing accounting (csrc/gol_profile.h) from the
// command line, for tests/test_profile_model.py.  One case per line of
// standard input:
//   consts                     -> kClockSubSlots kClockSubWords kClockSlotWords
//   slot n (word value) x n    -> the clock (GHz) of a slot that is zero but for those words
//   pass main ms ghz gens  xchg ms tied after  bnd ms tied after
//                              -> nothing: one pass added to the totals (main, xchg, bnd, tied: 0 / 1)
//   totals                     -> kernel_ms launches generations exchange_ms exchanges boundary_ms
//                                 boundary_launches exchange_exposed_ms pass_tail_ms clock_ghz,
//                                 and the totals start again from nothing
// Built with a plain host compiler: gol_profile.h needs no HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../akka-game-of-life_amd/csrc/gol_profile.h"

int main() {
    char line[8192];
    golprof::Totals totals;
    while (fgets(line, sizeof line, stdin)) {
        int n = 0, used = 0, main_timed, tied[2], timed[2];
        unsigned gens;
        double ms[3], ghz, after[2];
        if (strncmp(line, "consts", 6) == 0) {
            printf("%d %d %d\n", golprof::kClockSubSlots, golprof::kClockSubWords, golprof::kClockSlotWords);
        } else if (sscanf(line, "slot %d%n", &n, &used) == 1) {
            std::vector<unsigned long long> words(golprof::kClockSlotWords, 0);
            const char* at = line + used;
            for (int k = 0; k < n; ++k) {
                int word = -1, step = 0;
                unsigned long long value;
                const bool ok = sscanf(at, "%d %llu%n", &word, &value, &step) == 2;
                if (!ok || word < 0 || word >= golprof::kClockSlotWords) {
                    fprintf(stderr, "profile_probe: bad slot word: %s", line);
                    return 2;
                }
                words[word] = value;
                at += step;
            }
            printf("%.17g\n", golprof::slot_clock_ghz(words.data()));
        } else if (sscanf(line, "pass %d %lf %lf %u %d %lf %d %lf %d %lf %d %lf", &main_timed, &ms[0], &ghz, &gens,
                          &timed[0], &ms[1], &tied[0], &after[0], &timed[1], &ms[2], &tied[1], &after[1]) == 12) {
            golprof::Sample s;
            s.main = golprof::Part{main_timed != 0, false, ms[0], 0.0};
            s.main_ghz = ghz;
            s.generations = gens;
            s.exchange = golprof::Part{timed[0] != 0, tied[0] != 0, ms[1], after[0]};
            s.boundary = golprof::Part{timed[1] != 0, tied[1] != 0, ms[2], after[1]};
            golprof::add(totals, s);
        } else if (strncmp(line, "totals", 6) == 0) {
            const gol_profile_stats& st = totals.stats;
            printf("%.17g %llu %llu %.17g %llu %.17g %llu %.17g %.17g %.17g\n", st.kernel_ms,
                   (unsigned long long)st.launches, (unsigned long long)st.generations, st.exchange_ms,
                   (unsigned long long)st.exchanges, st.boundary_ms, (unsigned long long)st.boundary_launches,
                   st.exchange_exposed_ms, st.pass_tail_ms, golprof::clock_ghz(totals));
            totals = golprof::Totals{};
        } else {
            fprintf(stderr, "profile_probe: bad case: %s", line);
            return 2;
        }
    }
    return 0;
}
