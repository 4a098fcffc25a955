// schedule_probe -- the pass schedule's pure functions (csrc/gol_plan.h) from
// the command line, for tests/test_schedule_model.py.  One case per line of
// standard input, one line of results each:
//   band n lo0 hi0 lo1 hi1 strips gens resident band_rows present set frac div
//     -> row_lo0 row_hi0 band0 nbands0 row_lo1 row_hi1 band1 nbands1 waves grid small
//   pick band_rows rows strips gens resident -> the band before the small-board cut
//   xcd gens strips env_chunk        -> chunk
//   plan n cap fixed_depth hashed_row wide -> the depths
// Built with a plain host compiler: gol_plan.h needs no HIP.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../akka-game-of-life_amd/csrc/gol_plan.h"

constexpr int kWavesPerWG = 4;  // gol_kernels.h gol::kWavesPerWG

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int n, strips, gens, band_rows, present, set, div, env, cap, fixed, hashed, wide;
        int32_t lo[2], hi[2];
        int64_t resident;
        unsigned count;
        double frac;
        if (sscanf(line, "band %d %d %d %d %d %d %d %" SCNd64 " %d %d %d %lf %d", &n, &lo[0], &hi[0], &lo[1], &hi[1],
                   &strips, &gens, &resident, &band_rows, &present, &set, &frac, &div) == 13) {
            golplan::TailOverride tail;
            tail.present = present != 0;
            tail.set = set != 0;
            tail.frac = frac;
            tail.div = div;
            const golplan::BandPlan bp =
                golplan::band_plan(n, lo, hi, strips, gens, resident, band_rows, [&] { return tail; }, kWavesPerWG);
            printf("%d %d %d %d %d %d %d %d %" PRId64 " %d %d\n", bp.row_lo[0], bp.row_hi[0], bp.band[0], bp.nbands[0],
                   bp.row_lo[1], bp.row_hi[1], bp.band[1], bp.nbands[1], bp.waves, bp.grid, bp.small ? 1 : 0);
        } else if (sscanf(line, "pick %d %d %d %d %" SCNd64, &band_rows, &n, &strips, &gens, &resident) == 5) {
            printf("%d\n", golplan::pick_band(band_rows, n, strips, gens, resident));
        } else if (sscanf(line, "xcd %d %d %d", &gens, &strips, &env) == 3) {
            printf("%d\n", golplan::xcd_chunk(gens, strips, env, kWavesPerWG));
        } else if (sscanf(line, "plan %u %d %d %d %d", &count, &cap, &fixed, &hashed, &wide) == 5) {
            for (const int depth : golplan::plan_depths(count, cap, fixed, hashed != 0, wide != 0)) printf("%d ", depth);
            printf("\n");
        } else {
            fprintf(stderr, "schedule_probe: bad case: %s", line);
            return 2;
        }
    }
    return 0;
}
