// active_probe -- active-row stepping's pure functions (csrc/gol_active.h)
// from the command line, for tests/test_active_model.py.  One case per line of
// standard input, one line of results each; runs are printed as "lo hi lo hi
// ...":
//   consts                                  -> kActiveBlock kMaxRuns kFirstBackoff kMaxBackoff
//   dilate rows G wrap_y n lo hi ...        -> the runs to step
//   normalize rows n lo hi ...              -> the runs as the invariant keeps them
//   subtract na lo hi ... nb lo hi ...      -> the rows of a that are not in b
//   bitmap rows lo_block n nwords w ...     -> the runs of the bitmap's set bits
//   due rows_now rows_at_last_scan          -> 0 / 1
//   dense rows_launched rows                -> 0 / 1
//   backoff b                               -> the wait after the next dense scan
// Built with a plain host compiler: gol_active.h needs no HIP.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../akka-game-of-life_amd/csrc/gol_active.h"

using golactive::Run;
using golactive::Runs;

static bool read_runs(std::istringstream& in, Runs& runs) {
    int n;
    if (!(in >> n) || n < 0) return false;
    runs.clear();
    for (int k = 0; k < n; ++k) {
        Run r;
        if (!(in >> r.lo >> r.hi)) return false;
        runs.push_back(r);
    }
    return true;
}

static void print_runs(const Runs& runs) {
    for (const Run& r : runs) printf("%d %d ", r.lo, r.hi);
    printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        Runs a, b;
        int32_t rows;
        bool ok = true;
        if (op == "consts") {
            printf("%d %d %d %d\n", golactive::kActiveBlock, golactive::kMaxRuns, golactive::kFirstBackoff,
                   golactive::kMaxBackoff);
        } else if (op == "dilate") {
            int G, wrap;
            ok = (bool)(in >> rows >> G >> wrap) && read_runs(in, a);
            if (ok) print_runs(golactive::dilate(a, G, rows, wrap != 0));
        } else if (op == "normalize") {
            ok = (bool)(in >> rows) && read_runs(in, a);
            if (ok) print_runs(golactive::normalize(a, rows));
        } else if (op == "subtract") {
            ok = read_runs(in, a) && read_runs(in, b);
            if (ok) print_runs(golactive::subtract(a, b));
        } else if (op == "bitmap") {
            int32_t lo_block, n;
            int nwords;
            ok = (bool)(in >> rows >> lo_block >> n >> nwords) && nwords >= 0 && (int64_t)n <= 32 * (int64_t)nwords;
            std::vector<uint32_t> bits;
            for (int k = 0; ok && k < nwords; ++k) {
                uint32_t w;
                ok = (bool)(in >> w);
                bits.push_back(w);
            }
            if (ok) print_runs(golactive::from_bitmap(bits.data(), lo_block, n, rows));
        } else if (op == "due") {
            int64_t now, last;
            ok = (bool)(in >> now >> last);
            if (ok) printf("%d\n", golactive::scan_due(now, last) ? 1 : 0);
        } else if (op == "dense") {
            int64_t launched, total;
            ok = (bool)(in >> launched >> total);
            if (ok) printf("%d\n", golactive::dense(launched, total) ? 1 : 0);
        } else if (op == "backoff") {
            int bo;
            ok = (bool)(in >> bo);
            if (ok) printf("%d\n", golactive::next_backoff(bo));
        } else {
            ok = false;
        }
        if (!ok) {
            fprintf(stderr, "active_probe: bad case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
