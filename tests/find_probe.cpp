// find_probe -- the pattern search's anchor-row arithmetic (csrc/gol_active.h
// anchor_rows, clip) from the command line, for tests/test_find_model.py.  One
// case per line of standard input, one line of results each; runs are printed
// as "lo hi lo hi ...":
//   anchors rows ph wrap_y n lo hi ...   -> the anchor rows with a pattern row in a run
//   clip lo hi n lo hi ...               -> the rows of the runs inside [lo, hi)
// Built with a plain host compiler: gol_active.h needs no HIP.
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
        Runs a;
        bool ok = true;
        if (op == "anchors") {
            int32_t rows;
            int ph, wrap;
            ok = (bool)(in >> rows >> ph >> wrap) && read_runs(in, a);
            if (ok) print_runs(golactive::anchor_rows(a, ph, rows, wrap != 0));
        } else if (op == "clip") {
            int64_t lo, hi;
            ok = (bool)(in >> lo >> hi) && read_runs(in, a);
            if (ok) print_runs(golactive::clip(a, lo, hi));
        } else {
            ok = false;
        }
        if (!ok) {
            fprintf(stderr, "find_probe: bad case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
