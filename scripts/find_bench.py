#!/usr/bin/env python3
"""What a pattern search (gol_find) costs next to a
census of the same board (profiles/find.txt is this script's output).

    python scripts/find_bench.py [--small N] [--big N] [--reps R] [--out FILE]

One process; every shape is warmed up first; find and census of one context
alternate; medians of --reps (default 5) whole calls, host side -- both calls
synchronise before they return.  Each row is a search with a census beside it:

(a) a bordered glider on a Gosper gun at the centre of a --big (default 262144)
    torus after 1200 generations, the live rows known (stepped with active
    rows): time proportional to rows_searched;
(b) the same board after a snapshot / load round trip: nothing known, every
    row searched -- on a board this sparse one read of the plane, as the
    census is (expected: no more than twice the census);
(c) a bordered glider on a seeded --small (default 65536) torus at epoch 2;
(d) the 38 x 11 bordered gun on the same board.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife import patterns  # noqa: E402
from gameoflife.engine import GolEngine  # noqa: E402

GUN = ("24bo11b$22bobo11b$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o14b$2o8bo3bob2o4bobo11b$"
       "10bo5bo7bo11b$11bo3bo20b$12b2o!")
# the phase half of a gun's gliders are in at generations that are multiples of 60 (the others: two steps on)
GLIDER = ["O.O", ".OO", ".O."]
GUN_GENS = 1200


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def row(e, label, pattern, reps, say):
    """Warm both calls, then alternate them; one line of the table."""
    found = e.find(pattern, border=1)
    census = e.census()
    t_find, t_census = [], []
    for _ in range(reps):
        t_find.append(timed(lambda: e.find(pattern, border=1))[0])
        t_census.append(timed(e.census)[0])
    f, c = statistics.median(t_find), statistics.median(t_census)
    say(f"{label:<58} find {f:9.3f} ms (min {min(t_find):9.3f}, max {max(t_find):9.3f})   census {c:8.3f} ms "
        f"(min {min(t_census):8.3f}, max {max(t_census):8.3f})   find / census {f / c:7.3f}   "
        f"count {found['count']}, rows_searched {found['rows_searched']} of {e.rows}, population {census['population']}")
    return f, c


def main():
    argv = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--big", "--small", "--reps"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            del argv[i:i + 2]
    small, big = int(opts.get("--small", 65536)), int(opts.get("--big", 262144))
    reps = max(int(opts.get("--reps", 5)), 3)
    rows = []

    def say(s=""):
        print(s, flush=True)
        rows.append(s)

    say(f"find_bench: gol_find and gol_census of one context alternated in one process; whole calls, host side, "
        f"medians of {reps}; both calls synchronise before they return")
    gun = patterns.parse_rle(GUN).cells
    if big > 0:
        with GolEngine(big, big, active_rows=True) as e:
            e.place(gun, big // 2, big // 2)
            e.step(GUN_GENS)
            e.sync()
            say(f"-- a Gosper gun at the centre of a {big} x {big} torus (plane {e.rows * e.wwords * 4 / 2**20:.0f} MiB) "
                f"at epoch {e.epoch}; active rows {e.active_rows()}")
            row(e, "(a) bordered glider, live rows known", GLIDER, reps, say)
            before = e.hash()
            board = e.snapshot()
            e.load(board)
            del board
            assert e.hash() == before and e.active_rows() is None
            f, c = row(e, "(b) bordered glider, after snapshot / load (rows unknown)", GLIDER, reps, say)
            say(f"(b) expectation: find <= 2 x census: {'met' if f <= 2 * c else 'MISSED'} ({f / c:.3f} x)")
    if small > 0:
        with GolEngine(small, small) as e:
            e.seed(0x5EED)
            e.step(2)
            e.sync()
            say(f"-- a seeded {small} x {small} torus (plane {e.rows * e.wwords * 4 / 2**20:.0f} MiB) at epoch {e.epoch}")
            row(e, "(c) bordered glider", GLIDER, reps, say)
            row(e, "(d) bordered Gosper gun (38 x 11)", gun, reps, say)
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
