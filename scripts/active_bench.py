#!/usr/bin/env python3
"""What active-row stepping (gol_set_active_rows) buys
and costs (profiles/active_rows.txt is this script's output).

    python scripts/active_bench.py [--small N] [--big N] [--reps R] [--out FILE]

Two contexts of the same board in one process, one with the mode on and one
with it off, stepped alternately from the same state; every shape is warmed up
first and every timed window ends in gol_sync.

* a Gosper gun at the centre of an N x N torus (--small, default 65536, and
  --big, default 262144; 0 skips one), 1200 generations per window, unhashed
  and hashed: ms per generation in both modes and the share of the board's
  rows the mode-on passes launched, rows_stepped / (passes x rows);
* a seeded --small board, 600 generations per window.  The mode-off context
  is timed twice per round, before and after the mode-on one: off against off
  is the run-to-run spread that mode on must stay within.  Once with the mode
  on since the board was seeded, and once with the mode-on context forgetting
  the board before every window (the mode switched off and on again, which
  also resets its scan backoff): what switching it on over a dense board
  costs.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife import _native as N  # noqa: E402
from gameoflife import patterns  # noqa: E402
from gameoflife.engine import GolEngine  # noqa: E402

GUN = ("24bo11b$22bobo11b$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o14b$2o8bo3bob2o4bobo11b$"
       "10bo5bo7bo11b$11bo3bo20b$12b2o!")
GUN_GENS = 1200
SOUP_GENS = 600


def window(e, gens, hashed):
    """One timed window: `gens` generations and a gol_sync; seconds."""
    e.sync()
    t0 = time.perf_counter()
    e.step(gens, hashes=hashed)
    e.sync()
    return time.perf_counter() - t0


def per_gen(ts, gens):
    ms = [t * 1e3 / gens for t in ts]
    return f"median {statistics.median(ms):9.5f}   min {min(ms):9.5f}   max {max(ms):9.5f} ms/gen"


def gun_board(n, reps, say):
    gun = patterns.parse_rle(GUN).cells
    try:
        on, off = GolEngine(n, n, active_rows=True), GolEngine(n, n)
    except N.GolError as ex:
        say(f"-- gun on {n} x {n}: skipped, the contexts could not be created ({ex.message})")
        return
    with on, off:
        for e in (on, off):
            e.place(gun, n // 2, n // 2)
        say(f"-- a Gosper gun at the centre of a {n} x {n} torus (plane {on.rows * on.wwords * 4 / 2**20:.0f} MiB), "
            f"{GUN_GENS} generations per window, passes {sorted(set(on.pass_plan(1000)))} generations deep")
        for hashed in (False, True):
            for e in (on, off):  # warm the shape: kernels, hash slots, the scan's bitmap
                window(e, GUN_GENS, hashed)
            on.active_stats(reset=True)
            t_on, t_off = [], []
            for _ in range(reps):
                t_on.append(window(on, GUN_GENS, hashed))
                t_off.append(window(off, GUN_GENS, hashed))
            st = on.active_stats()
            assert on.hash() == off.hash() and on.epoch == off.epoch
            what = "hashed  " if hashed else "unhashed"
            say(f"{what} mode on   n={reps} {per_gen(t_on, GUN_GENS)}")
            say(f"{what} mode off  n={reps} {per_gen(t_off, GUN_GENS)}")
            say(f"{what} off / on (medians) {statistics.median(t_off) / statistics.median(t_on):8.1f} x   "
                f"rows_stepped / (passes x rows) = {st['rows_stepped']} / ({st['passes']} x {n}) = "
                f"{st['rows_stepped'] / (st['passes'] * n):.6f}   sparse passes {st['sparse_passes']} of {st['passes']}, "
                f"scans {st['scans']} ({st['rows_scanned']} rows), rows cleared {st['rows_cleared']}")
        c = on.census()
        say(f"epoch {on.epoch}: population {c['population']}, bbox {c['bbox']}, active rows {on.active_rows()}")


def soup_windows(on, off, reps, fresh):
    t_on, t_a, t_b = [], [], []
    for _ in range(reps):
        t_a.append(window(off, SOUP_GENS, False))
        if fresh:  # forget the board and the scan backoff
            on.set_active_rows(False)
            on.set_active_rows(True)
        t_on.append(window(on, SOUP_GENS, False))
        t_b.append(window(off, SOUP_GENS, False))
    return t_on, t_a, t_b


def soup_board(n, reps, say):
    with GolEngine(n, n, active_rows=True) as on, GolEngine(n, n) as off:
        for e in (on, off):
            e.seed(0x5EED)
        say(f"-- a seeded {n} x {n} torus, {SOUP_GENS} generations per window, unhashed; the mode-off context is timed "
            "before and after the mode-on one in every round")
        for e in (on, off):
            window(e, SOUP_GENS, False)
        for fresh in (False, True):
            on.active_stats(reset=True)
            t_on, t_a, t_b = soup_windows(on, off, reps, fresh)
            st = on.active_stats()
            say("the mode-on context forgets the board and its scan backoff before every window (the cost of switching "
                "the mode on over a dense board):" if fresh else
                "mode on since the board was seeded (one warm-up window before these):")
            say(f"mode off (before) n={reps} {per_gen(t_a, SOUP_GENS)}")
            say(f"mode on           n={reps} {per_gen(t_on, SOUP_GENS)}")
            say(f"mode off (after)  n={reps} {per_gen(t_b, SOUP_GENS)}")
            m_a, m_b = statistics.median(t_a), statistics.median(t_b)
            both = t_a + t_b
            spread = (max(both) - min(both)) / statistics.median(both)
            excess = statistics.median(t_on) / statistics.median(both) - 1.0
            say(f"off against off: medians differ by {abs(m_a - m_b) / min(m_a, m_b) * 100:.2f} %, all {2 * reps} "
                f"windows span {spread * 100:.2f} % of their median; mode on is {excess * 100:+.2f} % against the "
                f"median of the off windows: {'within' if excess <= spread else 'OUTSIDE'} the spread   "
                f"(scans {st['scans']} in {st['passes']} passes, sparse passes {st['sparse_passes']}, "
                f"rows_stepped / (passes x rows) = {st['rows_stepped'] / (st['passes'] * n):.3f})")


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

    say("active_bench: mode on and mode off contexts of one board in one process, stepped alternately; whole calls, "
        "host side, every window ending in gol_sync")
    for n in (small, big):
        if n > 0:
            gun_board(n, reps, say)
    if small > 0:
        soup_board(small, reps, say)
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
