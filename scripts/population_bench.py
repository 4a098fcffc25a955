#!/usr/bin/env python3
"""What a population series costs (gol_step_series, DESIGN.md section 5d;
profiles/population_series.txt is this script's output).

    python scripts/population_bench.py [--soup N] [--small N] [--gun N] [--reps R] [--out FILE]

One context per board in one process; the variants are stepped alternately,
round after round, from wherever the board stands; every shape is warmed up
first and every timed window ends in gol_sync.  Medians of --reps (5) windows,
ms per generation, of

* unhashed            step(n)
* hashed              step(n, hashes=True), timed twice per round (first and
                      last): hashed against hashed is the run-to-run spread
* population          step(n, populations=True)
* hash + population   step(n, hashes=True, populations=True)
* step(1) + census    one step(1) and one census() per point, the way without
                      the series (fewer points per window: it is slow)

on a seeded --soup (65536) square torus, 600 generations per window, a seeded
--small (4096) one, 1000 generations, and a Gosper gun at the centre of a
--gun (262144) one with active-row stepping, 1200 generations (0 skips a
board).  Decision rule of section 5d: the population-alone instances earn
their build time only if they beat their hashed siblings by more than the
hashed-against-hashed spread.
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


def window(e, gens, what):
    """One timed window of `gens` generations ending in gol_sync: (seconds,
    the last population the variant saw, or None)."""
    e.sync()
    last = None
    t0 = time.perf_counter()
    if what == "unhashed":
        e.step(gens)
    elif what.startswith("hashed"):
        e.step(gens, hashes=True)
    elif what == "population":
        last = int(e.step(gens, populations=True)[-1])
    elif what == "hash + population":
        last = int(e.step(gens, hashes=True, populations=True)[1][-1])
    else:
        for _ in range(gens):
            e.step(1)
            last = e.population()
    e.sync()
    return time.perf_counter() - t0, last


VARIANTS = ["hashed (first)", "unhashed", "population", "hash + population", "step(1) + census", "hashed (last)"]


def bench(e, title, gens, slow_gens, reps, say):
    say(f"-- {title}, {gens} generations per window ({slow_gens} for step(1) + census), passes "
        f"{sorted(set(e.pass_plan(min(gens, 1000), hashes=True)))} generations deep with a series, "
        f"{sorted(set(e.pass_plan(min(gens, 1000))))} without")
    n_of = {v: (slow_gens if v.startswith("step(1)") else gens) for v in VARIANTS}
    for v in VARIANTS:  # warm every shape: code objects, slots, census buffers
        window(e, n_of[v], v)
    ts = {v: [] for v in VARIANTS}
    for _ in range(reps):
        for v in VARIANTS:
            t, last = window(e, n_of[v], v)
            ts[v].append(t * 1e3 / n_of[v])
            if last is not None:
                assert last == e.population(), (v, last)
    med = {v: statistics.median(ts[v]) for v in VARIANTS}
    for v in VARIANTS:
        say(f"{v:20s} n={reps} median {med[v]:10.5f}   min {min(ts[v]):10.5f}   max {max(ts[v]):10.5f} ms/gen")
    both = ts["hashed (first)"] + ts["hashed (last)"]
    hashed = statistics.median(both)
    spread = (max(both) - min(both)) / hashed
    say(f"hashed against hashed: medians differ by "
        f"{abs(med['hashed (first)'] - med['hashed (last)']) / min(med['hashed (first)'], med['hashed (last)']) * 100:.2f}"
        f" %, all {2 * reps} windows span {spread * 100:.2f} % of their median ({hashed:.5f} ms/gen)")
    gain = 1.0 - med["population"] / hashed
    say(f"population alone is {gain * 100:+.2f} % faster than hashed: "
        f"{'MORE' if gain > spread else 'not more'} than the spread; hash + population costs "
        f"{(med['hash + population'] / hashed - 1.0) * 100:+.2f} % over hashed, "
        f"{(med['hash + population'] / med['unhashed'] - 1.0) * 100:+.2f} % over unhashed; "
        f"step(1) + census is {med['step(1) + census'] / med['population']:.1f} x population alone")
    say(f"epoch {e.epoch}, population {e.population()}")


def main():
    argv = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--soup", "--small", "--gun", "--reps"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            del argv[i:i + 2]
    soup, small, gun = int(opts.get("--soup", 65536)), int(opts.get("--small", 4096)), int(opts.get("--gun", 262144))
    reps = max(int(opts.get("--reps", 5)), 3)
    rows = []

    def say(s=""):
        print(s, flush=True)
        rows.append(s)

    say("population_bench: one context per board, the variants stepped alternately; whole calls, host side, every "
        "window ending in gol_sync")
    if soup > 0:
        with GolEngine(soup, soup) as e:
            e.seed(0x5EED)
            bench(e, f"a seeded {soup} x {soup} torus", 600, 60, reps, say)
    if small > 0:
        with GolEngine(small, small) as e:
            e.seed(0x5EED)
            bench(e, f"a seeded {small} x {small} torus", 1000, 200, reps, say)
    if gun > 0:
        try:
            e = GolEngine(gun, gun, active_rows=True)
        except N.GolError as ex:
            say(f"-- gun on {gun} x {gun}: skipped, the context could not be created ({ex.message})")
            e = None
        if e is not None:
            with e:
                e.place(patterns.parse_rle(GUN).cells, gun // 2, gun // 2)
                bench(e, f"a Gosper gun at the centre of a {gun} x {gun} torus, active rows on", 1200, 24, reps, say)
                st = e.active_stats()
                say(f"sparse passes {st['sparse_passes']} of {st['passes']}")
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
