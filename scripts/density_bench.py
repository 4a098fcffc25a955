#!/usr/bin/env python3
"""What the density map costs on one torus context, next to the census
(profiles/density.txt is this script's output).

    python scripts/density_bench.py [W [H [REPS]]] [--big N] [--out FILE]

* gol_density over the whole board at T = 64, 256 and 4096 against gol_census,
  interleaved in one process, each call ending in its own synchronise: both
  read rows x wwords x 4 bytes once with the same popcounts; the density adds
  a per-tile reduction, atomics, the map's way to the host and the host's
  add into the caller's buffer, and drops the bounding box.  Median, min .. max, the GB/s over the plane's bytes, and the
  ratio of the medians (the goal: within 1.25 x of the census).
* one 1024 x 1024 window at T = 1 and T = 8 (the fine kernel: the map is as
  large as, or larger than, the cells it reads).
* --big N: one more line on an N x N board (default 262144, an 8 GiB plane;
  skipped when the context cannot be created).
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife import _native as N  # noqa: E402
from gameoflife import patterns  # noqa: E402
from gameoflife.engine import GolEngine  # noqa: E402

COPY_PEAK_TBS = 6.55  # README.md: measured device copy peak
TILES = (64, 256, 4096)
GOAL = 1.25
GUN = ("24bo11b$22bobo11b$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o14b$2o8bo3bob2o4bobo11b$"
       "10bo5bo7bo11b$11bo3bo20b$12b2o!")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def line(label, ts, nbytes=None):
    med, lo, hi = statistics.median(ts), min(ts), max(ts)
    s = f"{label:28s} n={len(ts):3d} median {med * 1e3:10.4f} ms   min {lo * 1e3:10.4f}   max {hi * 1e3:10.4f}"
    if nbytes:
        s += f"   {nbytes / med / 1e9:8.1f} GB/s ({nbytes / med / 1e12 / COPY_PEAK_TBS * 100:5.1f} % of the copy peak)"
    return s


def whole_board(e, say, reps, tiles=TILES):
    """Census and whole-board density at each tile, interleaved; returns the
    density / census ratios of the medians."""
    nbytes = e.rows * e.wwords * 4
    # the C call into a caller-owned map, zeroed outside the timed part (as gol_census fills a caller-owned struct)
    maps = {t: np.zeros((-(-e.height // t), -(-e.width // t)), dtype=np.uint32) for t in tiles}

    def density(t):
        e._density_into(0, 0, e.width, e.height, t.bit_length() - 1, maps[t])

    for _ in range(3):  # warm every call (and grow the density grid to its largest)
        e.census()
        for t in tiles:
            density(t)
    tc, td = [], {t: [] for t in tiles}
    for _ in range(reps):
        tc.append(timed(e.census))
        for t in tiles:
            maps[t].fill(0)
            td[t].append(timed(lambda: density(t)))
    say(line("gol_census (yardstick)", tc, nbytes))
    ratios = {}
    for t in tiles:
        say(line(f"gol_density T={t}", td[t], nbytes))
        ratios[t] = statistics.median(td[t]) / statistics.median(tc)
    say(f"{'density / census (medians)':28s} " + "   ".join(
        f"T={t}: {r:.3f} ({'within' if r <= GOAL else 'MISSES'} the {GOAL} goal)" for t, r in ratios.items())
        + f"   census spread (max - min) {(max(tc) - min(tc)) * 1e3:.4f} ms")
    return ratios


def main():
    argv = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--big"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            del argv[i:i + 2]
    W = int(argv[0]) if len(argv) > 0 else 65536
    H = int(argv[1]) if len(argv) > 1 else W
    reps = max(int(argv[2]) if len(argv) > 2 else 24, 20)
    big = int(opts.get("--big", 262144))
    rows = []

    def say(s=""):
        print(s, flush=True)
        rows.append(s)

    gun = patterns.parse_rle(GUN).cells
    seen = []  # per board: {tile: density / census}
    with GolEngine(W, H) as e:
        nbytes = e.rows * e.wwords * 4
        say(f"density_bench: {W} x {H} torus, one context, plane {nbytes / 2**20:.0f} MiB "
            f"(rows x wwords x 4 bytes), copy peak {COPY_PEAK_TBS} TB/s; times are whole calls, host side, "
            "each ending in a synchronise")
        say("note: up to 256 MiB of a plane can stay in the Infinity Cache between calls, so at planes of that order the GB/s are call rates over the plane's bytes, not pure HBM rates")
        say("maps: " + ", ".join(f"T={t}: {-(-W // t)} x {-(-H // t)} counts ({-(-W // t) * -(-H // t) * 4 / 2**10:.0f} KiB "
                                 "stored to the host and added)" for t in TILES))
        for label, prepare in [("one gun on an empty board", lambda: e.place(gun, W // 2, H // 2)),
                               ("seeded (dense) board", lambda: e.seed(0x5EED)),
                               ("stepped 64 generations", lambda: e.step(64))]:
            prepare()
            e.sync()
            c = e.census()
            say(f"-- {label}: population {c['population']}, bbox {c['bbox']}")
            seen.append(whole_board(e, say, reps))
            assert int(e.density(256).sum()) == c["population"]
        say("-- a 1024 x 1024 window (the fine kernel), against read_region of the same window")
        x, y = W // 2 - 500, H // 2 - 500
        for t in (1, 8):
            ts = [timed(lambda: e.density(t, x, y, 1024, 1024)) for _ in range(reps + 1)]
            say(line(f"gol_density T={t} 1024 x 1024", ts[1:]))
        buf = np.zeros((1024, 32), dtype=np.uint32)
        ts = [timed(lambda: e._read_region_into(x, y, 1024, 1024, buf)) for _ in range(reps + 1)]
        say(line("gol_read_region 1024 x 1024", ts[1:]))
    if big > 0:
        try:
            e = GolEngine(big, big)
        except N.GolError as ex:
            say(f"-- {big} x {big}: skipped, the context could not be created ({ex.message})")
        else:
            with e:
                say(f"-- {big} x {big} torus, plane {e.rows * e.wwords * 4 / 2**30:.0f} GiB, seeded")
                e.seed(0x5EED)
                e.sync()
                whole_board(e, say, 20, tiles=(256,))
    say(f"-- density / census over the three {W} x {H} boards: " + "   ".join(
        f"T={t}: {min(r[t] for r in seen):.3f} .. {max(r[t] for r in seen):.3f}" for t in TILES) + f"   (goal {GOAL})")
    say("reading: beyond the counting pass a map costs 4 bytes per tile -- stored through the host link, then added "
        "into the caller's buffer by the host -- against T x T / 8 bytes of plane read per tile: the finer the "
        "whole-board map, the more of the call is the map and not the pass")
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
