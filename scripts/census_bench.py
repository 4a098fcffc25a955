#!/usr/bin/env python3
"""What the census and the window calls cost on one torus context, next to
the calls they replace (profiles/census_region.txt is this script's output).

    python scripts/census_bench.py [W [H [REPS]]] [--out FILE]

* gol_census against gol_hash, alternating, each call ending in its own
  synchronise: both read rows x wwords x 4 bytes once, and the hash does more
  arithmetic per word, so it is the yardstick.  Median, min .. max and the
  GB/s each achieves, next to the README's measured 6.55 TB/s copy peak.
* place() of the 36 x 9 Gosper gun and read_region() of a 64 x 64 window,
  against gol_load and gol_snapshot of the whole board.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife import patterns  # noqa: E402
from gameoflife.engine import GolEngine  # noqa: E402

COPY_PEAK_TBS = 6.55  # README.md: measured device copy peak
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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    W = int(args[0]) if len(args) > 0 else 65536
    H = int(args[1]) if len(args) > 1 else W
    reps = max(int(args[2]) if len(args) > 2 else 24, 20)
    rows = []

    def say(s=""):
        print(s, flush=True)
        rows.append(s)

    gun = patterns.parse_rle(GUN).cells
    with GolEngine(W, H) as e:
        nbytes = e.rows * e.wwords * 4
        say(f"census_bench: {W} x {H} torus, one context, plane {nbytes / 2**20:.0f} MiB "
            f"(rows x wwords x 4 bytes), copy peak {COPY_PEAK_TBS} TB/s")
        say("note: up to 256 MiB of a plane can stay in the Infinity Cache between calls, so at planes of that order the GB/s are call rates over the plane's bytes, not pure HBM rates")
        # a new context is all dead: the sparse case first, then the dense ones
        for label, prepare in [("one gun on an empty board", lambda: e.place(gun, W // 2, H // 2)),
                               ("seeded (dense) board", lambda: e.seed(0x5EED)),
                               ("stepped 64 generations", lambda: e.step(64))]:
            prepare()
            e.sync()
            for _ in range(3):  # warm both calls
                e.census()
                e.hash()
            tc, th = [], []
            for _ in range(reps):  # alternating; each call synchronises before it returns
                tc.append(timed(e.census))
                th.append(timed(e.hash))
            c = e.census()
            say(f"-- {label}: population {c['population']}, bbox {c['bbox']}")
            say(line("gol_census", tc, nbytes))
            say(line("gol_hash (yardstick)", th, nbytes))
            say(f"{'census / hash (medians)':28s} {statistics.median(tc) / statistics.median(th):.3f}   "
                f"hash spread (max - min) {(max(th) - min(th)) * 1e3:.4f} ms, "
                f"census spread {(max(tc) - min(tc)) * 1e3:.4f} ms")
        say("-- windows against whole-board transfers")
        tp = [timed(lambda: e.place(gun, W // 2 + 100, H // 2 + 40 * k)) for k in range(1, reps + 1)]
        say(line("place 36 x 9 gun (or)", tp[1:]))
        tr = [timed(lambda: e.read_region(W // 2 - 16, H // 2 - 16, 64, 64)) for _ in range(reps + 1)]
        say(line("read_region 64 x 64", tr[1:]))
        ts_, tl = [], []
        buf = np.zeros((e.rows, e.wwords), dtype=np.uint32)
        for _ in range(3):
            ts_.append(timed(lambda: e.snapshot(buf)))
        for _ in range(3):
            tl.append(timed(lambda: e.load(buf)))
        say(line("gol_snapshot (pageable host)", ts_[1:], nbytes))
        say(line("gol_load (pageable host)", tl[1:], nbytes))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
