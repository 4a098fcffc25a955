#!/usr/bin/env python3
"""What a census of a batch's objects kept on the device (gol_census_batch_*,
DESIGN.md section 5j) costs next to what a caller had before it:
GolBatch.objects -- the records cross to the host -- followed by batch.tally
(profiles/batch_census.txt is this script's output).

    python scripts/batch_census_bench.py [--boards N] [--reps R] [--out FILE]
    python scripts/batch_census_bench.py --tally-only [--boards N] [--reps R]
    python scripts/batch_census_bench.py --adds K [--boards N]

One process; both sides warmed up first; the two sides alternate; medians of
--reps (default 5) whole calls, host side -- every timed call ends
synchronised.

(a) --boards (default 16384) seeded 64 x 64 torus soups after
    step_cycles(65536); reach 1, max_objects 128.  Yardstick: objects(128)
    followed by tally -- run first, before this process has freed any array of
    32 MiB or more but its own.  Device: census_add followed by census_read,
    into a table emptied (census_begin, not timed) before every run, so that
    every key is inserted anew.  The gate, fixed before measuring: the device
    side's slowest run is faster than the yardstick's fastest, and
    census_names gives tally's names and totals.
(b) recorded, not gated: census_begin + census_add + census_read, census_add
    alone on a table that has the keys (the second and later reseeds of a
    search), census_read alone, census_begin alone, objects(128) alone and
    with max_objects = 1 (the objects launch without the records' copy), and
    one key under the highest contention: --boards boards tiled with blocks at
    pitch 3 (441 per board), max_objects 512, every record the same key.
--tally-only: (b)'s census_add lines alone -- what is run a second time against
    a build of the library without the wave aggregation
    (-DGOL_CENSUS_NO_AGGREGATE, GOL_LIB_PATH; built for this measurement only).
--adds K: no timing; the ash, census_begin and K census_add calls, for a
    kernel trace of the tally kernel alone.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife import patterns as P  # noqa: E402
from gameoflife.batch import GolBatch, census_names, pack_rows, tally  # noqa: E402

SEED = 0x5EED
OBJECTS = {"block": ["OO", "OO"], "beehive": [".OO.", "O..O", ".OO."], "blinker -": ["OOO"], "blinker |": ["O", "O", "O"]}
MAX_KEYS = 65536


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(ts):
    return f"{statistics.median(ts):10.3f} ms (min {min(ts):10.3f}, max {max(ts):10.3f})"


def blocks_board():
    cells = np.zeros((1, 64, 64), dtype=np.uint8)
    for y in range(0, 63, 3):
        for x in range(0, 63, 3):
            cells[0, y:y + 2, x:x + 2] = 1
    return pack_rows(cells)


def main():
    argv = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--boards", "--reps", "--adds"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            del argv[i:i + 2]
    tally_only = "--tally-only" in argv
    boards = int(opts.get("--boards", 16384))
    reps = max(int(opts.get("--reps", 5)), 3)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    table = P.object_table({"block": [OBJECTS["block"]], "beehive": [OBJECTS["beehive"]],
                            "blinker": [OBJECTS["blinker -"], OBJECTS["blinker |"]]})
    met = True
    with GolBatch(boards, 64, 64) as b:
        b.seed(SEED)
        period, _ = b.step_cycles(65536)

        if "--adds" in opts:
            b.census_begin(MAX_KEYS)
            for _ in range(int(opts["--adds"])):
                b.census_add(reach=1, max_objects=128)
            print(f"{opts['--adds']} census_add calls: {b.census_stats()}")
            return 0

        def yardstick():
            counts, objs = b.objects(reach=1, max_objects=128)
            return tally(counts, objs, table)

        def device():
            b.census_add(reach=1, max_objects=128)
            return b.census_read()

        def rest(name, fn, before=None, note=""):
            if before:
                before()
            fn()
            ts = []
            for _ in range(reps):
                if before:
                    before()
                ts.append(timed(fn))
            say(f"    {name:<44}{med(ts)}{note}")
            return statistics.median(ts)

        def begin():
            b.census_begin(MAX_KEYS)

        if not tally_only:
            say(f"batch_census_bench: whole calls, host side, medians of {reps}; every timed call ends synchronised; the "
                f"two sides of a comparison alternate in one process")
            want = yardstick()
            begin()
            entries = device()
            got, stats = census_names(entries, table), b.census_stats()
            same = got == want and sum(got.values()) == sum(want.values()) == stats["tallied"] == stats["seen"]
            t_dev, t_host = [], []
            for _ in range(reps):
                t_host.append(timed(yardstick))
                begin()
                t_dev.append(timed(device))
            d, h = statistics.median(t_dev), statistics.median(t_host)
            say(f"(a) {boards} boards of 64 x 64 torus after step_cycles(65536) ({int((period > 0).sum())} on a cycle); "
                f"reach 1, max_objects 128, max_keys {MAX_KEYS}")
            say(f"    census {got}")
            say(f"    {stats}; the largest count {int(entries['count'][0])}, keys seen once "
                f"{int((entries['count'] == 1).sum())}; {len(entries) * 32 / 1024:.0f} KiB of entries cross to the host")
            say(f"    {'census_add + census_read (emptied table)':<44}{med(t_dev)}")
            say(f"    {'objects(128) + tally':<44}{med(t_host)}   {boards * 128 * 16 / 2**20:.0f} MiB of records cross "
                f"to the host, then np.unique")
            met = same and max(t_dev) < min(t_host)
            say(f"    gate: the device side's slowest run faster than the yardstick's fastest, and the same names and "
                f"totals ({same}): {'met' if met else 'MISSED'} (max device {max(t_dev):.3f} ms, min yardstick "
                f"{min(t_host):.3f} ms; yardstick / device {h / d:.0f} x)")
            say("(b) recorded, not gated")
            rest("census_begin + census_add + census_read", lambda: (begin(), device()))
        else:
            say(f"tally only ({os.environ.get('GOL_LIB_PATH') or 'the tree build'}); {boards} boards, medians of {reps}")
        rest("census_add, emptied table", lambda: b.census_add(reach=1, max_objects=128), before=begin)
        begin()
        rest("census_add, the keys in the table", lambda: b.census_add(reach=1, max_objects=128))
        if not tally_only:
            rest("census_read alone", b.census_read, note=f"   {b.census_stats()['distinct']} keys")
            rest("census_begin alone", begin, note=f"   {2 * MAX_KEYS * 32 / 2**20:.0f} MiB table")
            begin()
            rest("objects(128) alone", lambda: b.objects(reach=1, max_objects=128))
            rest("objects(1) alone", lambda: b.objects(reach=1, max_objects=1),
                 note="   the objects launch without the records' copy")
        # one key, the highest contention
        b.load(np.repeat(blocks_board(), boards, axis=0))
        begin()
        rest("one key: census_add(max_objects=512)", lambda: b.census_add(reach=1, max_objects=512),
             note=f"   {boards * 441} blocks, {boards * 512 // 64} waves, one atomic add each to one slot")
        s = b.census_stats()
        e = b.census_read()
        assert len(e) == 1 and int(e[0]["count"]) == s["tallied"] == s["calls"] * boards * 441, (s, e)
        if not tally_only:
            rest("one key: objects(1) alone", lambda: b.objects(reach=1, max_objects=1))
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
