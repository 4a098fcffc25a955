#!/usr/bin/env python3
"""What cutting a batch's boards into objects on the device (gol_objects_batch,
DESIGN.md section 5i) costs next to what a caller had before it: snapshot() of
every board and labelling on the host (profiles/batch_objects.txt is this
script's output).

    python scripts/batch_objects_bench.py [--boards N] [--reps R] [--out FILE]

One process; both sides warmed up first; the two sides alternate; medians of
--reps (default 5) whole calls, host side -- every timed call ends
synchronised.

(a) --boards (default 16384) seeded 64 x 64 torus soups after
    step_cycles(65536); reach 1, max_objects 128 (raised to the next power of
    two that holds the largest count, and said so, if that exceeds 128).
    Device: one objects call.  Yardstick: snapshot() of all boards plus
    labelling alone (no boxes, no hashes) with the fastest labeller here:
    scipy.ndimage.label with 8-connectivity and the torus seams stitched by a
    union-find over the labels that face each other across them, if scipy is
    installed, else patterns.label_objects.  The gate, fixed before measuring:
    the device call's slowest run is faster than the yardstick's fastest, and
    both sides give the same count for every board.
(b) recorded, not gated: snapshot() alone, the call with max_objects = 1 (the
    counts alone), find of four patterns, reach 2, step(1000) of the same
    boards, and the raw soups (one object of about 2000 cells per board: long
    fills).
(c) where a call's time goes: (a)'s call through the C ABI into arrays that
    are kept, against GolBatch.objects' fresh arrays and find's match planes
    of the same size; then the call with max_objects = 1024 (256 MiB of
    records cross to the host), and the three again after it.
"""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife import _native as N  # noqa: E402
from gameoflife import patterns as P  # noqa: E402
from gameoflife.batch import OBJECT_DTYPE, GolBatch, tally, unpack_rows  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

SEED = 0x5EED
OBJECTS = {"block": ["OO", "OO"], "beehive": [".OO.", "O..O", ".OO."], "blinker -": ["OOO"], "blinker |": ["O", "O", "O"]}
EIGHT = np.ones((3, 3), dtype=np.int32)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(ts):
    return f"{statistics.median(ts):10.3f} ms (min {min(ts):10.3f}, max {max(ts):10.3f})"


def torus_count(cells):
    """Objects (8-connectivity) of one uint8 [H][W] torus board: scipy's plain labels, those that touch across a
    seam joined."""
    lab, n = ndimage.label(cells, structure=EIGHT)
    if n < 2:
        return n
    parent = list(range(n + 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    H, W = lab.shape
    for near, far in ((lab[0], lab[H - 1]), (lab[:, 0], lab[:, W - 1])):
        for d in (-1, 0, 1):
            a, c = near, np.roll(far, d)
            both = (a > 0) & (c > 0)
            for p, q in set(zip(a[both].tolist(), c[both].tolist())):
                rp, rq = find(p), find(q)
                if rp != rq:
                    parent[rp] = rq
                    n -= 1
    return n


def host_counts(rows, width):
    """uint32 [boards]: the objects (reach 1) of every torus board, labelled on the host."""
    cells = unpack_rows(rows, width)
    if ndimage is not None:
        return np.fromiter((torus_count(c) for c in cells), dtype=np.uint32, count=len(cells))
    return np.fromiter((len(P.label_objects(c)) for c in cells), dtype=np.uint32, count=len(cells))


def main():
    argv = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--boards", "--reps"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            del argv[i:i + 2]
    boards = int(opts.get("--boards", 16384))
    reps = max(int(opts.get("--reps", 5)), 3)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    labeller = "scipy.ndimage.label + seam union-find" if ndimage is not None else "patterns.label_objects"
    say(f"batch_objects_bench: whole calls, host side, medians of {reps}; every timed call ends synchronised; the two "
        f"sides of a comparison alternate in one process")
    with GolBatch(boards, 64, 64) as b:
        b.seed(SEED)
        period, _ = b.step_cycles(65536)
        most = int(b.objects(reach=1, max_objects=1)[0].max())
        room = 128
        while room < most:
            room *= 2

        def device():
            return b.objects(reach=1, max_objects=room)

        def host():
            return host_counts(b.snapshot(), 64)

        (got, objs), want = device(), host()
        same = bool(np.array_equal(got, want))
        t_dev, t_host, t_snap = [], [], []
        for _ in range(reps):
            t_dev.append(timed(device))
            t_host.append(timed(host))
            t_snap.append(timed(b.snapshot))
        d, h = statistics.median(t_dev), statistics.median(t_host)
        table = P.object_table({"block": [OBJECTS["block"]], "beehive": [OBJECTS["beehive"]],
                                "blinker": [OBJECTS["blinker -"], OBJECTS["blinker |"]]})
        census = tally(got, objs, table)
        say(f"(a) {boards} boards of 64 x 64 torus after step_cycles(65536) ({int((period > 0).sum())} on a cycle); "
            f"reach 1, max_objects {room}" + (" (raised from 128: see the largest count)" if room > 128 else ""))
        say(f"    objects in all {int(got.sum())}, largest count of a board {most}, boards truncated "
            f"{b.objects_stats()['boards_truncated']}; census {census}")
        say(f"    device objects              {med(t_dev)}   {boards * room * 16 / 2**20:.0f} MiB of records cross to "
            f"the host")
        say(f"    snapshot + host labelling   {med(t_host)}   ({labeller}; labelling alone, no boxes or hashes)")
        say(f"    snapshot alone              {med(t_snap)}")
        met = same and max(t_dev) < min(t_host)
        say(f"    gate: the device call's slowest run faster than the yardstick's fastest, and equal counts board by "
            f"board ({same}): {'met' if met else 'MISSED'} (max device {max(t_dev):.3f} ms, min host {min(t_host):.3f} "
            f"ms; host / device {h / d:.0f} x)")

        def rest(name, fn, note=""):
            fn()
            ts = [timed(fn) for _ in range(reps)]
            say(f"    {name:<28}{med(ts)}   {statistics.median(ts) / d:.2f} x (a)'s device call{note}")

        say("(b) recorded, not gated")
        rest("max_objects = 1", lambda: b.objects(reach=1, max_objects=1),
             " (the counts alone: the call without the records' copy)")
        rest("find, four patterns", lambda: b.find(list(OBJECTS.values()), border=1))
        rest("reach 2", lambda: b.objects(reach=2, max_objects=room))
        rest("step(1000), same boards", lambda: b.step(1000))
        b.seed(SEED)
        raw_counts = b.objects(reach=1, max_objects=room)[0]
        rest("raw soups, reach 1", lambda: b.objects(reach=1, max_objects=room),
             f" (largest count {int(raw_counts.max())})")
        rest("raw soups, max_objects = 1", lambda: b.objects(reach=1, max_objects=1))
        # (c) where the time of a call goes: the same call through the C ABI into arrays that are kept, so that no
        # fresh pages are touched; and what a process's allocator makes of 32 MiB arrays once 256 MiB ones were freed
        b.step_cycles(65536)
        counts = np.zeros(boards, dtype=np.uint32)
        kept = np.zeros((boards, room), dtype=OBJECT_DTYPE)
        cp, op = counts.ctypes.data_as(N._u32p), kept.ctypes.data_as(ctypes.POINTER(N.GolBatchObject))

        def raw():
            N.check_batch(N.lib.gol_objects_batch(b._h, 0, boards, 1, room, cp, counts.size, op, kept.size), b._h)

        def planes():
            return b.find(list(OBJECTS.values()), border=1, matches=True)

        say(f"(c) the ash again; max_objects {room} into arrays that are kept (the C call), into fresh arrays "
            f"(GolBatch.objects), and find's 32 MiB of match planes into fresh arrays")
        rest("kept arrays", raw)
        rest("fresh arrays", device)
        rest("find, matches=True", planes)
        rest("max_objects = 1024", lambda: b.objects(reach=1, max_objects=1024),
             f" ({boards * 1024 * 16 / 2**20:.0f} MiB of records, fresh arrays)")
        say("    after it (the process has freed arrays of 256 MiB):")
        rest("kept arrays", raw)
        rest("fresh arrays", device)
        rest("find, matches=True", planes)
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
