#!/usr/bin/env python3
"""What a batch of small boards (gol_batch_*) costs next
to the same boards as one context each (profiles/batch.txt is this script's
output).

    python scripts/batch_bench.py [--loop N] [--boards N] [--copies N] [--reps R] [--out FILE]

One process; every shape is warmed up first; where two sides are compared they
alternate; medians of --reps (default 5) whole calls, host side -- every timed
call ends synchronised.  The yardstick is a GolEngine context per board, each
stepped with an unhashed step(n) and a sync.

(a) --loop (default 256) boards of 64 x 64 torus, B3/S23, 1000 generations:
    one batch call against the loop over that many engines (the gate: the
    batch must be faster);
(b) --boards (default 16384) such boards: the batch alone, ns per
    board-generation, cell updates per second, time per launch;
(c) --copies (default 65536) copies of the reference's 8 x 8 clipped board,
    100 generations: the batch against one engine of that board, timed and
    multiplied;
(d) (b) with populations=True and with settled=True: their cost over the
    plain step.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife.batch import GolBatch  # noqa: E402
from gameoflife.engine import GolEngine  # noqa: E402

SEED = 0x5EED
AUTO_CHUNK = 1024  # gol_batch_set_chunk(0)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(ts):
    return f"{statistics.median(ts):10.3f} ms (min {min(ts):10.3f}, max {max(ts):10.3f})"


def main():
    argv = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--loop", "--boards", "--copies", "--reps"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            del argv[i:i + 2]
    n_loop, n_big = int(opts.get("--loop", 256)), int(opts.get("--boards", 16384))
    n_copies = int(opts.get("--copies", 65536))
    reps = max(int(opts.get("--reps", 5)), 3)
    rows = []

    def say(s=""):
        print(s, flush=True)
        rows.append(s)

    say(f"batch_bench: whole calls, host side, medians of {reps}; every timed call ends synchronised; the two sides "
        f"of a comparison alternate in one process")
    gens = 1000
    if n_loop > 0:
        engines = [GolEngine(64, 64) for _ in range(n_loop)]
        try:
            for i, e in enumerate(engines):
                e.seed(SEED + i)

            def loop():
                for e in engines:
                    e.step(gens)
                    e.sync()

            with GolBatch(n_loop, 64, 64) as b:
                b.seed(SEED)
                b.step(gens)
                loop()
                t_batch, t_loop = [], []
                for _ in range(reps):
                    t_batch.append(timed(lambda: b.step(gens)))
                    t_loop.append(timed(loop))
            fb, fl = statistics.median(t_batch), statistics.median(t_loop)
            say(f"(a) {n_loop} boards of 64 x 64 torus, B3/S23, {gens} generations")
            say(f"    batch, one call             {med(t_batch)}")
            say(f"    loop over {n_loop} engines       {med(t_loop)}   ({fl / n_loop:.3f} ms per engine)")
            say(f"    gate: batch faster than the loop: {'met' if fb < fl else 'MISSED'} (loop / batch {fl / fb:.1f} x)")
        finally:
            for e in engines:
                e.close()
    if n_big > 0:
        with GolBatch(n_big, 64, 64) as b:
            b.seed(SEED)
            b.step(gens)
            b.step(gens, populations=True)
            b.step(gens, settled=True)
            t_plain, t_pop, t_settle = [], [], []
            for _ in range(reps):
                t_plain.append(timed(lambda: b.step(gens)))
                t_pop.append(timed(lambda: b.step(gens, populations=True)))
                t_settle.append(timed(lambda: b.step(gens, settled=True)))
            p = statistics.median(t_plain)
            launches = -(-gens // AUTO_CHUNK)
            say(f"(b) {n_big} boards of 64 x 64 torus, B3/S23, {gens} generations, batch alone "
                f"({b.geometry()['waves']} waves)")
            say(f"    plain step                  {med(t_plain)}   {p * 1e6 / (n_big * gens):.4f} ns per "
                f"board-generation, {n_big * gens * 4096 / (p * 1e-3):.3e} cell updates / s, "
                f"{launches} launch(es) of {p / launches:.3f} ms at the automatic chunk of {AUTO_CHUNK}")
            say(f"(d) populations=True            {med(t_pop)}   {statistics.median(t_pop) / p:.2f} x the plain step "
                f"(the [boards][generations] series, {n_big * gens * 4 / 2**20:.0f} MiB, crosses to the host)")
            say(f"    settled=True                {med(t_settle)}   {statistics.median(t_settle) / p:.2f} x the plain step")
    if n_copies > 0:
        cgens = 100
        with GolEngine(8, 8, topology="ref-clipped") as e, GolBatch(n_copies, 8, 8, topology="ref-clipped") as b:
            e.seed(SEED)
            b.seed(SEED)

            def one():
                e.step(cgens)
                e.sync()

            one()
            b.step(cgens)
            t_batch, t_one = [], []
            for _ in range(reps):
                t_batch.append(timed(lambda: b.step(cgens)))
                t_one.append(timed(one))
            fb, fo = statistics.median(t_batch), statistics.median(t_one)
            say(f"(c) {n_copies} copies of the reference's 8 x 8 clipped board, B3/S23, {cgens} generations")
            say(f"    batch, one call             {med(t_batch)}   {fb * 1e6 / (n_copies * cgens):.4f} ns per board-generation")
            say(f"    one engine of that board    {med(t_one)}   x {n_copies} = {fo * n_copies:.0f} ms "
                f"(engine x copies / batch {fo * n_copies / fb:.0f} x)")
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
