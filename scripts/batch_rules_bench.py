#!/usr/bin/env python3
"""What per-board rules on a batch (gol_rules_batch_*, GolBatch.set_rules;
DESIGN.md section 5k) cost next to the uniform batch, and what a rule sweep in
one launch saves (profiles/batch_rules.txt is this script's output).

    python scripts/batch_rules_bench.py [--reps R] [--gens G] [--out FILE]

One process; both sides of a comparison are warmed up first and alternate;
medians of --reps (default 5) whole calls, host side -- every timed call ends
synchronised.  The boards are re-seeded (untimed) before every timed call, so
every call steps the same soups from generation 0.  The uniform side runs the
kernels a batch without per-board rules runs, which are instruction for
instruction those of the build before per-board rules existed (section 5k).

(A) 16384 seeded 64 x 64 tori, --gens (default 1000) generations, every board
    given B36/S23 through set_rules, against GolBatch(rule="B36/S23") on the
    same boards: one board per wave, the rule's masks scalar.  Recorded.
(B) 65536 seeded 16 x 16 tori (4 boards per wave, the rule per lane), board i
    under a rule word derived from i, against the uniform generic step
    (B36/S23) of the same geometry.  Recorded.
(C) the gate: 256 rules x 64 boards of 64 x 64 torus.  One side is one batch
    with per-board rules; the yardstick is what there was before: 256 uniform
    GolBatch handles of 64 boards each, created once outside the timing, each
    stepped (and so synchronised) in a loop.  The one-launch side must be
    faster.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife.batch import GolBatch, rule_sweep_words  # noqa: E402
from gameoflife.rules import rule_from_word, rule_word  # noqa: E402

SEED = 0xBA7C4


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(ts):
    return f"{statistics.median(ts):10.3f} ms (min {min(ts):10.3f}, max {max(ts):10.3f})"


def main():
    argv = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--reps", "--gens"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            del argv[i:i + 2]
    reps = max(int(opts.get("--reps", 5)), 3)
    gens = int(opts.get("--gens", 1000))
    rows = []

    def say(s=""):
        print(s, flush=True)
        rows.append(s)

    def seeded_step(b):
        b.seed(SEED)
        return timed(lambda: b.step(gens))

    def compare(label, what, uniform, ruled):
        """Two batches of one geometry, alternated; the populations after the last call say both stepped soups."""
        seeded_step(uniform), seeded_step(ruled)  # warm-up
        t_u, t_r = [], []
        for _ in range(reps):
            t_u.append(seeded_step(uniform))
            t_r.append(seeded_step(ruled))
        fu, fr = statistics.median(t_u), statistics.median(t_r)
        say(f"{label} {what}, {gens} generations")
        say(f"    uniform batch               {med(t_u)}")
        say(f"    per-board rules             {med(t_r)}   {fr / fu:.3f} x the uniform batch")
        return uniform.populations(), ruled.populations()

    say(f"batch_rules_bench: whole calls of {gens} generations, host side, medians of {reps}; re-seeded (untimed) "
        f"before every timed call; every timed call ends synchronised; the sides alternate in one process")

    boards = 16384
    with GolBatch(boards, 64, 64, rule="B36/S23") as u, GolBatch(boards, 64, 64) as r:
        r.set_rules(["B36/S23"] * boards)
        pu, pr = compare("(A)", f"{boards} seeded 64 x 64 tori, every board B36/S23 (one board per wave: scalar masks)",
                         u, r)
        say(f"    the two sides end on the same boards: {bool(np.array_equal(pu, pr))}")

    boards = 65536
    i = np.arange(boards, dtype=np.uint64)
    words = ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(20)).astype(np.uint32) & np.uint32(0x01FF01FF)
    with GolBatch(boards, 16, 16, rule="B36/S23") as u, GolBatch(boards, 16, 16) as r:
        r.set_rules(words)
        compare("(B)", f"{boards} seeded 16 x 16 tori, board i under a word derived from i ({np.unique(words).size} "
                f"distinct rules; 4 boards per wave: masks per lane) against uniform B36/S23", u, r)

    nrules, per = 256, 64
    masks = [m << 1 for m in range(16)]  # births and survivals on 1 .. 4 neighbours: B3/S23 is among them
    sweep = rule_sweep_words(masks, masks)
    assert sweep.size == nrules and rule_word("life") in sweep.tolist()
    handles = [GolBatch(per, 64, 64, rule=rule_from_word(w)) for w in sweep]
    try:
        with GolBatch(nrules * per, 64, 64) as one:
            one.set_rules(np.repeat(sweep, per))

            def loop():
                for h in handles:
                    h.seed(SEED)
                return timed(lambda: [h.step(gens) for h in handles])

            loop(), seeded_step(one)  # warm-up
            t_loop, t_one = [], []
            for _ in range(reps):
                t_loop.append(loop())
                t_one.append(seeded_step(one))
            fl, fo = statistics.median(t_loop), statistics.median(t_one)
            say(f"(C) {nrules} rules x {per} boards of 64 x 64 torus, {gens} generations")
            say(f"    loop over {nrules} uniform batches {med(t_loop)}   ({fl / nrules:.4f} ms per batch)")
            say(f"    one batch, per-board rules  {med(t_one)}")
            say(f"    gate: the one launch faster than the loop ({fl / fo:.1f} x): {'met' if fo < fl else 'MISSED'}")
    finally:
        for h in handles:
            h.close()
    if opts.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
