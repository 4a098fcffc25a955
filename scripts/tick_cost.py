#!/usr/bin/env python3
"""Per-call cost of gol_step(1) with and without the per-generation hash
(the reference's per-tick drive, BoardCreator.scala:113-116) on the default
7 x 7 board and on 4096^2.  --profile times the calls with kernel timing
enabled (gol_profile_enable): the record, the event pair and the clock-probe
slot of every launch (the calls of one board stay inside one window: no fold
falls into the timed loops).

    python scripts/tick_cost.py [--profile]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "akka-game-of-life_amd"))

from gameoflife.engine import GolEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--profile", action="store_true", help="time the calls with gol_profile_enable on")
    args = ap.parse_args()
    for W, H, topo in ((7, 7, "ref-clipped"), (4096, 4096, "torus")):
        with GolEngine(W, H, topology=topo, rule="life") as e:
            e.seed(1)
            e.profile(args.profile)
            for hashed in (False, True):
                e.step(50, hashes=hashed)
                e.sync()
                t0 = time.perf_counter()
                for _ in range(500):
                    e.step(1, hashes=hashed)
                e.sync()
                dt = time.perf_counter() - t0
                print(f"{W}x{H} {topo} step(1) hash={int(hashed)} profile={int(args.profile)}: "
                      f"{dt / 500 * 1e6:8.2f} us per call", flush=True)


if __name__ == "__main__":
    main()
