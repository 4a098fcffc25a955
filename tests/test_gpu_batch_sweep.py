"""GPU: the batch engine on every geometry its validator accepts (DESIGN.md
section 6, "The geometry sweeps"): 3844 tori and 16125 clipped boards, the
four visible-extent variants included, each bit-exact against the numpy models
of tests/batch_model.py, tests/batch_rules_model.py and tests/cycle_model.py.
tests/test_gpu_batch.py keeps the hand-picked shapes with their board counts,
chunk knobs and windows; this file varies the geometry alone.

One test is one height of one topology: every width and every visible-extent
variant of it, with k + 1 boards (k = 64 // H: one full wave and a last wave
of one board).  The cases, the counts the tests assert and the comparison come
from tests/sweep_cases.py, which tests/test_sweep_cases.py checks without a
device -- that the comparison notices a wrong mask or wrap bit among them."""
import pytest

import sweep_cases as S
from gameoflife.batch import GolBatch
from gameoflife.rules import Rule
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HEIGHTS = [("torus", H) for H in range(3, 65)] + [("ref-clipped", H) for H in range(1, 65)]


def _id(case):
    return f"{case[0]}-H{case[1]}"


def _uniform(b, W, H):
    """One step(6, populations, settled) call on the seeded boards, then the hashes and populations."""
    b.seed(S.batch_seed(W, H))
    pops, settled = b.step(S.SWEEP_GENS, populations=True, settled=True)
    assert b.epoch == S.SWEEP_GENS
    return {"final": b.snapshot(), "populations": pops, "settled": settled, "hashes": b.hashes(),
            "population": b.populations()}


@pytest.mark.parametrize("case", HEIGHTS, ids=_id)
def test_every_width_of_a_height(gpu, case):
    topology, H = case
    n, k = S.batch_boards(H), 64 // H
    ran = 0
    for geometry in S.batch_geometries(topology, H):
        W, _, vis = geometry
        # 1. the B3/S23 instance
        with GolBatch(n, W, H, topology=topology, rule="life", vis=vis) as b:
            g = b.geometry()
            assert g["boards_per_wave"] == k and g["waves"] == 2
            bad = S.mismatch(_uniform(b, W, H), S.expected_uniform(geometry, topology, O.LIFE))
            assert bad is None, (geometry, "B3/S23", bad)
            # 2. the RULES instance, on the same handle
            b.set_rules(S.batch_rule_words(W, H))
            b.seed(S.batch_seed(W, H))
            pops = b.step(S.SWEEP_GENS, populations=True)
            bad = S.mismatch({"final": b.snapshot(), "populations": pops}, S.expected_rules(geometry, topology))
            assert bad is None, (geometry, "per-board rules", bad)
        # 3. the uniform generic instance
        rule = S.uniform_rule(W, H)
        with GolBatch(n, W, H, topology=topology, rule=Rule(*rule), vis=vis) as b:
            bad = S.mismatch(_uniform(b, W, H), S.expected_uniform(geometry, topology, rule))
            assert bad is None, (geometry, rule, bad)
        ran += 1
    assert ran == S.batch_geometry_count(topology, H)


@pytest.mark.parametrize("case", HEIGHTS, ids=_id)
def test_longer_runs_of_a_height(gpu, case):
    """40 generations with settle words and 96 with cycle detection, at the
    smallest width, either side of the dword boundary, a wrap bit in the middle
    of the upper dword, and 64.  tests/test_sweep_cases.py asserts, on the
    model, that these boards include settled and unsettled ones, with and
    without a period."""
    topology, H = case
    n = S.batch_boards(H)
    ran = 0
    for geometry in S.long_run_geometries(topology, H):
        W, _, vis = geometry
        short, long = S.expected_long(geometry, topology)
        with GolBatch(n, W, H, topology=topology, rule="life", vis=vis) as b:
            b.seed(S.batch_seed(W, H))
            settled = b.step(S.SETTLE_GENS, settled=True)
            bad = S.mismatch({"final": b.snapshot(), "settled": settled}, short)
            assert bad is None, (geometry, "settle", bad)
            b.seed(S.batch_seed(W, H))
            period, seen = b.step_cycles(S.CYCLE_GENS)
            assert b.epoch == S.CYCLE_GENS
            bad = S.mismatch({"final": b.snapshot(), "period": period, "seen": seen}, long)
            assert bad is None, (geometry, "cycles", bad)
        ran += 1
    assert ran == S.long_run_count(topology, H)
