"""CPU: the model of cycle detection (tests/cycle_model.py) -- the closed form
against the literal schedule, and the known answers of patterns whose preperiod
and period are textbook facts, so the GPU tests compare the kernel with a
checked reference."""
import numpy as np
import pytest

import batch_model as M
import cycle_model as C
from oracle import oracle as O


def test_closed_form_equals_the_literal_schedule():
    for mu in range(0, 71):
        for lam in range(1, 71):
            seen = C.seen_for(mu, lam)
            assert C.schedule_of(mu, lam, 400) == (lam, seen), (mu, lam)
            # nothing is seen a generation earlier
            assert C.schedule_of(mu, lam, seen - 1) == (0, 0), (mu, lam)


def test_snapshot_generation_is_the_schedule():
    want = {1: 0, 2: 1, 3: 1, 4: 3, 7: 3, 8: 7, 15: 7, 16: 15, 2**32 - 1: 2**31 - 1}
    for g, t in want.items():
        assert C.snapshot_generation(g) == t
    for g in range(1, 2000):
        t = C.snapshot_generation(g)
        assert t < g <= 2 * t + 1 and (t & (t + 1)) == 0


KNOWN = [
    # (name, cells, topology, rule, N, period, seen)
    ("dead", C.place(12, 12), "torus", O.LIFE, 8, 1, 1),
    ("block", C.place(12, 12, C.BLOCK), "torus", O.LIFE, 8, 1, 1),
    ("blinker", C.place(12, 12, C.BLINKER), "torus", O.LIFE, 8, 2, 3),
    ("pulsar", C.place(32, 32, C.PULSAR), "torus", O.LIFE, 10, 3, 6),
    ("pentadecathlon", C.place(32, 32, C.PENTADECATHLON), "torus", O.LIFE, 40, 15, 30),
    ("glider-8", C.place(8, 8, C.GLIDER), "torus", O.LIFE, 70, 32, 63),
    ("glider-64", C.place(64, 64, C.GLIDER), "torus", O.LIFE, 520, 256, 511),
]


@pytest.mark.parametrize("case", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_patterns(case):
    _, cells, topo, rule, N, period, seen = case
    assert C.cycle_of(cells, N, topo, rule) == (period, seen)
    # one generation short of seen nothing is reported
    assert C.cycle_of(cells, seen - 1, topo, rule) == (0, 0)
    # the period is a fact about the board: preperiod 0, so the closed form gives seen
    assert C.seen_for(0, period) == seen


def test_rules_that_freeze_a_soup():
    soups = M.unpack(M.seed_rows(6, 8, 8, 0xBA7C4), 8)
    for cells in soups:
        # ref-effective is the identity: every board is a still life at once
        assert C.cycle_of(cells, 4, "torus", O.REF_EFFECTIVE) == (1, 1)
    # B0/S012345678: nothing dies, and a dead cell is born only with no live neighbour -- fixed after one generation
    # (a 64 x 64 soup: at half density a dead cell without a live neighbour is rare, one in 2^10 cells)
    cells = M.unpack(M.seed_rows(1, 64, 64, 0xBA7C4), 64)[0]
    assert not np.array_equal(M.step_board(cells, "torus", (0x001, 0x1FF)), cells)
    assert C.cycle_of(cells, 4, "torus", (0x001, 0x1FF)) == (1, 2)
    assert C.seen_for(1, 1) == 2


def test_run_returns_the_final_boards_and_per_board_answers():
    rows = M.pack(np.stack([C.place(8, 8, C.GLIDER), C.place(8, 8, C.BLINKER), C.place(8, 8)]))
    final, period, seen = C.run(rows, 8, 40)
    assert period.tolist() == [0, 2, 1] and seen.tolist() == [0, 3, 1]
    assert np.array_equal(final, M.run(rows, 8, 40)[0])
    final, period, seen = C.run(rows, 8, 63)
    assert period.tolist() == [32, 2, 1] and seen.tolist() == [63, 3, 1]
