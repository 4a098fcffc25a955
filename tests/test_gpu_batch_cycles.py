"""GPU: cycle detection on a batch (gol_cycle_step, GolBatch.step_cycles;
DESIGN.md section 5g) against the numpy model of tests/cycle_model.py.  Every
case asserts three things per board: the final snapshot word for word against
the model's x_N, (period, seen) against the model's literal schedule, and the
epoch.

The model is computed once per (shape, rule, boards, N) and shared read-only.
The counts quoted in the comments (how many boards cycle, with which periods)
are facts about the seeded boards under the model; the tests assert them on
the model's answer, so a device that returned all zeros could not pass."""
import functools

import numpy as np
import pytest

import batch_model as M
import cycle_model as C
from gameoflife import _native as N_
from gameoflife.batch import GolBatch
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 0xBA7C4
RULES = {"life": O.LIFE, "ref-literal": O.REF_LITERAL, "ref-effective": O.REF_EFFECTIVE,
         "B0/S012345678": (0x001, 0x1FF), "B36/S23": (0x048, 0x00C)}

T64 = (64, 64, "torus", None)
T8 = (8, 8, "torus", None)
T57 = (5, 7, "torus", None)
# (shape (W, H, topology, vis), boards, N, mixed: some board must not cycle)
CASES = [
    (T64, 5, 4096, True),                              # one board per wave: 3 cycle (period 2), 2 do not
    ((64, 64, "ref-clipped", (64, 63)), 5, 4096, False),  # all period 2, seen up to 2049
    (T8, 33, 512, False),                              # k = 8 and a short last wave: periods {1, 2, 32, 132}
    ((8, 8, "ref-clipped", None), 33, 256, False),     # periods {1, 2, 3}
    (T57, 37, 256, False),                             # k = 9 with an idle lane: periods {1, 2, 56}
    ((33, 21, "torus", None), 13, 2048, False),        # permutes, a row across the dword boundary; seen = N twice
    ((20, 64, "torus", None), 5, 2048, True),          # the narrow rotate loop; 2 of 5 do not cycle
    ((64, 3, "torus", None), 85, 512, True),           # k = 21: 4 of 85 cycle, one with period 62
    ((3, 3, "torus", None), 85, 64, False),            # every board period 1, seen at most 4
]


def _id(case):
    (W, H, topo, vis), boards, N = case[:3]
    return f"{W}x{H}-{topo}" + (f"-vis{vis[0]}x{vis[1]}" if vis else "") + f"-{boards}b-{N}g"


@functools.lru_cache(maxsize=None)
def _model(shape, boards, N, rule_name="life"):
    """(x_N rows [boards][H], period [boards], seen [boards]) of the seeded boards; read-only."""
    W, H, topo, vis = shape
    out = C.run(M.seed_rows(boards, W, H, SEED), W, N, topo, RULES[rule_name], vis)
    for a in out:
        a.setflags(write=False)
    return out


def _batch(boards, shape, rule_name="life"):
    W, H, topo, vis = shape
    return GolBatch(boards, W, H, topology=topo, rule=rule_name, vis=vis)


def _check(b, want, N):
    """One step_cycles(N) call on the seeded batch against the model's answer."""
    final, period, seen = want
    b.seed(SEED)
    got_period, got_seen = b.step_cycles(N)
    assert np.array_equal(got_period, period), (got_period.tolist(), period.tolist())
    assert np.array_equal(got_seen, seen), (got_seen.tolist(), seen.tolist())
    assert np.array_equal(b.snapshot(), final)
    assert b.epoch == N
    stats = b.cycle_stats()
    assert stats["boards_cycled"] == int((period > 0).sum()) and stats["max_period"] == int(period.max())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cycles_match_model(gpu, case):
    shape, boards, N, mixed = case
    want = _model(shape, boards, N)
    assert (want[1] > 0).any()
    assert (want[1] == 0).any() == mixed
    with _batch(boards, shape) as b:
        _check(b, want, N)


def test_fixture_facts_of_the_seeded_boards():
    """What the cases above exercise, asserted on the model (no device)."""
    assert _model(T64, 5, 4096)[2].tolist() == [513, 1025, 1025, 0, 0]
    assert _model(T64, 5, 4096)[1].tolist() == [2, 2, 2, 0, 0]
    assert int(_model(CASES[1][0], 5, 4096)[2].max()) == 2049
    period, seen = _model(T8, 33, 512)[1:]
    assert sorted(set(period.tolist())) == [1, 2, 32, 132] and int(seen.max()) == 387
    # mixed periods inside one wave of 8 boards: the fast-forward runs with per-lane remainders
    assert any(len(set(period[w:w + 8].tolist())) > 1 for w in range(0, 32, 8))
    assert sorted(set(_model(T57, 37, 256)[1].tolist())) == [1, 2, 56]
    assert (_model((33, 21, "torus", None), 13, 2048)[2] == 2048).sum() == 2  # seen at the very last generation
    period = _model((64, 3, "torus", None), 85, 512)[1]
    assert int((period > 0).sum()) == 4 and 62 in period.tolist()
    period, seen = _model((3, 3, "torus", None), 85, 64)[1:]
    assert set(period.tolist()) == {1} and int(seen.max()) == 4


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 387, 388])
def test_call_lengths_around_a_snapshot_and_a_seen(gpu, N):
    """8 x 8 torus: N = 1, 2, 3 end before any cycle can be seen (the model says none is), 63 and 64 leave some
    boards without one, 387 is the largest seen and 388 one past it."""
    want = _model(T8, 33, N)
    assert (want[1] > 0).any() == (N >= 63)
    assert (want[1] == 0).any() == (N <= 64)
    with _batch(33, T8) as b:
        _check(b, want, N)


@pytest.mark.parametrize("rule_name", ["B36/S23", "ref-literal"])
@pytest.mark.parametrize("case", [(T8, 33, 512), (T57, 37, 256)], ids=_id)
def test_generic_mask_loop(gpu, case, rule_name):
    shape, boards, N = case
    want = _model(shape, boards, N, rule_name)
    assert (want[1] > 0).any()
    with _batch(boards, shape, rule_name) as b:
        _check(b, want, N)


@pytest.mark.parametrize("case", [(T8, 33, 512), (T64, 5, 4096)], ids=_id)
def test_chunk_knob_changes_nothing(gpu, case):
    shape, boards, N = case
    want = _model(shape, boards, N)
    with _batch(boards, shape) as b:
        for chunk in (1, 7, 100, 0):
            b.set_chunk(chunk)
            _check(b, want, N)


def test_known_patterns_loaded_by_hand(gpu):
    # (W, H, N, [(cells, period, seen)])
    batches = [
        (32, 32, 40, [(C.place(32, 32), 1, 1), (C.place(32, 32, C.BLOCK), 1, 1), (C.place(32, 32, C.BLINKER), 2, 3),
                      (C.place(32, 32, C.PULSAR), 3, 6), (C.place(32, 32, C.PENTADECATHLON), 15, 30)]),
        (8, 8, 70, [(C.place(8, 8, C.GLIDER), 32, 63), (C.place(8, 8), 1, 1), (C.place(8, 8, C.BLOCK), 1, 1),
                    (C.place(8, 8, C.BLINKER), 2, 3)]),
        (64, 64, 520, [(C.place(64, 64, C.GLIDER), 256, 511), (C.place(64, 64, C.PULSAR), 3, 6),
                       (C.place(64, 64, C.BLOCK), 1, 1)]),
    ]
    for W, H, N, boards in batches:
        rows = M.pack(np.stack([c for c, _, _ in boards]))
        final, period, seen = C.run(rows, W, N)
        assert period.tolist() == [p for _, p, _ in boards] and seen.tolist() == [s for _, _, s in boards]
        with GolBatch(len(boards), W, H) as b:
            b.load(rows)
            got_period, got_seen = b.step_cycles(N)
            assert got_period.tolist() == period.tolist() and got_seen.tolist() == seen.tolist(), (W, H)
            assert np.array_equal(b.snapshot(), final) and b.epoch == N


def test_rules_that_freeze_a_soup(gpu):
    # ref-effective is the identity: (1, 1) for any soup
    with _batch(33, T8, "ref-effective") as b:
        b.seed(SEED)
        start = b.snapshot()
        period, seen = b.step_cycles(5)
        assert period.tolist() == [1] * 33 and seen.tolist() == [1] * 33
        assert np.array_equal(b.snapshot(), start)
    # B0/S012345678 fixes a soup after one generation: (1, 2)
    want = _model(T64, 2, 6, "B0/S012345678")
    assert want[1].tolist() == [1, 1] and want[2].tolist()[0] == 2
    with _batch(2, T64, "B0/S012345678") as b:
        _check(b, want, 6)


def test_equals_the_plain_step_64x64(gpu):
    with _batch(9, T64) as a, _batch(9, T64) as b:
        a.seed(SEED)
        b.seed(SEED)
        a.step(3000)
        period, _ = b.step_cycles(3000)
        assert (period > 0).any()
        assert np.array_equal(a.snapshot(), b.snapshot())
        assert np.array_equal(a.hashes(), b.hashes())
        assert a.epoch == b.epoch == 3000


def test_equals_the_plain_step_and_stops_launching_8x8(gpu):
    N = 100_000
    seen_want = _model(T8, 33, 512)[2]
    with _batch(33, T8) as a, _batch(33, T8) as b:
        a.seed(SEED)
        b.seed(SEED)
        a.step(N)
        period, seen = b.step_cycles(N)
        assert np.array_equal(seen, seen_want) and np.array_equal(period, _model(T8, 33, 512)[1])
        assert np.array_equal(a.snapshot(), b.snapshot())
        assert np.array_equal(a.hashes(), b.hashes())
        assert a.epoch == b.epoch == N
        # the plain step takes N / 1024 = 98 launches; here the chunks up to the largest seen (387: one chunk of
        # 1024), after which every board has a period of at most 132 <= chunk + 1, and one launch for the remainder
        stats = b.cycle_stats()
        assert stats["launches"] <= -(-int(seen_want.max()) // 1024) + 1 == 2
        assert stats["boards_cycled"] == 33 and stats["max_period"] == 132


def test_a_second_call_starts_its_own_schedule(gpu):
    rows = M.seed_rows(33, 8, 8, SEED)
    mid, period1, seen1 = C.run(rows, 8, 100)
    final, period2, seen2 = C.run(mid, 8, 400)
    assert (period1 == 0).any() and (period2 > 0).all()
    with _batch(33, T8) as b:
        b.seed(SEED)
        got = b.step_cycles(100)
        assert np.array_equal(got[0], period1) and np.array_equal(got[1], seen1)
        got = b.step_cycles(400)
        assert np.array_equal(got[0], period2) and np.array_equal(got[1], seen2)
        assert np.array_equal(b.snapshot(), final) and b.epoch == 500


def test_mixing_with_settle_detection(gpu):
    """The snapshots live in the plane settle detection keeps: a settle call before and after a cycle call
    still returns the model's settled, and the cycle call its own answer."""
    W, H = 12, 10
    rows = M.seed_rows(64, W, H, SEED)
    x30, _, settled1 = M.run(rows, W, 30)
    x80, period, seen = C.run(x30, W, 50)
    x110, _, settled2 = M.run(x80, W, 30)
    assert (settled1 == 0).any() and (settled1 != 0).any() and (period > 0).any()
    with GolBatch(64, W, H) as b:
        for chunk in (0, 7):
            b.set_chunk(chunk)
            b.seed(SEED)
            assert np.array_equal(b.step(30, settled=True), settled1)
            got = b.step_cycles(50)
            assert np.array_equal(got[0], period) and np.array_equal(got[1], seen)
            assert np.array_equal(b.snapshot(), x80)
            assert np.array_equal(b.step(30, settled=True), settled2)
            assert np.array_equal(b.snapshot(), x110) and b.epoch == 110


def test_arguments(gpu):
    want = _model(T8, 33, 64)
    with _batch(33, T8) as b:
        b.seed(SEED)
        assert b.cycle_stats() == {"launches": 0, "boards_cycled": 0, "max_period": 0}
        period = np.full(33, 0xDEAD, dtype=np.uint32)
        # generations = 0: nothing written, nothing advanced
        assert N_.lib.gol_cycle_step(b._h, 0, period.ctypes.data_as(N_._u32p), None) == N_.GOL_OK
        assert (period == 0xDEAD).all() and b.epoch == 0
        # either array may be NULL
        assert N_.lib.gol_cycle_step(b._h, 64, None, None) == N_.GOL_OK
        assert np.array_equal(b.snapshot(), want[0]) and b.epoch == 64
        b.seed(SEED)
        assert N_.lib.gol_cycle_step(b._h, 64, None, period.ctypes.data_as(N_._u32p)) == N_.GOL_OK
        assert np.array_equal(period, want[2])
        assert b.cycle_stats()["launches"] == 1
