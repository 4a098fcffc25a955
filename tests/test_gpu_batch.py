"""GPU: the batch engine (gol_batch_*, gameoflife.batch.GolBatch; DESIGN.md
section 5f) against the numpy model of tests/batch_model.py.  Every comparison
is per board: the final snapshot word for word and the whole population
series.

The model is computed once per (shape, rule) for the largest board count and
37 generations; a seeded board depends on its index alone, so the first n
boards of that run are the reference for every smaller count, and its history
the reference for every shorter run.

Shapes.  The issue lists (64, 64, clipped, vis (40, 50)); on that board columns
42 .. 63 have no visible neighbour, so it is one of the geometries gol_create --
and with it the batch -- refuses (tests/test_batch_capi.py asserts both).  The
64 x 64 clipped case with explicit visible extents is run at (64, 63) instead:
one board per wave, zero-filling shifts, a visible-column mask of all 64 bits
and a last row that is a sink."""
import functools

import numpy as np
import pytest

import batch_model as M
from gameoflife import _native as N
from gameoflife.batch import GolBatch
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 0xBA7C4
GENS = (1, 2, 3, 37)
# (W, H, topology, vis)
SHAPES = [
    (64, 64, "torus", None),          # one board per wave, DPP rotates
    (64, 64, "ref-clipped", (64, 63)),
    (63, 64, "ref-clipped", None),
    (8, 8, "ref-clipped", None),      # the reference board, k = 8, no idle lane
    (5, 7, "torus", None),            # k = 9, one idle lane
    (33, 21, "torus", None),          # k = 3, one idle lane, a row across the dword boundary
    (32, 33, "ref-clipped", None),    # k = 1, 31 idle lanes
    (64, 3, "torus", None),           # k = 21
    (3, 3, "torus", None),
    (20, 64, "torus", None),          # not in the issue's list: DPP rotates with the upper dword unused (width <= 32)
]
RULES = {"life": O.LIFE, "ref-literal": O.REF_LITERAL, "ref-effective": O.REF_EFFECTIVE,
         "B0/S012345678": (0x001, 0x1FF), "B36/S23": (0x048, 0x00C)}


def _id(shape):
    W, H, topo, vis = shape
    return f"{W}x{H}-{topo}" + (f"-vis{vis[0]}x{vis[1]}" if vis else "")


def _counts(H):
    k = 64 // H
    return sorted({1, max(k - 1, 1), k, k + 1, 4 * k + 1})


@functools.lru_cache(maxsize=None)
def _reference(shape, rule_name, gens=max(GENS), boards=None):
    """(states [gens + 1][n][H], populations [n][gens], settled [n]) of the seeded boards; read-only."""
    W, H, topo, vis = shape
    n = max(_counts(H)) if boards is None else boards
    states, pops, settled = M.run_history(M.seed_rows(n, W, H, SEED), W, gens, topo, RULES[rule_name], vis)
    for a in (states, pops, settled):
        a.setflags(write=False)
    return states, pops, settled


def _batch(boards, shape, rule_name="life"):
    W, H, topo, vis = shape
    return GolBatch(boards, W, H, topology=topo, rule=rule_name, vis=vis)


@pytest.mark.parametrize("rule_name", list(RULES))
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_step_matches_model(gpu, shape, rule_name):
    states, pops, _ = _reference(shape, rule_name)
    H = shape[1]
    k = 64 // H
    for boards in _counts(H):
        for gens in GENS:
            with _batch(boards, shape, rule_name) as b:
                g = b.geometry()
                assert g["boards_per_wave"] == k and g["waves"] == -(-boards // k)
                b.seed(SEED)
                got_pops = b.step(gens, populations=True)
                final = b.snapshot()
                assert b.epoch == gens
            assert np.array_equal(final, states[gens, :boards]), (boards, gens)
            assert np.array_equal(got_pops, pops[:boards, :gens]), (boards, gens)


def test_a_thousand_reference_boards(gpu):
    shape = (8, 8, "ref-clipped", None)
    states, pops, _ = _reference(shape, "life", 12, 1000)
    with _batch(1000, shape) as b:
        b.seed(SEED)
        got = b.step(12, populations=True)
        assert np.array_equal(b.snapshot(), states[12])
        assert np.array_equal(got, pops)
        assert np.array_equal(b.populations(), pops[:, -1])


@pytest.mark.parametrize("shape", [(8, 8, "ref-clipped", None), (5, 7, "torus", None),
                                   (8, 8, "torus", None), (5, 7, "ref-clipped", None)], ids=_id)
def test_seams_do_not_leak(gpu, shape):
    """All-live, empty and seeded boards alternate inside every wave: an empty
    board stays empty and every board equals the model run alone."""
    W, H, topo, vis = shape
    boards = 3 * (64 // H) + 2
    rows = M.seed_rows(boards, W, H, SEED)
    rows[0::3] = np.uint64((1 << W) - 1)
    rows[1::3] = 0
    states, pops, _ = M.run_history(rows, W, 10, topo, O.LIFE, vis)
    with _batch(boards, shape) as b:
        b.load(rows)
        got = b.step(10, populations=True)
        final = b.snapshot()
    assert not final[1::3].any() and not got[1::3].any()
    assert np.array_equal(final, states[10])
    assert np.array_equal(got, pops)


def test_load_and_snapshot_windows(gpu):
    shape = (5, 7, "torus", None)
    W, H = 5, 7
    boards = 20  # k = 9: boards 4 .. 14 start and end inside a wave
    rows = M.seed_rows(boards, W, H, SEED)
    with _batch(boards, shape) as b:
        b.seed(1)
        seeded = b.snapshot()
        junk = rows[4:15] | np.uint64(0xFFFF_FFFF_FFFF_FFE0)  # bits at x >= width are ignored
        b.load(junk, first=4)
        assert b.epoch == 0
        want = seeded.copy()
        want[4:15] = rows[4:15]
        assert np.array_equal(b.snapshot(), want)
        assert np.array_equal(b.snapshot(7, 5), want[7:12])
        assert np.array_equal(b.cells(3, 4), M.unpack(want[3:7], W))
        b.load(M.unpack(rows[:2], W), first=18)  # cells
        want[18:20] = rows[:2]
        assert np.array_equal(b.snapshot(18), want[18:])
        b.step(3)
        assert np.array_equal(b.snapshot(), M.run(want, W, 3)[0])
        for first, count in ((-1, 2), (20, 1), (19, 2), (0, 0), (0, 21)):
            out = np.full((max(count, 1), H), 0xAB, dtype=np.uint64)
            rc = N.lib.gol_batch_snapshot(b._h, first, count, out.ctypes.data_as(N._u64p))
            assert rc == N.GOL_EINVAL and (out == 0xAB).all(), (first, count)
            assert N.lib.gol_batch_load(b._h, first, count, out.ctypes.data_as(N._u64p)) == N.GOL_EINVAL
        assert np.array_equal(b.snapshot(), M.run(want, W, 3)[0]) and b.epoch == 3


@pytest.mark.parametrize("shape", [(64, 64, "torus", None), (33, 21, "torus", None), (8, 8, "ref-clipped", None)],
                         ids=_id)
def test_seed_matches_model(gpu, shape):
    W, H = shape[0], shape[1]
    with _batch(11, shape) as b:
        b.seed(0x1234_5678_9ABC_DEF0)
        assert np.array_equal(b.snapshot(), M.seed_rows(11, W, H, 0x1234_5678_9ABC_DEF0))
        assert b.epoch == 0


SETTLE_SHAPE = (12, 10, "torus", None)


def test_settled(gpu):
    _, pops, want = _reference(SETTLE_SHAPE, "life", 30, 64)
    # a condition on the input: 30 generations split these soups
    assert (want == 0).any() and (want != 0).any()
    with _batch(64, SETTLE_SHAPE) as b:
        b.seed(SEED)
        got = b.step(30, settled=True)
        assert np.array_equal(got, want)
        # both series at once, and the settle words of a second call start afresh
        b.seed(SEED)
        got_pops, got = b.step(30, populations=True, settled=True)
        assert np.array_equal(got, want) and np.array_equal(got_pops, pops)
        again = b.step(4, settled=True)
        assert np.array_equal(again[want != 0], np.full(int((want != 0).sum()), 2, dtype=np.uint32))


def test_settled_blinker_block_glider(gpu):
    def board(live):
        c = np.zeros((12, 12), dtype=np.uint8)
        for x, y in live:
            c[y, x] = 1
        return c
    cells = np.stack([board([(4, 5), (5, 5), (6, 5)]), board([(4, 4), (5, 4), (4, 5), (5, 5)]),
                      board([(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)])])
    with GolBatch(3, 12, 12) as b:
        b.load(cells)
        assert b.step(20, settled=True).tolist() == [2, 2, 0]
        b.load(cells)
        assert b.step(1, settled=True).tolist() == [0, 0, 0]


@pytest.mark.parametrize("shape", [(33, 21, "torus", None), (8, 8, "ref-clipped", None), (64, 64, "torus", None)],
                         ids=_id)
def test_chunk_knob_changes_nothing(gpu, shape):
    states, pops, _ = _reference(shape, "life")
    boards = states.shape[1]
    with _batch(boards, shape) as b:
        b.seed(SEED)
        one_pops, one_settled = b.step(37, populations=True, settled=True)
        assert np.array_equal(b.snapshot(), states[37]) and np.array_equal(one_pops, pops)
        b.set_chunk(7)
        b.seed(SEED)
        p7, s7 = b.step(37, populations=True, settled=True)
        assert np.array_equal(b.snapshot(), states[37])
        assert np.array_equal(p7, one_pops) and np.array_equal(s7, one_settled)
        b.set_chunk(0)
        b.seed(SEED)
        pa = b.step(20, populations=True)
        pb = b.step(17, populations=True)
        assert b.epoch == 37
        assert np.array_equal(b.snapshot(), states[37])
        assert np.array_equal(np.concatenate([pa, pb], axis=1), one_pops)
        b.set_chunk(1)
        b.seed(SEED)
        p1, s1 = b.step(5, populations=True, settled=True)
        assert np.array_equal(b.snapshot(), states[5]) and np.array_equal(p1, pops[:, :5])
        b.set_chunk(0)
        b.seed(SEED)
        assert np.array_equal(b.step(5, settled=True), s1)


def test_chunk_knob_settled_on_soups(gpu):
    _, _, want = _reference(SETTLE_SHAPE, "life", 30, 64)
    with _batch(64, SETTLE_SHAPE) as b:
        for chunk in (7, 1, 2, 29):
            b.set_chunk(chunk)
            b.seed(SEED)
            assert np.array_equal(b.step(30, settled=True), want), chunk


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_hashes_match_model(gpu, shape):
    states, pops, _ = _reference(shape, "life")
    W = shape[0]
    boards = states.shape[1]
    with _batch(boards, shape) as b:
        b.seed(SEED)
        assert np.array_equal(b.hashes(), M.hashes(states[0], W))
        b.step(9)
        assert np.array_equal(b.hashes(), M.hashes(states[9], W))
        assert np.array_equal(b.populations(), pops[:, 8])


@pytest.mark.parametrize("shape", [(64, 64, "torus", None), (8, 8, "ref-clipped", None)], ids=_id)
def test_hashes_equal_the_main_engine(gpu, shape):
    from gameoflife.engine import GolEngine
    W, H, topo, vis = shape
    rows = M.seed_rows(3, W, H, SEED)
    with _batch(3, shape) as b:
        b.seed(SEED)
        h0 = b.hashes()
        b.step(9)
        h9 = b.hashes()
    for i in range(3):
        with GolEngine(W, H, topology=topo, rule="life") as e:
            e.load(O.pack(M.unpack(rows[i:i + 1], W)[0]))
            assert e.hash() == int(h0[i])
            e.step(9)
            assert e.hash() == int(h9[i])


def test_series_only_when_asked(gpu):
    shape = (33, 21, "torus", None)
    states, _, _ = _reference(shape, "life")
    boards = states.shape[1]
    with _batch(boards, shape) as b:
        b.seed(SEED)
        pops = np.full(boards * 10, 0xDEAD, dtype=np.uint32)
        settled = np.full(boards, 0xBEEF, dtype=np.uint32)
        # capacity is ignored without an array; nothing is written to either
        assert N.lib.gol_batch_step(b._h, 10, None, 0, None) == N.GOL_OK
        assert (pops == 0xDEAD).all() and (settled == 0xBEEF).all()
        assert np.array_equal(b.snapshot(), states[10])
        # a short buffer: refused, nothing advanced, nothing written
        rc = N.lib.gol_batch_step(b._h, 10, pops.ctypes.data_as(N._u32p), boards * 10 - 1,
                                  settled.ctypes.data_as(N._u32p))
        assert rc == N.GOL_EINVAL and b.epoch == 10
        assert (pops == 0xDEAD).all() and (settled == 0xBEEF).all()
        assert np.array_equal(b.snapshot(), states[10])
        assert N.lib.gol_batch_step(b._h, 0, None, 0, None) == N.GOL_OK and b.epoch == 10
        assert N.lib.gol_batch_hashes(b._h, 0, boards, None, None) == N.GOL_EINVAL


def test_epoch_bookkeeping(gpu):
    with GolBatch(5, 8, 8, topology="ref-clipped") as b:
        assert b.epoch == 0
        b.seed(3)
        b.step(4)
        b.step(0)
        b.step(3, populations=True)
        assert b.epoch == 7
        b.seed(4)
        assert b.epoch == 0
        b.step(2)
        b.load(np.zeros((1, 8), dtype=np.uint64), first=2)
        assert b.epoch == 0
        b.set_chunk(3)
        b.step(10)
        assert b.epoch == 10
