"""GPU: the pattern search on a batch (gol_find_batch, GolBatch.find; DESIGN.md
section 5h).  Counts, and match planes bit for bit, against the cell-level
model of tests/find_model.py on the unpacked boards.  The shapes are those of
tests/test_gpu_batch_cycles.py, seeded alike (tests/batch_find_cases.py); the
model's answers are computed once per (shape, list) and shared read-only, and
every case asserts on the model's answer that some count is > 0 and some is 0,
so neither an all-zero nor an everything-matches device answer can pass."""
import numpy as np
import pytest

import batch_find_cases as K
import batch_model as M
import cycle_model as C
from gameoflife import _native as N_
from gameoflife.batch import GolBatch, match_positions
from gameoflife.engine import GolEngine
from gameoflife import patterns as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

T8 = K.SHAPES[2][0]
C8 = K.SHAPES[3][0]
T64 = K.SHAPES[0][0]


def _batch(boards, shape):
    W, H, topo, vis = shape
    return GolBatch(boards, W, H, topology=topo, vis=vis)


def _find(b, patterns, matches=True):
    """GolBatch.find of prepared (cells, care) pairs."""
    return b.find([c for c, _ in patterns], care=[m for _, m in patterns], matches=matches)


def _check(b, patterns, counts, planes):
    assert (counts > 0).any() and (counts == 0).any()
    got_counts, got_planes = _find(b, patterns)
    assert got_counts.dtype == np.uint32 and got_planes.dtype == np.uint64
    assert np.array_equal(got_counts, counts), (got_counts.tolist(), counts.tolist())
    assert np.array_equal(got_planes, planes)
    assert np.array_equal(_find(b, patterns, matches=False), counts)  # the launch without match planes


@pytest.mark.parametrize("case", K.SHAPES, ids=K.shape_id)
def test_soup_patterns_match_model(gpu, case):
    """The raw seeded soup: the 1 x 1 live cell (the populations), the bare block, a care mask with holes, the empty
    3 x 3 box, board 0 itself as a pattern of the board's size and, on 64 columns, cared columns 0, 31, 32 and 63."""
    shape, boards, _ = case
    patterns, counts, planes = K.reference_for(shape, boards, 0, "soup")
    with _batch(boards, shape) as b:
        b.seed(K.SEED)
        _check(b, patterns, counts, planes)
        assert np.array_equal(b.find(["O"])[:, 0], b.populations())
        whole = [p for p, (c, _) in enumerate(patterns) if c.shape == (shape[1], shape[0])][-1]
        got = b.find(patterns[whole][0], matches=True)  # npatterns = 1
        assert np.array_equal(got[0][:, 0], counts[:, whole]) and int(got[1][0, 0, 0]) & 1


@pytest.mark.parametrize("case", K.SHAPES[K.ASH_SHAPES], ids=K.shape_id)
def test_ash_objects_standing_alone_match_model(gpu, case):
    """Block, both blinker phases, beehive and a glider with border=1 after 1024 / 512 / 64 generations."""
    shape, boards, gens = case
    patterns, counts, planes = K.reference_for(shape, boards, gens, "ash")
    with _batch(boards, shape) as b:
        b.seed(K.SEED)
        b.step(gens)
        assert np.array_equal(b.snapshot(), K.boards_after(shape, boards, gens))
        _check(b, patterns, counts, planes)


@pytest.mark.parametrize("case", K.SHAPES, ids=K.shape_id)
def test_nine_patterns_in_one_call_and_the_launch_cut(gpu, case):
    """A list of 9 in one call; then the same list under a cut of 5 cared cells -- fewer than most of its patterns
    have, so nearly every pattern goes in a launch of its own -- and under cuts that group them otherwise."""
    shape, boards, _ = case
    patterns, counts, planes = K.reference_for(shape, boards, 0, "nine")
    assert len(patterns) == 9
    cared = sum(int(m.sum()) for _, m in patterns)
    with _batch(boards, shape) as b:
        b.seed(K.SEED)
        _check(b, patterns, counts, planes)
        launches = {}
        for cut in (5, 16, 1, 0):
            b.set_find_cut(cut)
            _check(b, patterns, counts, planes)
            stats = b.find_stats()
            assert stats["cared_cells"] == cared
            launches[cut] = stats["launches"]
        assert launches[1] == 9 and launches[1] >= launches[5] >= launches[16] >= launches[0] >= 1
        assert launches[5] > 1
        if cared <= N_.GOL_FIND_BATCH_AUTO_CUT:
            assert launches[0] == 1


def _load9(cells_by_board, W=8, H=8):
    rows = np.zeros((9, H), dtype=np.uint64)
    for i, cells in cells_by_board.items():
        rows[i] = M.pack(np.asarray(cells, dtype=np.uint8)[None])[0]
    return rows


def test_seams_by_hand(gpu):
    # a block over both seams of board 4: cells (7, 7), (0, 7), (7, 0), (0, 0)
    wrapped = np.zeros((8, 8), dtype=np.uint8)
    wrapped[[7, 7, 0, 0], [7, 0, 7, 0]] = 1
    # a live cell on the last row of board 2 and one on row 0 of board 3, same column: the lane seam
    last, first = np.zeros((8, 8), dtype=np.uint8), np.zeros((8, 8), dtype=np.uint8)
    last[7, 3] = first[0, 3] = 1
    rows = _load9({4: wrapped, 2: last, 3: first})
    domino = [P.as_search(["O", "O"])]
    block = [P.as_search(K.BLOCK, border=1)]
    for shape in (T8, C8):
        torus = shape[2] == "torus"
        with _batch(9, shape) as b:
            b.load(rows)
            counts, planes = _find(b, block)
            want = np.zeros(9, dtype=np.uint32)
            want[4] = 1 if torus else 0  # the same cells are four corners on a clipped board
            assert np.array_equal(counts[:, 0], want)
            # the bordered block's top-left cell is the border's: the block at (7, 7) is found at anchor (6, 6)
            assert match_positions(planes[0], 8).tolist() == ([[4, 6, 6]] if torus else [])
            counts, planes = _find(b, domino)
            assert counts[2, 0] == 0 and counts[3, 0] == 0  # not a vertical domino of either board
            # board 4's corners are two dominoes on a torus (anchors (0, 7) and (7, 7)), none on a clipped board
            assert counts[:, 0].tolist() == [0, 0, 0, 0, 2 if torus else 0, 0, 0, 0, 0]
            ref = K.reference(rows, shape, block + domino)
            got = _find(b, block + domino)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_glider_in_each_orientation_is_counted_once(gpu):
    images = P.orientations(P.from_rows(K.GLIDER))
    assert len(images) == 8
    boards = np.zeros((9, 8, 8), dtype=np.uint8)
    for i, (cells, _) in enumerate(images):
        boards[i, 2:5, 3:6] = cells
    with GolBatch(9, 8, 8) as b:
        b.load(boards)
        counts, planes = b.find(K.GLIDER, border=1, orientations=True, matches=True)
        assert counts.shape == (9, 1) and planes.shape == (1, 9, 8)
        assert counts[:, 0].tolist() == [1] * 8 + [0]
        assert match_positions(planes[0], 8).tolist() == [[i, 2, 1] for i in range(8)]  # the border's top-left cell
        one = b.find(K.GLIDER, border=1)  # the orientation as written alone
        assert one[:, 0].tolist() == [1] + [0] * 8
        # a list: each pattern folded by itself
        both = b.find([K.GLIDER, K.BLOCK], border=1, orientations=True)
        assert both.shape == (9, 2) and both[:, 0].tolist() == [1] * 8 + [0] and not both[:, 1].any()


@pytest.mark.parametrize("shape,boards,gens", [(T8, 33, 512), (T64, 5, 100)], ids=["8x8", "64x64"])
def test_find_changes_nothing(gpu, shape, boards, gens):
    """snapshot, hashes and epoch after a find, and what a following settle step and cycle step return: those of a
    batch that never searched (the search must not write the plane settle and cycle detection keep)."""
    W = shape[0]
    rows = M.seed_rows(boards, W, shape[1], K.SEED)
    x30, _, settled30 = M.run(rows, W, 30)
    final, period, seen = C.run(x30, W, gens)
    patterns = K.nine_patterns(shape, boards)
    with _batch(boards, shape) as b:
        b.seed(K.SEED)
        b.step(7, settled=True)
        before = (b.snapshot(), b.hashes(), b.epoch)
        for chunk in (3, 0):
            b.set_chunk(chunk)  # the step's chunk is nothing to the search
            got = _find(b, patterns)
            ref = K.reference(before[0], shape, patterns)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.array_equal(b.snapshot(), before[0]) and np.array_equal(b.hashes(), before[1])
        assert b.epoch == before[2] == 7
        b.seed(K.SEED)
        _find(b, patterns)
        assert np.array_equal(b.step(30, settled=True), settled30)
        _find(b, patterns)
        got = b.step_cycles(gens)
        assert np.array_equal(got[0], period) and np.array_equal(got[1], seen)
        assert (period > 0).any() == (shape is T8)
        assert np.array_equal(b.snapshot(), final) and b.epoch == 30 + gens


def test_equals_the_context_path(gpu):
    """One 64 x 64 torus board in a GolEngine: find(pattern, border=1) gives the count and positions of the batch's
    match plane for that board."""
    rows = K.boards_after(T64, 5, 1024)
    cells = M.unpack(rows, 64)
    with _batch(5, T64) as b, GolEngine(64, 64, topology="torus") as e:
        b.load(rows)
        e.load(O.pack(cells[1]))
        for obj in (K.BLOCK, K.BLINKER_H, K.BEEHIVE):
            counts, planes = b.find(obj, border=1, matches=True)
            want = e.find(obj, border=1)
            assert want["count"] > 0 and counts[1, 0] == want["count"]
            mine = match_positions(planes[0], 64)
            mine = mine[mine[:, 0] == 1][:, 1:]
            assert np.array_equal(mine, want["matches"])  # both sorted by (y, x)


def test_arguments(gpu):
    with GolBatch(3, 8, 8) as b:
        b.seed(K.SEED)
        assert b.find_stats() == {"launches": 0, "cared_cells": 0}
        block = np.array([3, 3], dtype=np.uint64)
        t = (N_.GolBatchPattern * 1)()
        t[0].pw, t[0].ph, t[0].cells = 2, 2, block.ctypes.data_as(N_._u64p)
        counts = np.full(3, 0xDEAD, dtype=np.uint32)
        planes = np.full(24, 0xBEEF, dtype=np.uint64)
        cp, pp = counts.ctypes.data_as(N_._u32p), planes.ctypes.data_as(N_._u64p)
        L = N_.lib
        for rc in (L.gol_find_batch(b._h, t, 1, cp, 2, None, 0),       # a short counts capacity
                   L.gol_find_batch(b._h, t, 1, cp, 3, pp, 23),        # a short matches capacity
                   L.gol_find_batch(b._h, t, 1, None, 3, None, 0),     # counts_out is required
                   L.gol_find_batch(b._h, None, 1, cp, 3, None, 0),
                   L.gol_find_batch(b._h, t, 0, cp, 3, None, 0)):
            assert rc == N_.GOL_EINVAL and L.gol_batch_last_error(b._h)
        t[0].pw = 9
        assert L.gol_find_batch(b._h, t, 1, cp, 3, pp, 24) == N_.GOL_EINVAL
        assert b"pattern 0" in L.gol_batch_last_error(b._h)
        assert (counts == 0xDEAD).all() and (planes == 0xBEEF).all() and b.find_stats()["launches"] == 0
        t[0].pw = 2
        assert L.gol_find_batch(b._h, t, 1, cp, 3, pp, 24) == N_.GOL_OK
        ref = K.reference(b.snapshot(), T8, [P.as_search(K.BLOCK)])
        assert np.array_equal(counts, ref[0][:, 0]) and np.array_equal(planes.reshape(1, 3, 8), ref[1])
        # bits at k >= pw are ignored in both rows
        noisy = np.array([0xF3, 0x13], dtype=np.uint64)
        care = np.array([0xFF, 0xFF], dtype=np.uint64)
        t[0].cells, t[0].care = noisy.ctypes.data_as(N_._u64p), care.ctypes.data_as(N_._u64p)
        again = np.zeros(3, dtype=np.uint32)
        assert L.gol_find_batch(b._h, t, 1, again.ctypes.data_as(N_._u32p), 3, None, 0) == N_.GOL_OK
        assert np.array_equal(again, counts)
        with pytest.raises(ValueError):
            b.find(np.ones((9, 2), dtype=np.uint8))
