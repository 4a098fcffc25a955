"""GPU: the objects of a batch's boards (gol_objects_batch, GolBatch.objects;
DESIGN.md section 5i).  Counts and records bit for bit against the cell-level
model of tests/objects_model.py (a breadth-first search, boxes by listing the
empty runs, the C oracle's hash).  The seeded boards are those of
tests/objects_cases.py, computed once and shared read-only with the CPU tests;
the boards are loaded from the model's states, so nothing here depends on the
step kernels but the tests that say so."""
import ctypes

import numpy as np
import pytest

import batch_model as M
import objects_cases as C
import objects_model as OM
from gameoflife import _native as N
from gameoflife import patterns as P
from gameoflife.batch import OBJECT_DTYPE, GolBatch, match_positions, tally
from test_gpu_batch_cycles import _model as cycle_model

pytestmark = pytest.mark.gpu

T64, C64, T8, C8 = (C.SHAPES[i][0] for i in range(4))
BLOCK = ["OO", "OO"]
BLINKER_H = ["OOO"]
BLINKER_V = ["O", "O", "O"]
BEEHIVE = [".OO.", "O..O", ".OO."]


def _batch(boards, shape):
    W, H, topo, vis = shape
    return GolBatch(boards, W, H, topology=topo, vis=vis)


def _same(got, want):
    """(counts, objects) equal bit for bit."""
    assert got[0].dtype == np.uint32 and got[1].dtype == OBJECT_DTYPE
    assert np.array_equal(got[0], want[0]), (got[0].tolist(), want[0].tolist())
    differ = np.flatnonzero((got[1] != want[1]).any(axis=1))
    assert differ.size == 0, (differ[:4].tolist(), got[1][differ[0]][:6].tolist(), want[1][differ[0]][:6].tolist())
    assert got[1].tobytes() == want[1].tobytes()  # the reserved field and the records past the count: zero


def _cells(W, H, *boards):
    """uint8 [n][H][W] boards from lists of (x, y)."""
    out = np.zeros((len(boards), H, W), dtype=np.uint8)
    for b, cells in zip(out, boards):
        for x, y in cells:
            b[y, x] = 1
    return out


def _by_hand(shape, cells, reach, max_objects=16):
    """GolBatch.objects of hand-made boards, checked against the model; returns it."""
    W, H, topo, vis = shape
    with _batch(len(cells), shape) as b:
        b.load(cells)
        got = b.objects(reach=reach, max_objects=max_objects)
        stats = b.objects_stats()
    want = OM.batch_objects(M.pack(cells), W, topo == "torus", reach, max_objects)
    _same(got, want)
    assert stats == {"launches": 1, "objects": int(want[0].sum()),
                     "boards_truncated": int((want[0] > max_objects).sum())}
    return got


def _box(rec):
    return tuple(int(rec[f]) for f in ("x", "y", "w", "h", "population"))


@pytest.mark.parametrize("reach", C.REACHES)
@pytest.mark.parametrize("case", C.SHAPES, ids=C.shape_id)
def test_seeded_shapes_match_model(gpu, case, reach):
    shape, boards = case
    with _batch(boards, shape) as b:
        for g in C.generations(shape):
            want = C.model(shape, boards, g, reach)
            assert 0 < want[0].max() <= C.MAX_OBJECTS  # nothing is truncated
            b.load(C.states(shape, boards)[g])
            _same(b.objects(reach=reach, max_objects=C.MAX_OBJECTS), want)
            assert b.objects_stats() == {"launches": 1, "objects": int(want[0].sum()), "boards_truncated": 0}


def test_the_largest_count_of_the_seeded_shapes_is_73():
    most = max(int(C.model(s, n, g, r)[0].max()) for s, n in C.SHAPES for g in C.generations(s) for r in C.REACHES)
    assert most == 73 == int(C.model(T64, 5, 64, 1)[0].max())


def test_truncation_keeps_the_counts_exact(gpu):
    full = C.model(T64, 5, 64, 1)
    want = C.model(T64, 5, 64, 1, 8)
    assert np.array_equal(want[0], full[0]) and np.array_equal(want[1], full[1][:, :8]) and (full[0] > 8).all()
    with _batch(5, T64) as b:
        b.load(C.states(T64, 5)[64])
        _same(b.objects(reach=1, max_objects=8), want)
        assert b.objects_stats() == {"launches": 1, "objects": int(full[0].sum()), "boards_truncated": 5}
        _same(b.objects(reach=1, max_objects=C.MAX_OBJECTS), full)  # the buffers grow
        assert b.objects_stats()["boards_truncated"] == 0


def test_every_second_cell_is_1024_objects_or_one(gpu):
    cells = _cells(64, 64, [(x, y) for y in range(0, 64, 2) for x in range(0, 64, 2)])
    counts, objs = _by_hand(T64, cells, 1, 1024)
    assert counts.tolist() == [1024] and (objs["population"] == 1).all() and (objs["w"] == 1).all()
    assert len(set(objs["hash"][0].tolist())) == 1
    counts, objs = _by_hand(T64, cells, 2, 1024)
    assert counts.tolist() == [1] and _box(objs[0, 0]) == (0, 0, 64, 64, 1024)
    counts, objs = _by_hand(T64, cells, 1, 5)  # 1024 objects and room for 5
    assert counts.tolist() == [1024]


@pytest.mark.parametrize("shape", [T64, C64], ids=["torus", "ref-clipped"])
def test_a_serpentine_is_one_object(gpu, shape):
    """Corridors one cell wide in columns 1 .. 62 and rows 1 .. 61, joined at alternating ends: at reach 1 the fill
    walks all of it, about 1950 steps."""
    snake = [(x, y) for y in range(1, 62, 2) for x in range(1, 63)]
    snake += [(62 if (y // 2) % 2 else 1, y) for y in range(2, 61, 2)]
    cells = _cells(64, 64, snake)
    for reach in C.REACHES:
        counts, objs = _by_hand(shape, cells, reach)
        assert counts.tolist() == [1] and _box(objs[0, 0]) == (1, 1, 62, 61, len(snake))


def test_a_block_on_both_seams(gpu):
    corners = [(0, 0), (63, 0), (0, 63), (63, 63)]
    cells = _cells(64, 64, corners)
    for reach in C.REACHES:
        counts, objs = _by_hand(T64, cells, reach)
        assert counts.tolist() == [1] and _box(objs[0, 0]) == (63, 63, 2, 2, 4)
        assert int(objs[0, 0]["hash"]) == P.object_hash(BLOCK)
        counts, objs = _by_hand(C64, cells, reach)
        assert counts.tolist() == [4]
        assert [_box(r)[:2] for r in objs[0, :4]] == corners and (objs[0, :4]["hash"] == P.object_hash(["O"])).all()


@pytest.mark.parametrize("shape", [T8, C8], ids=["torus", "ref-clipped"])
def test_boards_of_one_wave_never_join(gpu, shape):
    torus = shape[2] == "torus"
    # board 0's last row and board 1's first are neighbouring lanes; board 2 holds both rows itself; 9 boards: 2 waves
    cells = _cells(8, 8, [(3, 7)], [(3, 0)], [(3, 7), (4, 0)], [], [], [], [], [(0, 7)], [(0, 0), (7, 7)])
    for reach in C.REACHES:
        counts, objs = _by_hand(shape, cells, reach)
        assert counts.tolist() == ([1, 1, 1, 0, 0, 0, 0, 1, 1] if torus else [1, 1, 2, 0, 0, 0, 0, 1, 2])
        assert _box(objs[0, 0]) == (3, 7, 1, 1, 1) and _box(objs[1, 0]) == (3, 0, 1, 1, 1)
        if torus:
            assert _box(objs[2, 0]) == (3, 7, 2, 2, 2) and _box(objs[8, 0]) == (7, 7, 2, 2, 2)


def test_reach_decides_whether_a_gap_of_one_joins(gpu):
    for shape in (T64, C64, T8, C8, C.SHAPES[5][0]):
        cells = _cells(shape[0], shape[1], [(0, 0), (2, 0)])
        counts, objs = _by_hand(shape, cells, 1)
        assert counts.tolist() == [2] and _box(objs[0, 0]) == (0, 0, 1, 1, 1) and _box(objs[0, 1]) == (2, 0, 1, 1, 1)
        counts, objs = _by_hand(shape, cells, 2)
        assert counts.tolist() == [1] and _box(objs[0, 0]) == (0, 0, 3, 1, 2)
        assert int(objs[0, 0]["hash"]) == P.object_hash(["O.O"])


def test_a_full_row_goes_round_and_a_dead_board_has_nothing(gpu):
    for shape in (T64, T8, C.SHAPES[5][0], C.SHAPES[4][0]):
        W, H = shape[:2]
        cells = _cells(W, H, [(x, 2) for x in range(W)], [], [(1, y) for y in range(H)])
        for reach in C.REACHES:
            counts, objs = _by_hand(shape, cells, reach)
            assert counts.tolist() == [1, 0, 1]
            assert _box(objs[0, 0]) == (0, 2, W, 1, W) and _box(objs[2, 0]) == (1, 0, 1, H, H)
            assert not objs[1].tobytes().strip(b"\0")


@pytest.mark.parametrize("case,gens", [(C.SHAPES[0], 1024), (C.SHAPES[1], 1024), (C.SHAPES[2], 512),
                                       (C.SHAPES[5], 512)], ids=lambda v: C.shape_id(v) if isinstance(v, tuple) else None)
def test_records_agree_with_the_device_search(gpu, case, gens):
    """On the ash: the records with a pattern's (object_hash, w, h, population) are the anchors find(pattern,
    border=reach) reports, moved by reach.  Two things the search wants beyond the object being one: on a clipped
    board it has no anchor left of or above the board, so there the records whose box starts within `reach` of
    those edges are not among its matches; and its border is the whole ring round the pattern's box, whose corners
    are further than `reach` from a beehive's cells -- a record whose ring holds a cell of another object (seen on
    the snapshot) is no match.  Around a filled rectangle (block, blinker) every cell of the ring is within `reach`
    of the object, so there the ring is asserted to be dead."""
    shape, boards = case
    W, H, topo, vis = shape
    torus = topo == "torus"
    with _batch(boards, shape) as b:
        b.seed(C.SEED)
        b.step(gens)
        assert np.array_equal(b.snapshot(), C.states(shape, boards)[gens])
        board_cells = M.unpack(b.snapshot(), W)
        found = 0
        for reach in C.REACHES:
            counts, objs = b.objects(reach=reach, max_objects=C.MAX_OBJECTS)
            for pat in (BLOCK, BEEHIVE, BLINKER_H, BLINKER_V):
                cells = P.as_cells(pat)
                if cells.shape[1] + 2 * reach > W or cells.shape[0] + 2 * reach > H:
                    continue
                key = (P.object_hash(pat), cells.shape[1], cells.shape[0], int(cells.sum()))
                is_it = ((objs["hash"] == key[0]) & (objs["w"] == key[1]) & (objs["h"] == key[2]) &
                         (objs["population"] == key[3]))
                if not torus:
                    is_it &= (objs["x"] >= reach) & (objs["y"] >= reach)
                for bi, ji in zip(*np.nonzero(is_it)):  # the ring round the box, from the snapshot
                    r = objs[bi, ji]
                    ys = np.arange(int(r["y"]) - reach, int(r["y"]) + int(r["h"]) + reach)
                    xs = np.arange(int(r["x"]) - reach, int(r["x"]) + int(r["w"]) + reach)
                    if torus:
                        ys, xs = ys % H, xs % W
                    else:
                        ys, xs = ys[ys < H], xs[xs < W]
                    ring_dead = int(board_cells[bi][np.ix_(ys, xs)].sum()) == key[3]
                    assert ring_dead or pat is BEEHIVE, (pat, reach, bi, ji)
                    is_it[bi, ji] = ring_dead
                n, planes = b.find(pat, border=reach, matches=True)
                assert np.array_equal(is_it.sum(axis=1), n[:, 0]), (pat, reach)
                at = match_positions(planes[0], W)
                at[:, 1] = (at[:, 1] + reach) % W
                at[:, 2] = (at[:, 2] + reach) % H
                bi, ji = np.nonzero(is_it)
                mine = np.stack([bi, objs["x"][bi, ji], objs["y"][bi, ji]], axis=1).astype(np.int64)
                assert sorted(map(tuple, at.tolist())) == sorted(map(tuple, mine.tolist())), (pat, reach)
                found += len(mine)
            table = P.object_table({"block": [BLOCK], "beehive": [BEEHIVE], "blinker": [BLINKER_H, BLINKER_V]})
            census = tally(counts, objs, table)
            assert sum(census.values()) == int(counts.sum())
        assert found > 0


def test_sub_ranges_are_rows_of_the_whole_call(gpu):
    for shape, boards in (C.SHAPES[2], C.SHAPES[4], C.SHAPES[0]):
        g = C.generations(shape)[-1]
        whole = C.model(shape, boards, g, 1)
        with _batch(boards, shape) as b:
            b.load(C.states(shape, boards)[g])
            for first, count in ((0, 1), (boards - 1, 1), (1, boards - 1), (3, 2), (boards // 2, boards - boards // 2)):
                got = b.objects(reach=1, max_objects=C.MAX_OBJECTS, first=first, count=count)
                _same(got, (whole[0][first:first + count], whole[1][first:first + count]))
            _same(b.objects(reach=1, max_objects=C.MAX_OBJECTS, first=2), (whole[0][2:], whole[1][2:]))


def test_a_call_changes_nothing(gpu):
    boards, N_ = 33, 512
    W, H, topo, vis = T8
    rows = M.seed_rows(boards, W, H, C.SEED)
    with _batch(boards, T8) as b:
        b.seed(C.SEED)
        b.step(3)
        before = (b.snapshot(), b.hashes(), b.epoch)
        for reach in C.REACHES:
            b.objects(reach=reach)
        assert np.array_equal(b.snapshot(), before[0]) and np.array_equal(b.hashes(), before[1])
        assert b.epoch == before[2] == 3
        # a settle step that follows gives the model's answer
        b.seed(C.SEED)
        b.objects()
        pops, settled = b.step(64, populations=True, settled=True)
        want = M.run(rows, W, 64, topo)
        assert np.array_equal(b.snapshot(), want[0]) and np.array_equal(pops, want[1])
        assert np.array_equal(settled, want[2])
        # ... and so does a cycle step, and one after a call between two of them
        final, period, seen = cycle_model(T8, boards, N_)
        b.seed(C.SEED)
        b.objects()
        got = b.step_cycles(N_)
        assert np.array_equal(got[0], period) and np.array_equal(got[1], seen) and np.array_equal(b.snapshot(), final)
        with _batch(boards, T8) as other:
            other.seed(C.SEED)
            other.step_cycles(100)
            plain = other.step_cycles(N_ - 100)
            b.seed(C.SEED)
            b.step_cycles(100)
            b.objects(reach=2, max_objects=7)
            mine = b.step_cycles(N_ - 100)
            assert np.array_equal(mine[0], plain[0]) and np.array_equal(mine[1], plain[1])
            assert np.array_equal(b.snapshot(), other.snapshot()) and b.epoch == other.epoch == N_


def test_refusals_leave_the_outputs_untouched(gpu):
    with _batch(3, T8) as b:
        b.seed(C.SEED)
        counts = np.full(3, 0xABCDEF01, dtype=np.uint32)
        objs = np.full(3 * 4 * 16, 0x5A, dtype=np.uint8).view(OBJECT_DTYPE)
        sentinel = (counts.copy(), objs.copy())
        cp, op = counts.ctypes.data_as(N._u32p), objs.ctypes.data_as(ctypes.POINTER(N.GolBatchObject))
        refusals = {
            "reach 0": ((0, 3, 0, 4, cp, 3, op, 12), b"reach must be 1 or 2"),
            "reach 3": ((0, 3, 3, 4, cp, 3, op, 12), b"reach must be 1 or 2"),
            "max_objects 0": ((0, 3, 1, 0, cp, 3, op, 12), b"max_objects must be 1 .. 1024"),
            "max_objects 1025": ((0, 3, 1, 1025, cp, 3, op, 12), b"max_objects must be 1 .. 1024"),
            "first -1": ((-1, 3, 1, 4, cp, 3, op, 12), b"outside the batch"),
            "count 0": ((0, 0, 1, 4, cp, 3, op, 12), b"outside the batch"),
            "past the end": ((1, 3, 1, 4, cp, 3, op, 12), b"outside the batch"),
            "null counts": ((0, 3, 1, 4, None, 3, op, 12), b"null"),
            "null objects": ((0, 3, 1, 4, cp, 3, None, 12), b"null"),
            "short counts": ((0, 3, 1, 4, cp, 2, op, 12), b"counts_out holds 2"),
            "short objects": ((0, 3, 1, 4, cp, 3, op, 11), b"objects_out holds 11"),
        }
        for what, (args, word) in refusals.items():
            assert N.lib.gol_objects_batch(b._h, *args) == N.GOL_EINVAL, what
            assert word in N.lib.gol_batch_last_error(b._h), (what, N.lib.gol_batch_last_error(b._h))
            assert np.array_equal(counts, sentinel[0]) and objs.tobytes() == sentinel[1].tobytes(), what
        assert b.objects_stats() == {"launches": 0, "objects": 0, "boards_truncated": 0}
        assert N.lib.gol_objects_batch(b._h, 0, 3, 1, 4, cp, 3, op, 12) == N.GOL_OK
        _same((counts, objs.reshape(3, 4)), OM.batch_objects(M.seed_rows(3, 8, 8, C.SEED), 8, True, 1, 4))
