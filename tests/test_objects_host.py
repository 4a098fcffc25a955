"""CPU: the host side of the objects of a board (patterns.label_objects,
object_hash, object_table) against the cell-level model
of tests/objects_model.py on the seeded boards of tests/objects_cases.py."""
import numpy as np
import pytest

import batch_model as M
import objects_cases as C
import objects_model as OM
from gameoflife import patterns as P

BLOCK = ["OO", "OO"]
BLINKER = ["OOO"]
GLIDER = [".O.", "..O", "OOO"]
BEEHIVE = [".OO.", "O..O", ".OO."]


@pytest.mark.parametrize("case", C.SHAPES, ids=C.shape_id)
def test_label_objects_equals_the_model(case):
    shape, boards = case
    W, H, topo, vis = shape
    torus = topo == "torus"
    for g in C.generations(shape):
        cells = M.unpack(C.states(shape, boards)[g], W)
        for reach in C.REACHES:
            counts, objects = C.model(shape, boards, g, reach)
            assert counts.max() <= C.MAX_OBJECTS
            for b in range(boards):
                got = P.label_objects(cells[b], torus=torus, reach=reach)
                assert got.dtype == P.OBJECT_DTYPE and len(got) == counts[b], (g, reach, b)
                assert np.array_equal(got, objects[b, :counts[b]]), (g, reach, b)


def test_fixture_facts_of_the_seeded_boards():
    """What the device tests rely on, asserted on the model."""
    T64 = C.SHAPES[0]
    assert T64[0][:3] == (64, 64, "torus")
    most = max(int(C.model(s, n, g, r)[0].max()) for s, n in C.SHAPES for g in C.generations(s) for r in C.REACHES)
    assert most == 73 == int(C.model(T64[0], T64[1], 64, 1)[0].max())
    # the raw soups hold one object of about 2000 cells
    assert all(1800 < int(o["population"].max()) < 2300 for o in C.model(T64[0], T64[1], 0, 1)[1])
    # objects that go round an axis occur, on the small tori at least
    counts, objects = C.model(C.SHAPES[8][0], C.SHAPES[8][1], 0, 1)
    assert (objects["w"][counts > 0, 0] == 3).any()


def test_object_hash_is_the_board_hash_at_the_corner():
    for pat in (BLOCK, BLINKER, GLIDER, BEEHIVE, ["O"], ["O.O", "...", "O.O"]):
        cells = P.as_cells(pat)
        for H, W in ((8, 8), (64, 64), (21, 33), (7, 5)):
            board = np.zeros((H, W), dtype=np.uint8)
            board[:cells.shape[0], :cells.shape[1]] = cells
            assert P.object_hash(pat) == M.board_hash(board), (pat, H, W)
    # every form as_cells takes, and dead outer rows and columns do not count
    assert P.object_hash(P.as_cells(GLIDER)) == P.object_hash(GLIDER) == P.object_hash("bo$2bo$3o!")
    assert P.object_hash(["....", ".OO.", ".OO.", "...."]) == P.object_hash(BLOCK)
    assert len({P.object_hash(p) for p in (BLOCK, BLINKER, GLIDER, BEEHIVE, ["O"])}) == 5


@pytest.mark.parametrize("at", [(0, 0), (5, 3), (62, 10), (63, 63), (63, 0), (17, 63)])
def test_a_block_has_one_hash_wherever_it_is(at):
    x, y = at
    board = np.zeros((64, 64), dtype=np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            board[(y + dy) % 64, (x + dx) % 64] = 1
    for label in (P.label_objects, OM.board_objects):
        recs = label(board, torus=True, reach=1)
        assert len(recs) == 1
        r = recs[0]
        assert (int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(r["population"])) == (x, y, 2, 2, 4)
        assert int(r["hash"]) == P.object_hash(BLOCK) and int(r["reserved"]) == 0


def test_object_table_covers_the_orientations():
    assert len(P.object_table({"block": [BLOCK]})) == 1
    assert len(P.object_table({"blinker": [BLINKER, ["O", "O", "O"]]})) == 2
    assert len(P.object_table({"blinker": [BLINKER]})) == 2  # the turned image is the other phase
    assert len(P.object_table({"glider": [GLIDER]})) == 8
    table = P.object_table({"block": [BLOCK], "beehive": [BEEHIVE]})
    assert table[(P.object_hash(BLOCK), 2, 2, 4)] == "block"
    assert table[(P.object_hash(BEEHIVE), 4, 3, 6)] == "beehive"
    assert table[(P.object_hash([".O.", "O.O", "O.O", ".O."]), 3, 4, 6)] == "beehive"
    with pytest.raises(ValueError):
        P.object_table({"a": [BLOCK], "b": [BLOCK]})


def test_label_objects_refuses_what_it_cannot_label():
    with pytest.raises(ValueError):
        P.label_objects(np.zeros((4, 4), dtype=np.uint8), reach=3)
    with pytest.raises(ValueError):
        P.label_objects(np.zeros((4, 65), dtype=np.uint8))
    assert len(P.label_objects(np.zeros((4, 4), dtype=np.uint8))) == 0
