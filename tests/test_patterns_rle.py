"""CPU: gameoflife.patterns (RLE and O/. rows) and the numpy region model
the GPU window tests compare against (tests/region_model.py)."""
import numpy as np
import pytest

import region_model as M
from gameoflife import patterns as P
from known_patterns import GOSPER_GUN_ROWS

GOSPER_RLE = ("24bo11b$22bobo11b$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o14b$2o8bo3bob2o4bobo11b$"
              "10bo5bo7bo11b$11bo3bo20b$12b2o!")
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)


def test_gosper_gun_rle_is_the_known_pattern():
    p = P.parse_rle(GOSPER_RLE)
    assert (p.width, p.height, p.rule) == (36, 9, None)
    np.testing.assert_array_equal(p.cells, P.from_rows(GOSPER_GUN_ROWS))
    assert int(p.cells.sum()) == 36


def test_glider_rle():
    p = P.parse_rle("bob$2bo$3o!")
    np.testing.assert_array_equal(p.cells, GLIDER)


def test_header_comments_and_line_breaks():
    text = "#N Glider\n#C a comment with x = 1, y = 1\nx = 3, y = 3, rule = B3/S23\nbob$2b\no$3o!\nignored after the end"
    p = P.parse_rle(text)
    assert p.rule == "B3/S23" and (p.width, p.height) == (3, 3)
    np.testing.assert_array_equal(p.cells, GLIDER)
    # the header's extents win over the body's: trailing dead columns and rows
    q = P.parse_rle("x = 5, y = 4\nbob$2bo$3o!")
    assert q.cells.shape == (4, 5) and q.rule is None
    np.testing.assert_array_equal(q.cells[:3, :3], GLIDER)
    assert q.cells.sum() == 5


def test_row_counts_skip_rows():
    p = P.parse_rle("o3$2o!")
    assert p.cells.shape == (4, 2)
    np.testing.assert_array_equal(p.cells, [[1, 0], [0, 0], [0, 0], [1, 1]])


@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (7, 33), (33, 7), (70, 70)])
@pytest.mark.parametrize("fill", ["random", "sparse", "empty"])
def test_rle_round_trip(shape, fill):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    if fill == "random":
        c = (rng.random(shape) < 0.5).astype(np.uint8)
    elif fill == "sparse":  # empty rows (also first and last) and trailing dead columns
        c = (rng.random(shape) < 0.1).astype(np.uint8)
        c[::3] = 0
        c[-1] = 0
        c[:, shape[1] // 2:] = 0
    else:
        c = np.zeros(shape, dtype=np.uint8)
    text = P.to_rle(c)
    assert all(len(line) <= 70 for line in text.splitlines())
    back = P.parse_rle(text)
    assert (back.height, back.width) == shape and back.rule == "B3/S23"
    np.testing.assert_array_equal(back.cells, c)


@pytest.mark.parametrize("text", ["3x!", "2o$3", "bo$0o!", "x = 2, y = 2\n3o!", "x = 3, y = 1\no$o!", "2!", "o?o!"])
def test_garbage_raises(text):
    with pytest.raises(ValueError):
        P.parse_rle(text)


def test_from_rows_and_as_cells():
    np.testing.assert_array_equal(P.from_rows([".O.", "..O", "OOO"]), GLIDER)
    np.testing.assert_array_equal(P.from_rows(["O", "..O"]), [[1, 0, 0], [0, 0, 1]])
    with pytest.raises(ValueError):
        P.from_rows(["O.x"])
    for form in ("bob$2bo$3o!", [".O.", "..O", "OOO"], GLIDER, P.parse_rle("bob$2bo$3o!")):
        np.testing.assert_array_equal(P.as_cells(form), GLIDER)


# ---- the region model itself ---------------------------------------------------

def _board(H, W, seed):
    return (np.random.default_rng(seed).random((H, W)) < 0.5).astype(np.uint8)


@pytest.mark.parametrize("x0,y0,w,h", [(0, 0, 1, 1), (5, 1, 33, 3), (62, 6, 5, 5), (5, 0, 64, 2), (63, 0, 1, 8)])
def test_model_copy_then_read_returns_the_pattern(x0, y0, w, h):
    b = _board(8, 64, 1)
    p = _board(h, w, 2)
    out = M.write_region(b, x0, y0, p, "copy")
    np.testing.assert_array_equal(M.read_region(out, x0, y0, w, h), p)
    # nothing outside the window moved
    mask = np.ones_like(b)
    mask = M.write_region(mask, x0, y0, np.ones((h, w), dtype=np.uint8), "clear")
    np.testing.assert_array_equal(out * mask, b * mask)
    assert int(mask.sum()) == b.size - w * h


def test_model_truth_tables():
    old = np.array([[0, 0, 1, 1]], dtype=np.uint8)
    pat = np.array([[0, 1, 0, 1]], dtype=np.uint8)
    want = {"copy": [0, 1, 0, 1], "or": [0, 1, 1, 1], "xor": [0, 1, 1, 0], "clear": [0, 0, 1, 0]}
    for mode in M.MODES:
        b = np.zeros((3, 8), dtype=np.uint8)
        b[1, 6:8] = old[0, :2]  # the window wraps in x
        b[1, 0:2] = old[0, 2:]
        out = M.write_region(b, 6, 1, pat, mode)
        np.testing.assert_array_equal(M.read_region(out, 6, 1, 4, 1)[0], want[mode], err_msg=mode)


def test_model_clipped_refuses_wrap_and_census():
    b = np.zeros((7, 7), dtype=np.uint8)
    with pytest.raises(AssertionError):
        M.write_region(b, 5, 0, np.ones((1, 3), dtype=np.uint8), torus=False)
    assert M.census(b) == {"population": 0, "bbox": None}
    b[2, 5] = b[6, 1] = 1
    assert M.census(b, row0=10) == {"population": 2, "bbox": (1, 12, 5, 16)}
