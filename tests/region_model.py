"""The truth for gol_read_region / gol_write_region / gol_census: a numpy
model on an unpacked [H][W] cell array, with modular fancy indexing for the
torus.  Not a test module; tests/test_patterns_rle.py checks the model itself."""
import numpy as np

MODES = ("copy", "or", "xor", "clear")


def _index(board, x0, y0, w, h, torus):
    H, W = board.shape
    assert 1 <= w <= W and 1 <= h <= H and 0 <= x0 < W and 0 <= y0 < H
    if not torus:
        assert x0 + w <= W and y0 + h <= H
    ys = (y0 + np.arange(h)) % H
    xs = (x0 + np.arange(w)) % W
    return np.ix_(ys, xs)


def read_region(board, x0, y0, w, h, torus=True):
    return board[_index(board, x0, y0, w, h, torus)].copy()


def write_region(board, x0, y0, pattern, mode="copy", torus=True):
    """A new board: `pattern` ([h][w] cells) combined into the window."""
    p = np.asarray(pattern, dtype=np.uint8) & 1
    h, w = p.shape
    ix = _index(board, x0, y0, w, h, torus)
    out = board.copy()
    old = out[ix]
    out[ix] = {"copy": p, "or": old | p, "xor": old ^ p, "clear": old & (1 - p)}[mode]
    return out


def census(board, row0=0):
    """{"population", "bbox"} of rows given as a [rows][W] cell array whose
    first row is global row `row0` (bbox (min_x, min_y, max_x, max_y), None
    when nothing is alive)."""
    ys, xs = np.nonzero(board)
    if ys.size == 0:
        return {"population": 0, "bbox": None}
    return {"population": int(ys.size),
            "bbox": (int(xs.min()), int(ys.min()) + row0, int(xs.max()), int(ys.max()) + row0)}
