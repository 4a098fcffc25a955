"""Brute-force numpy model of gol_find (include/gol.h "Pattern search") on an
unpacked [H][W] cell array: one np.roll of the board (torus) or one dead-padded
copy (clipped) per cared cell.  Independent of gameoflife.patterns' matcher."""
import numpy as np


def match_map(board, cells, care, torus):
    """bool [H][W]: anchor (x, y) matches iff board cell (x + k, y + i) equals
    pattern cell (k, i) for every cared (k, i); coordinates wrap on a torus,
    cells beyond a clipped board read dead."""
    board = np.asarray(board, dtype=np.uint8)
    H, W = board.shape
    ph, pw = np.asarray(cells).shape
    ok = np.ones((H, W), dtype=bool)
    if not torus:
        padded = np.zeros((H + ph, W + pw), dtype=np.uint8)
        padded[:H, :W] = board
    for i in range(ph):
        for k in range(pw):
            if not care[i][k]:
                continue
            if torus:
                seen = np.roll(board, (-i, -k), axis=(0, 1))
            else:
                seen = padded[i:i + H, k:k + W]
            ok &= seen == (1 if cells[i][k] else 0)
    return ok


def window_mask(H, W, x0, y0, w, h, torus):
    """bool [H][W]: the anchors of the window (x0, y0, w, h)."""
    ys, xs = np.arange(H), np.arange(W)
    if torus:
        in_y, in_x = (ys - y0) % H < h, (xs - x0) % W < w
    else:
        in_y, in_x = (ys >= y0) & (ys < y0 + h), (xs >= x0) & (xs < x0 + w)
    return in_y[:, None] & in_x[None, :]


def find(board, cells, care, torus, x0=0, y0=0, w=None, h=None):
    """int64 [n][2] of (x, y): the matches among the window's anchors, sorted
    by (y, x)."""
    H, W = np.asarray(board).shape
    w = W if w is None else w
    h = H if h is None else h
    ok = match_map(board, cells, care, torus) & window_mask(H, W, x0, y0, w, h, torus)
    ys, xs = np.nonzero(ok)  # row-major: sorted by (y, x)
    return np.stack([xs, ys], axis=1).astype(np.int64)


def examined_rows(H, row0, rows, ph, torus):
    """The anchor rows a shard [row0, row0 + rows) examines: those it owns
    whose pattern rows are all its own, or off the end of a clipped board."""
    out = []
    for y in range(row0, row0 + rows):
        ok = True
        for i in range(ph):
            r = y + i
            if torus:
                r %= H
            elif r >= H:
                continue
            ok = ok and row0 <= r < row0 + rows
        if ok:
            out.append(y)
    return out
