"""The truth for gol_density: a numpy model on an unpacked [H][W] cell array,
built on region_model.read_region.  Not a test module;
tests/test_density_model.py checks the model itself."""
import numpy as np

import region_model as M


def density(board, x0, y0, w, h, tile, torus=True, row0=0, rows=None):
    """uint32 [ceil(h / tile)][ceil(w / tile)]: the live cells per tile x tile
    block of the window, tiles anchored at the window origin, counting only
    the cells whose board row lies in [row0, row0 + rows) (a shard's rows;
    `rows` None: to the end of the board)."""
    H = board.shape[0]
    rows = H - row0 if rows is None else rows
    win = M.read_region(board, x0, y0, w, h, torus).astype(np.uint32)
    ys = (y0 + np.arange(h)) % H
    win[(ys < row0) | (ys >= row0 + rows)] = 0
    th, tw = -(-h // tile), -(-w // tile)
    padded = np.zeros((th * tile, tw * tile), dtype=np.uint32)
    padded[:h, :w] = win
    return padded.reshape(th, tile, tw, tile).sum(axis=(1, 3), dtype=np.uint32)
