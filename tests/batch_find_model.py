"""Bit-parallel numpy model of the batch pattern search (gol_find_batch;
DESIGN.md section 5h) on uint64 rows.  It restates the kernel's arithmetic --
the rotate within `width` written as two shifts that never reach 64, the zero
fill of a clipped board, the inversion for dead pattern cells, the row wrap
inside a board -- where tests/find_model.py is the cell-level definition it is
checked against."""
import numpy as np

U = np.uint64
ALL = U(0xFFFFFFFFFFFFFFFF)


def wmask(width):
    return ALL if width >= 64 else U((1 << width) - 1)


def pack_row_bits(cells):
    """uint8 [h][w] -> uint64 [h], bit k = column k."""
    c = np.asarray(cells, dtype=np.uint8)
    return ((c != 0).astype(U) << np.arange(c.shape[1], dtype=U)).sum(axis=1, dtype=U)


def shift_k(rows, k, width, torus):
    """Board column x + k at bit x: the rotate right by k within width, or the
    zero-filling shift.  Bits at x >= width of the result are unspecified."""
    sh = rows >> U(k)
    if torus:
        sh = sh | ((rows << U(1)) << U(width - 1 - k))  # width - k may be 64: 1 and width - 1 - k never are
    return sh


def match_rows(rows, width, cells, care, torus):
    """rows: uint64 [n][H] boards.  cells, care: uint8 [ph][pw].  uint64 [n][H]:
    bit x of [b][y] set iff anchor (x, y) of board b matches."""
    rows = np.asarray(rows, dtype=U)
    n, H = rows.shape
    pcare = pack_row_bits(care)
    pcells = pack_row_bits(cells) & pcare
    cand = np.full((n, H), wmask(width), dtype=U)
    for i in range(len(pcare)):
        if pcare[i] == 0:
            continue
        if torus:
            r = np.roll(rows, -i, axis=1)  # row (y + i) mod H of the same board
        else:
            r = np.zeros_like(rows)
            r[:, :H - i] = rows[:, i:]     # dead past the board's last row
        for k in range(64):
            if not (int(pcare[i]) >> k) & 1:
                continue
            inv = U(0) if (int(pcells[i]) >> k) & 1 else ALL
            cand &= shift_k(r, k, width, torus) ^ inv
    return cand


def counts(planes):
    """uint64 [n][H] match rows -> uint32 [n] matches per board."""
    p = np.asarray(planes, dtype=U)
    return np.unpackbits(p.view(np.uint8).reshape(p.shape[0], -1), axis=1).sum(axis=1).astype(np.uint32)
