"""An independent, cell-level model of a batch's soups (include/gol.h
gol_soup_batch*), and the shapes the CPU and the GPU
tests hold the product to.

Per window cell the orbit under the group is enumerated from the maps as the
header states them and its lexicographic minimum (v, u) taken; t(u) is summed
from the eight mixes with Python integers.  No bit-sliced comparator, no
fundamental-domain masks, no steps: nothing of the product's plan."""
import functools

import numpy as np

M64 = (1 << 64) - 1
SEED = 0x50C1A1

SYMMETRIES = ("C1", "C2", "C4", "D2_X", "D2_Y", "D2_DIAG", "D4_PLUS", "D4_DIAG", "D8")
SQUARE = ("C4", "D2_DIAG", "D4_DIAG", "D8")  # the groups with a T or an R: they need w == h
ANY = tuple(s for s in SYMMETRIES if s not in SQUARE)


def mix(seed, c):
    z = (seed + 0x9E3779B97F4A7C15 * (c + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _e(u, v, w, h):
    return u, v


def _x(u, v, w, h):
    return w - 1 - u, v


def _y(u, v, w, h):
    return u, h - 1 - v


def _xy(u, v, w, h):
    return w - 1 - u, h - 1 - v


def _t(u, v, w, h):
    return v, u


def _txy(u, v, w, h):
    return _t(*_xy(u, v, w, h), w, h)


def _r(u, v, w, h):
    return h - 1 - v, u


def _r3(u, v, w, h):
    return _r(*_r(*_r(u, v, w, h), w, h), w, h)


GROUPS = {
    "C1": (_e,), "C2": (_e, _xy), "C4": (_e, _r, _xy, _r3), "D2_X": (_e, _x), "D2_Y": (_e, _y), "D2_DIAG": (_e, _t),
    "D4_PLUS": (_e, _x, _y, _xy), "D4_DIAG": (_e, _t, _xy, _txy), "D8": (_e, _x, _y, _xy, _t, _txy, _r, _r3),
}


@functools.lru_cache(maxsize=None)
def t_row(seed, soup, v):
    """t(u) for u in 0 .. 63 of window row v of soup number `soup`."""
    z = [mix(seed, (((soup * 64 + v) & M64) * 8 + j) & M64) for j in range(8)]
    return tuple(sum(((z[j] >> u) & 1) << j for j in range(8)) for u in range(64))


@functools.lru_cache(maxsize=None)
def canonical(symmetry, w, h):
    """{(u, v): (u*, v*)}: the member of each cell's orbit with the smallest (v', u')."""
    out = {}
    for v in range(h):
        for u in range(w):
            vs, us = min((b, a) for a, b in (g(u, v, w, h) for g in GROUPS[symmetry]))
            out[u, v] = (us, vs)
    return out


def distinct_expected(symmetry, w, h, n):
    """Whether n soups of this window should all differ: a soup has one free
    cell per orbit, so two of n fair ones coincide with probability about
    n^2 / 2^(orbits + 1) -- asked for where that is below 1 / 128."""
    orbits = len(set(canonical(symmetry, w, h).values()))
    return 2 ** orbits >= 64 * n * n


def board(width, height, seed, soup, window, density, symmetry):
    """uint64 [height]: the board that holds soup number `soup`."""
    x, y, w, h = (0, 0, width, height) if window is None else window
    canon = canonical(symmetry, w, h)
    rows = [0] * height
    for v in range(h):
        r = 0
        for u in range(w):
            us, vs = canon[u, v]
            r |= (1 if t_row(seed, soup & M64, vs)[us] < density else 0) << u
        rows[y + v] = r << x
    return np.array(rows, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def boards(width, height, seed, index0, n, window, density, symmetry):
    """uint64 [n][height], read-only: board b holds soup number index0 + b (mod 2^64)."""
    out = np.stack([board(width, height, seed, (index0 + b) & M64, window, density, symmetry) for b in range(n)])
    out.setflags(write=False)
    return out


def window_cells(rows, window):
    """uint8 [n][h][w]: the window's cells of uint64 [n][H] rows."""
    x, y, w, h = window
    r = np.asarray(rows, dtype=np.uint64)[:, y:y + h]
    return ((r[:, :, None] >> (np.uint64(x) + np.arange(w, dtype=np.uint64))) & np.uint64(1)).astype(np.uint8)


def invariant(cells, symmetry):
    """Whether uint8 [n][h][w] windows are unchanged by every element of the
    group, by numpy flips and transposes: independent of the maps above."""
    c = np.asarray(cells)
    fx, fy, tr = (lambda a: a[:, :, ::-1]), (lambda a: a[:, ::-1, :]), (lambda a: a.transpose(0, 2, 1))
    rot = lambda a: fx(tr(a))  # noqa: E731  (a quarter turn)
    images = {
        "C1": [], "C2": [fx(fy(c))], "D2_X": [fx(c)], "D2_Y": [fy(c)], "D4_PLUS": [fx(c), fy(c), fx(fy(c))],
    }
    if c.shape[1] == c.shape[2]:
        images.update({
            "C4": [rot(c), rot(rot(c)), rot(rot(rot(c)))], "D2_DIAG": [tr(c)],
            "D4_DIAG": [tr(c), fx(fy(c)), tr(fx(fy(c)))],
            "D8": [fx(c), fy(c), fx(fy(c)), tr(c), tr(fx(fy(c))), rot(c), rot(rot(rot(c)))],
        })
    return all(np.array_equal(c, i) for i in images[symmetry])


# The shapes both test files use: (width, height, topology, vis, boards) and per shape the
# (window, density, symmetry) cases.  Each reaches another path or seam of the kernel:
#   64 x 64 torus, 5 boards    one board per wave; whole-board windows (the wide transpose, bit 63), the
#                              conventional 16 x 16 (the narrow transpose), an odd 15 x 15 at the left edge and
#                              the last rows, and 20 x 9 touching bit 63 and the last row
#   40 x 20 torus, 7 boards    three boards per wave, four idle lanes, a last wave with one board: the lane seam;
#                              33 x 20 crosses the dword boundary
#   8 x 8 clipped, 130 boards  eight boards per wave, a third workgroup's worth of waves, 1 x 1
def _cases():
    big = (64, 64, "torus", None, 5)
    out = {big: [(None, 128, s) for s in SYMMETRIES] + [(None, d, s) for d in (1, 255) for s in ("C1", "D8")]}
    out[big] += [(win, 128, s) for win in ((24, 24, 16, 16), (0, 49, 15, 15)) for s in SYMMETRIES]
    out[big] += [((44, 55, 20, 9), 128, s) for s in ANY]
    mid = (40, 20, "torus", None, 7)
    out[mid] = [((31, 11, 9, 9), 128, s) for s in ("D8", "D4_DIAG", "C4")] + [((3, 0, 33, 20), 128, "D4_PLUS")]
    small = (8, 8, "ref-clipped", (7, 7), 130)
    out[small] = [((0, 0, 8, 8), 128, "D8"), ((0, 0, 7, 7), 128, "C4"), ((5, 2, 1, 1), 128, "C1")]
    return out


SHAPES = _cases()
CASES = [(shape, case) for shape, cases in SHAPES.items() for case in cases]


def case_id(sc):
    (W, H, topo, _, n), (win, density, sym) = sc
    where = "whole" if win is None else "%dx%d@%d,%d" % (win[2], win[3], win[0], win[1])
    return f"{W}x{H}-{topo}-{n}-{where}-d{density}-{sym}"
