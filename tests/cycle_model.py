"""numpy model of cycle detection on a batch (gol_cycle_step; DESIGN.md section
5g) -- test infrastructure next to tests/batch_model.py, whose step it uses.
Brent's algorithm on the fixed schedule of include/gol.h: with x_g the board
after g generations of a call, snapshots at t_k = 2^k - 1, x_g compared with
x_{t_k} for t_k < g <= t_{k+1}; seen is the first g that matches and period =
seen - t_k.  cycle_of follows the schedule literally, seen_for is the closed
form."""
import numpy as np

import batch_model as M
from oracle import oracle as O


def snapshot_generation(g):
    """The t_k that generation g >= 1 of a call is compared with."""
    assert g >= 1
    return (1 << (g.bit_length() - 1)) - 1


def seen_for(mu, lam):
    """seen of a board that enters a cycle of period lam after mu generations:
    t_k + lam for the smallest k with t_k >= mu and 2^k >= lam."""
    k = 0
    while (1 << k) - 1 < mu or (1 << k) < lam:
        k += 1
    return (1 << k) - 1 + lam


def schedule_of(mu, lam, limit):
    """(period, seen) of the abstract sequence x_g = g for g < mu, mu + (g - mu)
    % lam after, by the literal schedule over generations 1 .. limit."""
    def state(g):
        return g if g < mu else mu + (g - mu) % lam
    snap, tk = state(0), 0
    for g in range(1, limit + 1):
        if state(g) == snap:
            return g - tk, g
        if g & (g + 1) == 0:
            snap, tk = state(g), g
    return 0, 0


def run_board(cells, N, topology="torus", rule=O.LIFE, vis=None):
    """One uint8 [H][W] board advanced N generations: (x_N, period, seen)."""
    x = np.asarray(cells, dtype=np.uint8)
    snap, tk = x, 0
    period = seen = 0
    for g in range(1, N + 1):
        x = M.step_board(x, topology, rule, vis)
        if seen == 0 and np.array_equal(x, snap):
            period, seen = g - tk, g
        if g & (g + 1) == 0:
            snap, tk = x, g
    return x, period, seen


def cycle_of(cells, N, topology="torus", rule=O.LIFE, vis=None):
    """(period, seen) of one board over a call of N generations; (0, 0): none."""
    return run_board(cells, N, topology, rule, vis)[1:]


def run(rows, W, N, topology="torus", rule=O.LIFE, vis=None):
    """Every board of uint64 [n][H] `rows` advanced N generations alone:
    (final rows uint64 [n][H], period uint32 [n], seen uint32 [n])."""
    cells = M.unpack(rows, W)
    n = cells.shape[0]
    final = np.zeros((n, cells.shape[1]), dtype=np.uint64)
    period = np.zeros(n, dtype=np.uint32)
    seen = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        x, period[i], seen[i] = run_board(cells[i], N, topology, rule, vis)
        final[i] = M.pack(x)
    return final, period, seen


# Known patterns, as O/. rows placed on a dead board.
BLOCK = ["OO", "OO"]
BLINKER = ["OOO"]
GLIDER = [".O.", "..O", "OOO"]
PULSAR = ["..OOO...OOO..", ".............", "O....O.O....O", "O....O.O....O", "O....O.O....O", "..OOO...OOO..",
          ".............", "..OOO...OOO..", "O....O.O....O", "O....O.O....O", "O....O.O....O", ".............",
          "..OOO...OOO.."]
PENTADECATHLON = ["..O....O..", "OO.OOOO.OO", "..O....O.."]


def place(W, H, pattern=(), x0=None, y0=None):
    """uint8 [H][W]: `pattern` (rows of O / .) on a dead board, centred unless placed."""
    c = np.zeros((H, W), dtype=np.uint8)
    if not pattern:
        return c
    ph, pw = len(pattern), max(len(r) for r in pattern)
    x0 = (W - pw) // 2 if x0 is None else x0
    y0 = (H - ph) // 2 if y0 is None else y0
    for dy, row in enumerate(pattern):
        for dx, ch in enumerate(row):
            if ch == "O":
                c[y0 + dy, x0 + dx] = 1
    return c
