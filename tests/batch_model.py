"""numpy model of the batch engine (gol_batch_*) -- test
infrastructure.  A board steps with the scalar C oracle (oracle.step_cells:
oracle.step_packed is only valid for torus widths that are multiples of 32);
the seed restates gol_batch_seed; populations and the settle rule come from
the model's own history; hashes are oracle.hash_packed of the packed cells."""
import numpy as np

from oracle import oracle as O

TOPOLOGY = {"torus": O.TORUS, "ref-clipped": O.REF_CLIPPED}
MASK64 = (1 << 64) - 1


def seed_rows(boards, W, H, seed):
    """uint64 [boards][H]: splitmix64 of counter k = i * H + y, low W bits."""
    k = np.arange(boards * H, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK64) + np.uint64(0x9E3779B97F4A7C15) * (k + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    if W < 64:
        z &= np.uint64((1 << W) - 1)
    return z.reshape(boards, H)


def unpack(rows, W):
    """uint64 [n][H] -> uint8 [n][H][W]."""
    r = np.asarray(rows, dtype=np.uint64)
    return ((r[..., None] >> np.arange(W, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def pack(cells):
    """uint8 [n][H][W] -> uint64 [n][H]."""
    c = np.asarray(cells, dtype=np.uint64)
    return (c << np.arange(c.shape[-1], dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def step_board(cells, topology="torus", rule=O.LIFE, vis=None):
    """One generation of one uint8 [H][W] board."""
    return O.step_cells(cells, TOPOLOGY[topology], rule, vis=vis)


def history(cells, gens, topology="torus", rule=O.LIFE, vis=None):
    """[gens + 1] boards: the board and its next `gens` generations."""
    out = [np.asarray(cells, dtype=np.uint8)]
    for _ in range(gens):
        out.append(step_board(out[-1], topology, rule, vis))
    return out


def settled_at(hist):
    """The smallest g in 2 .. len(hist) - 1 with hist[g] == hist[g - 2], or 0."""
    for g in range(2, len(hist)):
        if np.array_equal(hist[g], hist[g - 2]):
            return g
    return 0


def run_history(rows, W, gens, topology="torus", rule=O.LIFE, vis=None):
    """Every board of uint64 [n][H] `rows` advanced `gens` generations alone:
    (states uint64 [gens + 1][n][H], populations uint32 [n][gens], settled
    uint32 [n]); states[g] is every board after g generations."""
    cells = unpack(rows, W)
    n, H = cells.shape[0], cells.shape[1]
    states = np.zeros((gens + 1, n, H), dtype=np.uint64)
    pops = np.zeros((n, gens), dtype=np.uint32)
    settled = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        hist = history(cells[i], gens, topology, rule, vis)
        states[:, i] = pack(np.stack(hist))
        pops[i] = [int(h.sum()) for h in hist[1:]]
        settled[i] = settled_at(hist)
    return states, pops, settled


def run(rows, W, gens, topology="torus", rule=O.LIFE, vis=None):
    """(final rows uint64 [n][H], populations uint32 [n][gens], settled uint32 [n])."""
    states, pops, settled = run_history(rows, W, gens, topology, rule, vis)
    return states[-1], pops, settled


def board_hash(cells):
    """The state hash of one uint8 [H][W] board (row0 = 0)."""
    c = np.asarray(cells, dtype=np.uint8)
    return O.hash_packed(O.pack(c), c.shape[1])


def hashes(rows, W):
    return np.array([board_hash(c) for c in unpack(rows, W)], dtype=np.uint64)
