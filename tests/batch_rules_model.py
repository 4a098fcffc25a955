"""numpy model of a batch with per-board rules (gol_rules_batch_*; DESIGN.md
section 5k) -- test infrastructure.  Board i steps under rule i, alone, by
batch_model.run_history on that one board with that rule: the model knows
nothing of waves, lanes or launches.  The rule list is the same for every
test: seven named rules cycled by board index, then words drawn from
splitmix64 of the index."""
import numpy as np

import batch_model as M
from gameoflife.rules import rule_word

MASK64 = (1 << 64) - 1
WORD_BITS = 0x01FF01FF

# cycled by board index; B0/S012345678 has a birth on 0 neighbours, B/S kills everything,
# B012345678/S012345678 fills the board
NAMED = ("life", "B36/S23", "B0/S012345678", "ref-literal", "ref-effective", "B/S", "B012345678/S012345678")


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def rule_words(boards):
    """uint32 [boards]: board i's rule word -- the named rules for i < 7, then splitmix64(i) & 0x01FF01FF."""
    return np.array([rule_word(NAMED[i]) if i < len(NAMED) else splitmix64(i) & WORD_BITS for i in range(boards)],
                    dtype=np.uint32)


def named_words(boards):
    """uint32 [boards]: the seven named rules only, cycled by board index."""
    return np.array([rule_word(NAMED[i % len(NAMED)]) for i in range(boards)], dtype=np.uint32)


def masks(word):
    """(birth, survive) of a rule word, as the oracle takes a rule."""
    word = int(word)
    return word & 0x1FF, (word >> 16) & 0x1FF


def run_history(rows, W, gens, words, topology="torus", vis=None):
    """batch_model.run_history with board i under words[i]: (states uint64
    [gens + 1][n][H], populations uint32 [n][gens], settled uint32 [n])."""
    rows = np.asarray(rows, dtype=np.uint64)
    n, H = rows.shape
    assert len(words) == n
    states = np.zeros((gens + 1, n, H), dtype=np.uint64)
    pops = np.zeros((n, gens), dtype=np.uint32)
    settled = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        s, p, t = M.run_history(rows[i:i + 1], W, gens, topology, masks(words[i]), vis)
        states[:, i], pops[i], settled[i] = s[:, 0], p[0], t[0]
    return states, pops, settled


def run(rows, W, gens, words, topology="torus", vis=None):
    """(final rows uint64 [n][H], populations uint32 [n][gens], settled uint32 [n])."""
    states, pops, settled = run_history(rows, W, gens, words, topology, vis)
    return states[-1], pops, settled
