"""GPU: the entry points that share a context's per-generation accumulators
(step with hashes, with populations, with both, with neither; hash()), one
after the other on one context and across the step's 1024-generation chunk
boundary, against the CPU oracle.

Reference: oracle.run_packed for the hashes and the final board, the board
stepped with oracle.step_packed and its bits counted for the populations (as
in tests/test_gpu_population.py).  Boards: a 128 x 16 B3/S23 torus (pair
layout, 4 words per row), the same torus as a two-shard in-process group (8
rows each) and a 70 x 9 clipped board.  Seeds, checked on the oracle: torus
seed 1412 never repeats a state in the 2077 generations of the sequence (92
live cells at the end); clipped seed 1370 is the longest-lived of seeds 1 ..
1499 (309 distinct states, 26 live cells at the end)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (generations, hashes, populations); None: hash()
SEQUENCE = [(5, True, True), (3, True, False), None, (2, False, True), (1030, True, False), (1030, True, True),
            (7, False, False), None]
TOTAL = sum(s[0] for s in SEQUENCE if s)


def popcount(packed):
    return int(np.unpackbits(np.ascontiguousarray(packed).view(np.uint8)).sum())


@functools.lru_cache(maxsize=None)
def reference(kind):
    """(board, final board, hashes, populations) over the whole sequence."""
    if kind == "torus":
        W, topo = 128, O.TORUS
        board = O.seed_packed(W, 16, 1412)
    else:
        W, topo = 70, O.REF_CLIPPED
        board = O.pack((np.random.default_rng(1370).random((9, W)) < 0.5).astype(np.uint8))
    final, hashes = O.run_packed(board, W, TOTAL, topo, O.LIFE)
    pops = np.zeros(TOTAL, dtype=np.uint64)
    cur = board
    for g in range(TOTAL):
        cur = O.step_packed(cur, W, topo, O.LIFE)
        pops[g] = popcount(cur)
    assert np.array_equal(cur, final) and pops[-1] > 0
    for a in (board, final, hashes, pops):
        a.setflags(write=False)
    return board, final, hashes, pops


def run_sequence(target, final, hashes, pops):
    """The sequence on `target` (an engine or a shard group at epoch 0)."""
    epoch = 0
    for k, item in enumerate(SEQUENCE):
        if item is None:
            assert target.hash() == int(hashes[epoch - 1]), f"step {k + 1}: hash() at epoch {epoch}"
            continue
        n, with_hashes, with_pops = item
        out = target.step(n, hashes=with_hashes, populations=with_pops)
        got_h, got_p = out if with_hashes and with_pops else (out, None) if with_hashes else (None, out)
        for name, got, want in (("hashes", got_h, hashes), ("populations", got_p, pops)):
            if got is None:
                continue
            want = want[epoch:epoch + n]
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (f"step {k + 1} ({n} generations from epoch {epoch}): {name} differ first at "
                                   f"generation {bad[0] + 1}: {got[bad[0]]} != {want[bad[0]]}")
        epoch += n
        assert target.epoch == epoch
    bad = np.argwhere(target.snapshot() != final)
    assert bad.size == 0, f"first wrong word (row, col) {tuple(bad[0])}"


@pytest.mark.parametrize("kind", ["torus", "clipped"])
def test_one_context(gpu, kind):
    from gameoflife.engine import GolEngine
    board, final, hashes, pops = reference(kind)
    H, W = board.shape[0], 128 if kind == "torus" else 70
    with GolEngine(W, H, topology="torus" if kind == "torus" else "ref-clipped") as e:
        e.load(board)
        run_sequence(e, final, hashes, pops)


def test_two_shard_group(gpu):
    from gameoflife.engine import GolEngine, ShardGroup
    board, final, hashes, pops = reference("torus")
    shards = []
    for r0 in (0, 8):
        e = GolEngine(128, 16, row0=r0, rows=8)
        e.load(board[r0:r0 + 8])
        shards.append(e)
    g = ShardGroup(shards)
    try:
        run_sequence(g, final, hashes, pops)
    finally:
        g.close()
        for s in shards:
            s.close()
