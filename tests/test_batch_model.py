"""CPU: the batch engine's numpy model (tests/batch_model.py) against the
independent restatements it must agree with, so the GPU tests compare the
kernels with a checked reference."""
import numpy as np
import pytest

import batch_model as M
from oracle import oracle as O


@pytest.mark.parametrize("W", [3, 5, 33, 63, 64])
def test_torus_step_equals_np_step(W):
    rng = np.random.default_rng(W)
    for H in (3, 7, 21):
        cells = rng.integers(0, 2, size=(H, W), dtype=np.uint8)
        for rule in (O.LIFE, (0x048, 0x00C), (0x001, 0x1FF)):
            a = cells
            for _ in range(4):
                want = O.np_step(a, O.TORUS, rule)
                a = M.step_board(a, "torus", rule)
                assert np.array_equal(a, want), (W, H, rule)


def test_clipped_step_equals_np_step():
    rng = np.random.default_rng(7)
    for (W, H, vis) in ((8, 8, None), (64, 64, (40, 50)), (63, 64, None), (32, 33, None)):
        cells = rng.integers(0, 2, size=(H, W), dtype=np.uint8)
        want = O.np_step(cells, O.REF_CLIPPED, O.LIFE, vis=vis)
        assert np.array_equal(M.step_board(cells, "ref-clipped", O.LIFE, vis), want), (W, H, vis)


def _board(W, H, live):
    c = np.zeros((H, W), dtype=np.uint8)
    for x, y in live:
        c[y, x] = 1
    return c


def test_settle_rule_blinker_block_glider():
    blinker = _board(12, 12, [(4, 5), (5, 5), (6, 5)])
    assert M.settled_at(M.history(blinker, 20)) == 2
    block = _board(12, 12, [(4, 4), (5, 4), (4, 5), (5, 5)])
    assert M.settled_at(M.history(block, 20)) == 2
    glider = _board(12, 12, [(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)])
    assert M.settled_at(M.history(glider, 20)) == 0
    # ... and through run(): rows in, settle words out
    rows = M.pack(np.stack([blinker, block, glider]))
    final, pops, settled = M.run(rows, 12, 20)
    assert settled.tolist() == [2, 2, 0]
    assert pops[:, -1].tolist() == [3, 4, 5]
    assert np.array_equal(final[1], rows[1])


@pytest.mark.parametrize("W", [3, 8, 33, 63, 64])
def test_seed_rows_are_masked_to_width(W):
    rows = M.seed_rows(5, W, 7, 0xC0FFEE)
    assert rows.shape == (5, 7) and rows.dtype == np.uint64
    if W < 64:
        assert int(rows.max()) < (1 << W)
    # the low W bits of the full 64-bit output, restated with Python integers
    want = []
    for k in range(35):
        z = (0xC0FFEE + 0x9E3779B97F4A7C15 * (k + 1)) & M.MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M.MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M.MASK64
        want.append((z ^ (z >> 31)) & ((1 << W) - 1))
    assert rows.reshape(-1).tolist() == want


def test_pack_unpack_and_hash_agree_with_np_hash():
    rng = np.random.default_rng(3)
    for W in (7, 8, 33, 64):
        cells = rng.integers(0, 2, size=(2, 9, W), dtype=np.uint8)
        rows = M.pack(cells)
        assert np.array_equal(M.unpack(rows, W), cells)
        for i in range(2):
            assert int(M.hashes(rows, W)[i]) == O.np_hash(O.pack(cells[i]), W)
