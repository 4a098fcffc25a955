"""CPU: the bit-parallel model of the batch pattern search
(tests/batch_find_model.py) against the cell-level definition
(tests/find_model.py) on every shape and pattern list the GPU tests use, the
64-bit shift's edge cases, and patterns.orientations."""
import numpy as np
import pytest

import batch_find_cases as K
import batch_find_model as B
import batch_model as M
import find_model as F
from gameoflife import patterns as P


@pytest.mark.parametrize("case", K.SHAPES, ids=K.shape_id)
@pytest.mark.parametrize("which", ["soup", "ash", "nine"])
def test_model_equals_the_cell_level_definition(case, which):
    shape, boards, gens = case
    if which == "ash" and case not in K.SHAPES[K.ASH_SHAPES]:
        return
    gens = gens if which == "ash" else 0
    patterns, counts, planes = K.reference_for(shape, boards, gens, which)
    rows = K.boards_after(shape, boards, gens)
    for p, (cells, care) in enumerate(patterns):
        got = B.match_rows(rows, shape[0], cells, care, shape[2] == "torus")
        assert np.array_equal(got, planes[p]), (p, cells.shape)
        assert np.array_equal(B.counts(got), counts[:, p])
    # what the GPU cases rely on: an all-zero answer, or an all-ones one, cannot pass
    assert (counts > 0).any() and (counts == 0).any()


def test_fixture_facts_of_the_seeded_boards():
    """What the GPU cases exercise, asserted on the cell-level model."""
    for case in K.SHAPES:
        shape, boards, _ = case
        patterns, counts, _ = K.reference_for(shape, boards, 0, "soup")
        rows = K.boards_after(shape, boards, 0)
        assert np.array_equal(counts[:, 0], B.counts(rows))  # the 1 x 1 live cell counts the population
        assert counts[:, 1].sum() >= 67 and 9 <= counts[:, 1].max() <= 282  # the bare block on the raw soup
        whole = [p for p, (c, _) in enumerate(patterns) if c.shape == (shape[1], shape[0])][-1]
        assert counts[0, whole] >= 1  # board 0 itself, at its anchor (0, 0)
    ash = {K.shape_id(c): K.reference_for(c[0], c[1], c[2], "ash")[1] for c in K.SHAPES[K.ASH_SHAPES]}
    assert int(ash["64x64-torus-5b"][:, 0].sum()) == 48
    assert int(ash["64x64-ref-clipped-vis64x63-5b"][:, 0].sum()) == 47
    blocks = ash["33x21-torus-13b"][:, 0]
    assert int(blocks.sum()) == 16 and int((blocks == 0).sum()) == 4


def _against_cells(width, height, cells, care, torus, n=6, seed=7):
    rng = np.random.default_rng(seed)
    boards = rng.integers(0, 2, size=(n, height, width), dtype=np.uint8)
    rows = M.pack(boards)
    got = B.match_rows(rows, width, cells, care, torus)
    want = M.pack(np.array([F.match_map(b, cells, care, torus) for b in boards], dtype=np.uint8))
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("torus", [True, False])
def test_shift_edge_cases(torus):
    def single(width, k, bit):
        cells = np.zeros((1, k + 1), dtype=np.uint8)
        care = np.zeros((1, k + 1), dtype=np.uint8)
        cells[0, k], care[0, k] = bit, 1
        return cells, care
    for bit in (0, 1):
        for k in (0, 63):  # width 64: the rotate's left part shifts by 64 - k = 64 at k = 0
            assert _against_cells(64, 5, *single(64, k, bit), torus).any()
        assert _against_cells(33, 4, *single(33, 32, bit), torus).any()  # k = 32: the upper dword alone
        for k in (0, 1, 2):
            _against_cells(3, 3, *single(3, k, bit), torus)
    # cared columns on both sides of bit 31 / 32 on width 33
    cells = np.zeros((2, 33), dtype=np.uint8)
    care = np.zeros((2, 33), dtype=np.uint8)
    cells[0, [30, 32]], care[:, 30:33] = 1, 1
    _against_cells(33, 4, cells, care, torus, n=40)
    # k = 0 on width 64 is the row itself
    rows = np.array([[0x8000000000000001, 0x0123456789ABCDEF]], dtype=np.uint64)
    assert np.array_equal(B.shift_k(rows, 0, 64, torus) & B.wmask(64), rows)
    if torus:
        assert B.shift_k(rows, 63, 64, True)[0, 0] == np.uint64(0x0000000000000003)


def test_orientations_counts():
    n = lambda rows, care=None: len(P.orientations(P.from_rows(rows), care))  # noqa: E731
    assert n(K.BLOCK) == 1 and n(K.BLINKER_H) == 2 and n(K.GLIDER) == 8 and n(K.BEEHIVE) == 2
    care = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0]], dtype=np.uint8)  # asymmetric under all 8
    images = P.orientations(np.zeros((3, 3), dtype=np.uint8), care)
    assert len(images) == 8
    # the pattern itself comes first, and every image keeps its cared cells
    first = P.orientations(P.from_rows(K.GLIDER))[0]
    assert np.array_equal(first[0], P.from_rows(K.GLIDER)) and first[1].all()
    assert all(int(m.sum()) == 3 and not c.any() for c, m in images)
    # uncared cells do not tell images apart
    noisy = np.array([[1, 1], [1, 1]], dtype=np.uint8)
    assert len(P.orientations(noisy, np.array([[1, 1], [1, 1]]))) == 1
    assert len(P.orientations(np.array([[1, 0], [0, 0]]), np.array([[0, 1], [1, 0]]))) == 2


@pytest.mark.parametrize("rows", [K.BLOCK, K.BLINKER_H, K.GLIDER, K.BEEHIVE, ["O?O", "?.?"]])
def test_as_search_border_commutes_with_orientations(rows):
    cells, care = P.as_search(rows)
    turned_then_bordered = [P.as_search(c, m, border=1) for c, m in P.orientations(cells, care)]
    bordered_then_turned = P.orientations(*P.as_search(rows, border=1))
    assert len(turned_then_bordered) == len(bordered_then_turned)
    for (c1, m1), (c2, m2) in zip(turned_then_bordered, bordered_then_turned):
        assert np.array_equal(c1, c2) and np.array_equal(m1, m2)
