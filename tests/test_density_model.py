"""CPU: the numpy density model (tests/density_model.py) against a brute-force
double loop, the pictures of gameoflife.view, and what GolEngine.density and
gol_density refuse before any device is touched."""
import ctypes

import numpy as np
import pytest

import density_model as D

W, H = 11, 9
TILES = (1, 2, 4, 16)


def board():
    return (np.random.default_rng(5).random((H, W)) < 0.5).astype(np.uint8)


def brute(cells, x0, y0, w, h, tile, row0=0, rows=None):
    rows = cells.shape[0] - row0 if rows is None else rows
    out = np.zeros((-(-h // tile), -(-w // tile)), dtype=np.uint32)
    for i in range(h):
        for k in range(w):
            y, x = (y0 + i) % cells.shape[0], (x0 + k) % cells.shape[1]
            if row0 <= y < row0 + rows:
                out[i // tile, k // tile] += cells[y, x]
    return out


# wrapped windows: over both seams, as wide and as tall as the board, one cell
WRAPPED = [(0, 0, W, H), (9, 7, 5, 5), (3, 2, W, H), (10, 8, 1, 1), (4, 0, 7, 3)]
CLIPPED = [(0, 0, W, H), (2, 1, 4, 3), (W - 3, H - 2, 3, 2), (0, 0, 1, 1)]


@pytest.mark.parametrize("tile", TILES)
def test_model_matches_the_double_loop(tile):
    cells = board()
    for torus, wins in ((True, WRAPPED), (False, CLIPPED)):
        for x0, y0, w, h in wins:
            got = D.density(cells, x0, y0, w, h, tile, torus)
            assert got.dtype == np.uint32 and got.shape == (-(-h // tile), -(-w // tile))
            np.testing.assert_array_equal(got, brute(cells, x0, y0, w, h, tile), err_msg=str((torus, x0, y0, w, h)))
            assert int(got.sum()) == int(cells[np.ix_((y0 + np.arange(h)) % H, (x0 + np.arange(w)) % W)].sum())


@pytest.mark.parametrize("tile", TILES)
def test_shard_slices_sum_to_the_whole(tile):
    cells = board()
    for x0, y0, w, h in WRAPPED:
        whole = D.density(cells, x0, y0, w, h, tile)
        parts = []
        for row0, rows in ((0, 2), (2, 4), (6, 3)):  # boundaries that cut through tile rows
            part = D.density(cells, x0, y0, w, h, tile, row0=row0, rows=rows)
            np.testing.assert_array_equal(part, brute(cells, x0, y0, w, h, tile, row0, rows))
            parts.append(part)
        np.testing.assert_array_equal(sum(parts), whole)


def test_ascii_picture():
    from gameoflife import view
    counts = np.array([[0, 1, 8, 16], [16, 0, 3, 9]], dtype=np.uint32)
    rows = view.density_ascii(counts, 4)
    assert [len(r) for r in rows] == [4, 4]
    ramp = view.RAMP
    for r, line in zip(counts, rows):
        for c, ch in zip(r, line):
            assert (ch == ramp[0]) == (c == 0)           # a count of 0, and only that, gives the first character
            assert ch == ramp[-1] if c == 16 else ch != ramp[-1]
    assert rows[0][1] == ramp[1]                          # 1 / 16 rounds to level 0: lifted to the second
    assert ramp.index(rows[0][2]) < ramp.index(rows[1][3]) <= len(ramp) - 2
    assert view.density_ascii(counts, 4, ramp=".#") == [".###", "#.##"]
    # one live cell in the coarsest tile is still seen
    assert view.density_ascii(np.array([[1, 0]], dtype=np.uint32), 32768) == [ramp[1] + ramp[0]]
    with pytest.raises(ValueError):
        view.density_ascii(counts, 4, ramp="x")


def test_pgm_picture():
    from gameoflife import view
    counts = np.array([[0, 1, 8], [16, 0, 3]], dtype=np.uint32)
    pgm = view.density_pgm(counts, 4)
    header = b"P5\n3 2\n255\n"
    assert pgm.startswith(header) and len(pgm) == len(header) + 6
    px = np.frombuffer(pgm[len(header):], dtype=np.uint8).reshape(2, 3)
    np.testing.assert_array_equal(px == 0, counts == 0)
    assert px[1, 0] == 255 and px[0, 1] >= 1 and px[0, 2] == 8 * 255 // 16
    one = view.density_pgm(np.array([[1]], dtype=np.uint32), 32768)
    assert one[-1] == 1


@pytest.mark.parametrize("tile", [0, 3, 65536, -4, 2.0, True])
def test_engine_rejects_tiles_before_touching_the_library(tile):
    from gameoflife.engine import GolEngine, ShardGroup
    e = GolEngine.__new__(GolEngine)  # no context: anything past the tile check would fail otherwise
    with pytest.raises(ValueError):
        e.density(tile)
    g = ShardGroup.__new__(ShardGroup)
    with pytest.raises(ValueError):
        g.density(tile)


def test_null_context_is_refused():
    from gameoflife import _native as N
    buf = np.full((2, 2), 7, dtype=np.uint32)
    assert N.lib.gol_density(None, 0, 0, 1, 1, 0, buf.ctypes.data_as(N._u32p), 2) == N.GOL_EINVAL
    assert N.lib.gol_last_error(None)
    assert N.lib.gol_density(None, 0, 0, 1, 1, 0, ctypes.cast(None, N._u32p), 2) == N.GOL_EINVAL
    assert (buf == 7).all()
