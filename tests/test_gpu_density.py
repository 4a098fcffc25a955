"""GPU: gol_density against the numpy density model (tests/density_model.py),
which reads the engine's own snapshot.  Counts are integers: every comparison
is exact.  The fine kernel (T <= 32) and the coarse one (T >= 64) both run on
the smallest boards of each device layout and on boards whose rows hold
several 16-byte chunks, with windows that are unaligned, cross tile edges by
one cell, wrap both seams or sit flush with a clipped board's far corner."""
import ctypes

import numpy as np
import pytest

import density_model as D
from known_patterns import GOSPER_GUN_ROWS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPOCH = 2  # boards are seeded and stepped: a density of the seeded plane alone would not show a stale plane


def ids(boards):
    return [f"{t}-{w}x{h}" for t, w, h in boards]


def stepped(topology, W, H, seed=11, **kw):
    """(engine, its board as cells) after EPOCH generations."""
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    e = GolEngine(W, H, topology=topology, **kw)
    e.seed(seed)
    e.step(EPOCH)
    return e, codec.unpack(e.snapshot(), W)


def check_windows(e, cells, topology, wins, log2_tiles):
    torus = topology == "torus"
    for lg in log2_tiles:
        for x0, y0, w, h in wins:
            want = D.density(cells, x0, y0, w, h, 1 << lg, torus)
            got = e.density(1 << lg, x0, y0, w, h)
            assert got.dtype == np.uint32 and got.shape == want.shape
            np.testing.assert_array_equal(got, want, err_msg=str((lg, x0, y0, w, h)))


# ---- fine regime: the smallest boards of each layout (as tests/test_gpu_region.py) ----
FINE_BOARDS = [("torus", 64, 8), ("torus", 96, 8), ("torus", 256, 16), ("ref-clipped", 7, 7), ("ref-clipped", 70, 9)]


def fine_windows(topology, W, H):
    torus = topology == "torus"
    cand = [(0, 0, 1, 1), (5, 1, 31, 3), (5, 1, 33, 3), (31, 0, 2, 1), (3, 3, 67, 4), (0, 0, W, H)]
    if torus:
        cand += [(W - 2, H - 2, 5, 5), (5, 0, W, 2), (W - 1, 0, 1, H)]
    else:
        cand += [(2, 1, 4, 3), (W - 3, H - 2, 3, 2)]
    fits = [c for c in cand if c[2] <= W and c[3] <= H and c[0] < W and c[1] < H
            and (torus or (c[0] + c[2] <= W and c[1] + c[3] <= H))]
    assert len(fits) >= 4, fits
    return fits


@pytest.mark.parametrize("topology,W,H", FINE_BOARDS, ids=ids(FINE_BOARDS))
def test_small_boards_match_the_model(gpu, topology, W, H):
    e, cells = stepped(topology, W, H)
    with e:
        check_windows(e, cells, topology, fine_windows(topology, W, H), range(0, 7))
        assert e.epoch == EPOCH


# ---- coarse regime: pairs with four 16-byte chunks per row; 17 row-major words, the last chunk partial;
# a clipped board with a partial last word ----
COARSE_BOARDS = [("torus", 512, 264), ("torus", 544, 264), ("ref-clipped", 530, 270)]


def coarse_windows(topology, W, H):
    wins = [(0, 0, W, H), (33, 0, 257, 129), (63, 7, 130, 1)]
    if topology == "torus":
        return wins + [(129, 5, W, H), (W - 70, H - 100, 300, 200)]
    return wins + [(W - 257, H - 129, 257, 129)]


@pytest.mark.parametrize("topology,W,H", COARSE_BOARDS, ids=ids(COARSE_BOARDS))
def test_chunked_boards_match_the_model(gpu, topology, W, H):
    e, cells = stepped(topology, W, H)
    with e:
        check_windows(e, cells, topology, coarse_windows(topology, W, H), range(5, 9))
        assert e.epoch == EPOCH


def test_tile_limits_on_a_one_wave_row(gpu):
    """4096 x 4096: a row is one wave of 16-byte lanes.  Tiles of one group, of
    two chunks and of half the board; the largest tile; and the census."""
    W = 4096
    e, cells = stepped("torus", W, W)
    with e:
        check_windows(e, cells, "torus", [(0, 0, W, W)], (6, 8, 11))
        pop = e.population()
        assert pop == int(cells.sum())
        top = e.density(32768)
        assert top.shape == (1, 1) and int(top[0, 0]) == pop
        assert int(e.density(256).sum(dtype=np.uint64)) == pop


# ---- shards ----
def make_group(topology, W, H, blocks, seed=5):
    from gameoflife.engine import GolEngine, ShardGroup
    shards, r0 = [], 0
    for rows in blocks:
        s = GolEngine(W, H, topology=topology, row0=r0, rows=rows)
        s.seed(seed)
        shards.append(s)
        r0 += rows
    assert r0 == H
    return shards, ShardGroup(shards)


@pytest.mark.parametrize("topology,W,H", [("torus", 512, 264), ("ref-clipped", 530, 270)], ids=["torus", "clipped"])
def test_shards_add_into_one_map(gpu, topology, W, H):
    """Three shards whose boundaries (rows 88 and 176) are multiples of 8 but
    cut through tile rows at T = 32 and T = 128: the group's map is the
    model's, each shard's own map the model of its rows."""
    from gameoflife import codec
    torus = topology == "torus"
    shards, group = make_group(topology, W, H, (88, 88, H - 176))
    try:
        group.step(EPOCH)
        cells = codec.unpack(group.snapshot(), W)
        for tile in (8, 32, 128):
            for x0, y0, w, h in [(0, 0, W, H)] + ([(129, 200, W, H)] if torus else []):
                np.testing.assert_array_equal(group.density(tile, x0, y0, w, h),
                                              D.density(cells, x0, y0, w, h, tile, torus), err_msg=str((tile, x0, y0)))
                for s in shards:
                    np.testing.assert_array_equal(s.density(tile, x0, y0, w, h),
                                                  D.density(cells, x0, y0, w, h, tile, torus, s.row0, s.rows),
                                                  err_msg=str((tile, x0, y0, s.row0)))
        assert group.epoch == EPOCH
    finally:
        group.close()
        for s in shards:
            s.close()


# ---- the raw call ----
def raw(e, x0, y0, w, h, lg, buf, pitch=None, null=False):
    from gameoflife import _native as N
    p = ctypes.cast(None, N._u32p) if null else buf.ctypes.data_as(N._u32p)
    return N.lib.gol_density(e._h if e is not None else None, x0, y0, w, h, lg, p, buf.shape[1] if pitch is None else pitch)


@pytest.mark.parametrize("lg", [1, 6], ids=["fine", "coarse"])
def test_raw_call_adds_and_keeps_the_rest(gpu, lg):
    """A prefilled buffer with a wide pitch: the call adds, and touches only
    the first tw entries of the map rows the shard has board rows in."""
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    W, H, T = 256, 192, 1 << lg
    board = O.run_packed(O.seed_packed(W, H, 5), W, EPOCH, want_hashes=False)[0]
    cells = codec.unpack(board, W)
    x0, y0, w, h = 3, 0, 200, H
    tw, th = -(-w // T), -(-h // T)
    row0, rows = 70, 61  # board rows 70 .. 130: in the middle of a tile row at either tile
    with GolEngine(W, H, row0=row0, rows=rows) as e:
        e.load(board[row0:row0 + rows])
        buf = np.full((th, tw + 2), 7, dtype=np.uint32)
        assert raw(e, x0, y0, w, h, lg, buf) == 0
        want = D.density(cells, x0, y0, w, h, T, True, row0, rows)
        touched = np.zeros(th, dtype=bool)
        touched[row0 // T:(row0 + rows - 1) // T + 1] = True
        assert 0 < touched.sum() < th
        np.testing.assert_array_equal(buf[touched, :tw], want[touched] + 7)
        assert (want[~touched] == 0).all() and (buf[~touched] == 7).all() and (buf[:, tw:] == 7).all()
        # windows that miss the shard: above it, below it, and over the y seam
        for wy, wh in ((0, 70), (131, 61), (131, 131)):
            miss = np.full((-(-wh // T), tw), 7, dtype=np.uint32)
            assert raw(e, x0, wy, w, wh, lg, miss) == 0
            assert (miss == 7).all()
        assert e.epoch == 0


def test_refusals(gpu):
    from gameoflife import _native as N
    from gameoflife.engine import GolEngine
    buf = np.full((16, 8), 7, dtype=np.uint32)

    def refused(e, rc):
        assert rc == N.GOL_EINVAL
        assert N.lib.gol_last_error(e._h if e is not None else None)
        assert N.take_hip_error() == 0
        assert (buf == 7).all()

    W, H = 256, 16
    with GolEngine(W, H) as e:
        e.seed(3)
        e.step(3)
        before = e.hash()
        for lg in (-1, 16):
            refused(e, raw(e, 0, 0, 8, 8, lg, buf))
        refused(e, raw(e, 0, 0, 8, 8, 0, buf, null=True))
        refused(e, raw(e, 0, 0, 64, 8, 2, buf, pitch=15))  # tw = 16
        assert raw(e, 0, 0, 32, 8, 2, buf.copy(), pitch=8) == N.GOL_OK  # tw = 8 = pitch
        for x0, y0, w, h in [(0, 0, 0, 1), (0, 0, 1, 0), (W, 0, 1, 1), (0, H, 1, 1), (-1, 0, 1, 1), (0, 0, W + 1, 1),
                             (0, 0, 1, H + 1)]:
            refused(e, raw(e, x0, y0, w, h, 3, buf))
        refused(None, raw(None, 0, 0, 1, 1, 0, buf))
        assert e.hash() == before and e.epoch == 3
    with GolEngine(70, 9, topology="ref-clipped") as e:
        e.seed(3)
        for x0, y0, w, h in [(60, 0, 11, 1), (0, 8, 1, 2), (69, 8, 2, 2)]:  # a clipped board does not wrap
            refused(e, raw(e, x0, y0, w, h, 1, buf))
        assert raw(e, 60, 8, 10, 1, 1, buf.copy()) == N.GOL_OK  # flush with the corner


# ---- ordering and purity ----
def test_ordered_after_asynchronous_steps_and_pure(gpu):
    """density right behind an unhashed (asynchronous) step sees the stepped
    board; it changes neither the epoch nor the hash nor what later steps
    compute; a snapshot in flight keeps its board."""
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    W, H, seed = 256, 64, 21
    start = O.seed_packed(W, H, seed)
    at3, _ = O.run_packed(start, W, 3)
    at7, want_hashes = O.run_packed(at3, W, 4)
    with GolEngine(W, H) as e:
        e.seed(seed)
        e.step(3)  # not waited for
        for tile in (4, 64):
            np.testing.assert_array_equal(e.density(tile, 250, 60, 70, 9),
                                          D.density(codec.unpack(at3, W), 250, 60, 70, 9, tile))
        assert e.epoch == 3 and e.hash() == O.hash_packed(at3, W)
        np.testing.assert_array_equal(e.step(4, hashes=True), want_hashes)
        buf = e.host_buffer()
        e.snapshot_async(buf)
        for tile in (4, 64):
            np.testing.assert_array_equal(e.density(tile), D.density(codec.unpack(at7, W), 0, 0, W, H, tile))
        assert e.snapshot_wait() == 7
        np.testing.assert_array_equal(buf, at7)
        assert e.epoch == 7 and e.hash() == O.hash_packed(at7, W)


# ---- known answer ----
def test_gun_shows_where_the_census_says(gpu):
    """A Gosper gun at (5000, 5000) on 16384^2 after 120 generations: the map
    sums to the census population (36 cells and four gliders) and is zero
    outside the tiles the census's bounding box meets."""
    from gameoflife.engine import GolEngine
    W, T = 16384, 1024
    with GolEngine(W, W) as e:
        e.place(GOSPER_GUN_ROWS, 5000, 5000)
        e.step(120)
        c = e.census()
        assert c["population"] == 36 + 5 * 4
        m = e.density(T)
        assert m.shape == (W // T, W // T) and int(m.sum()) == c["population"]
        x_lo, y_lo, x_hi, y_hi = c["bbox"]
        inside = np.zeros_like(m, dtype=bool)
        inside[y_lo // T:y_hi // T + 1, x_lo // T:x_hi // T + 1] = True
        assert (m[~inside] == 0).all() and m[inside].any()
