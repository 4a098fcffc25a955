"""GPU: gol_census (population and bounding box counted on the device)
against numpy on snapshot(), on the smallest boards of each layout and on one
large enough for several workgroups and grid-stride iterations."""
import numpy as np
import pytest

import region_model as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

I64_MAX = 2**63 - 1
SENTINEL = (0, I64_MAX, -1, I64_MAX, -1)
BOARDS = [("torus", 64, 8), ("torus", 96, 8), ("torus", 256, 16), ("ref-clipped", 7, 7), ("ref-clipped", 70, 9),
          ("torus", 4096, 512)]
BOARD_IDS = [f"{t}-{w}x{h}" for t, w, h in BOARDS]


def check(e, W):
    """The engine's census equals numpy's on its own snapshot."""
    from gameoflife import codec
    want = M.census(codec.unpack(e.snapshot(), W), e.row0)
    got = e.census()
    assert got == want
    assert e.population() == want["population"]
    return got


@pytest.mark.parametrize("topology,W,H", BOARDS, ids=BOARD_IDS)
def test_census_matches_numpy(gpu, topology, W, H):
    from gameoflife.engine import GolEngine
    with GolEngine(W, H, topology=topology) as e:
        # empty: the sentinels that let shards combine by sum / min / max
        assert e._census_raw() == SENTINEL
        assert e.census() == {"population": 0, "bbox": None}
        # full: every stored cell, on a clipped board those outside the visible extent too
        e.load(O.pack(np.ones((H, W), dtype=np.uint8)))
        assert e.census() == {"population": W * H, "bbox": (0, 0, W - 1, H - 1)}
        # one live cell: the corners, and a cell in the second word / odd column of a pair
        singles = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)] + ([(33, 3)] if W > 33 else [(4, 3)])
        for x, y in singles:
            cells = np.zeros((H, W), dtype=np.uint8)
            cells[y, x] = 1
            e.load(O.pack(cells))
            assert e.census() == {"population": 1, "bbox": (x, y, x, y)}, (x, y)
        # two cells whose box no single word holds
        cells = np.zeros((H, W), dtype=np.uint8)
        cells[H - 2, 1] = cells[1, W - 2] = 1
        e.load(O.pack(cells))
        assert e.census() == {"population": 2, "bbox": (1, 1, W - 2, H - 2)}
        # seeded boards, fresh and after a few generations; the census leaves the board alone
        for seed in (1, 2):
            e.seed(seed)
            before = e.hash()
            got = check(e, W)
            assert got["population"] == M.census(O.unpack(O.seed_packed(W, H, seed), W))["population"]
            assert e.hash() == before and e.epoch == 0
            e.step(3)
            check(e, W)
            assert e.epoch == 3


def test_sparse_boxes_on_the_large_board(gpu):
    """Random sparse boards on 4096 x 512: the box edges fall in arbitrary
    words and rows, far from where most lanes look."""
    from gameoflife.engine import GolEngine
    W, H = 4096, 512
    rng = np.random.default_rng(4)
    with GolEngine(W, H) as e:
        for n in (2, 5, 40):
            cells = np.zeros((H, W), dtype=np.uint8)
            cells[rng.integers(0, H, n), rng.integers(0, W, n)] = 1
            e.load(O.pack(cells))
            assert e.census() == M.census(cells)


def test_shards_combine_by_sum_min_max(gpu):
    from gameoflife.engine import GolEngine, ShardGroup
    W, H = 256, 16
    shards, r0 = [], 0
    for rows in (5, 5, 6):
        s = GolEngine(W, H, row0=r0, rows=rows)
        s.seed(8)
        shards.append(s)
        r0 += rows
    group = ShardGroup(shards)
    with GolEngine(W, H) as single:
        single.seed(8)
        group.step(4)
        single.step(4)
        assert group.census() == single.census() == check(single, W)
        assert group.population() == single.population()
        for s in shards:  # each shard's box is in global coordinates
            check(s, W)
    # live cells in the first shard's rows only: the others report the sentinels
    cells = np.zeros((H, W), dtype=np.uint8)
    cells[1, 200] = cells[4, 7] = 1
    packed = O.pack(cells)
    r0 = 0
    for s in shards:
        s.load(packed[r0:r0 + s.rows])
        r0 += s.rows
    assert shards[0].census() == {"population": 2, "bbox": (7, 1, 200, 4)}
    assert shards[1]._census_raw() == SENTINEL and shards[2]._census_raw() == SENTINEL
    assert group.census() == {"population": 2, "bbox": (7, 1, 200, 4)}
    group.close()
    for s in shards:
        s.close()
