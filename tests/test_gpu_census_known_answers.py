"""GPU: the published Life facts of tests/known_patterns.py checked without a
host round-trip -- each pattern is dropped with place() on an empty torus and
its population read with population() (gol_census), so the same check runs at
any board size.  No snapshot is taken."""
import numpy as np
import pytest

import region_model as M
from known_patterns import CASES, GOSPER_GUN, board
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def as_pattern(cells):
    """(cell array, x offset, y offset) of a list of (x, y) offsets from the
    board centre."""
    xs, ys = [x for x, _ in cells], [y for _, y in cells]
    p = np.zeros((max(ys) - min(ys) + 1, max(xs) - min(xs) + 1), dtype=np.uint8)
    for x, y in cells:
        p[y - min(ys), x - min(xs)] = 1
    return p, min(xs), min(ys)


@pytest.mark.parametrize("name,cells,W,checks", CASES, ids=lambda v: v if isinstance(v, str) else "")
def test_published_populations_by_census(gpu, name, cells, W, checks):
    from gameoflife.engine import GolEngine
    p, dx, dy = as_pattern(cells)
    with GolEngine(W, W) as e:
        e.place(p, W // 2 + dx, W // 2 + dy)
        assert e.census() == {"population": len(cells),
                              "bbox": (W // 2 + dx, W // 2 + dy, W // 2 + dx + p.shape[1] - 1,
                                       W // 2 + dy + p.shape[0] - 1)}
        done = 0
        for gen, want in checks:
            e.step(gen - done)
            done = gen
            assert e.population() == want, (name, gen)
        assert e.epoch == done


def test_gun_box_grows_as_the_oracle_says(gpu):
    """The Gosper gun on 512^2 at one generation per pass: after a period the
    population is 36 + 5 and the box has grown by the glider's travel, exactly
    as the oracle's board has it."""
    from gameoflife.engine import GolEngine
    W = 512
    p, dx, dy = as_pattern(GOSPER_GUN)
    with GolEngine(W, W) as e:
        e.set_tuning(gens_per_pass=1)
        e.place(p, W // 2 + dx, W // 2 + dy)
        start = board(O.pack, W, GOSPER_GUN)
        assert e.census() == M.census(O.unpack(start, W))
        e.step(30)
        final, _ = O.run_packed(start, W, 30, want_hashes=False)
        want = M.census(O.unpack(final, W))
        assert want["population"] == 41
        assert e.census() == want
        assert want["bbox"] != M.census(O.unpack(start, W))["bbox"]
