"""GPU: soups generated on the device (gol_soup_batch, GolBatch.soup; DESIGN.md
section 5l).  snapshot() must equal, bit for bit, the cell-level model of
tests/soup_model.py on the shapes listed there -- one board per wave with wide,
narrow and odd windows, windows that touch bit 63 and the last row; three
boards per wave with idle lanes and a last wave of one board (the lane seam:
a T or Y source lane must stay inside the lane's own board); eight boards per
wave on the reference's clipped board -- and the call must behave as load()
does towards everything else a batch keeps.  The model's boards are computed
once per case and shared read-only."""
import numpy as np
import pytest

import soup_model as SM
from gameoflife import _native as N
from gameoflife import batch
from gameoflife.batch import GolBatch
from gameoflife.rules import rule_word

pytestmark = pytest.mark.gpu

INDEX0 = 7
SENTINEL = np.uint64(0x5A5A5A5A5A5A5A5A)
BIG = (64, 64, "torus", None, 5)
MID = (40, 20, "torus", None, 7)
SMALL = (8, 8, "ref-clipped", (7, 7), 130)
# one case per shape for the behaviour tests: the conventional soup, the lane seam, the reference's board
BEHAVIOUR = [(BIG, ((24, 24, 16, 16), 128, "D8")), (MID, ((31, 11, 9, 9), 128, "C4")),
             (SMALL, ((0, 0, 7, 7), 128, "C4"))]


def _batch(shape, **kw):
    W, H, topo, vis, n = shape
    return GolBatch(n, W, H, topology=topo, vis=vis, **kw)


def _model(shape, case, index0=INDEX0):
    W, H, _, _, n = shape
    return SM.boards(W, H, SM.SEED, index0, n, *case)


def _soup(b, case, **kw):
    win, density, sym = case
    b.soup(SM.SEED, window=win, density=density, symmetry=sym, index0=kw.pop("index0", INDEX0), **kw)


def _sentinel(shape):
    W, H, _, _, n = shape
    rows = np.full((n, H), SENTINEL & np.uint64((1 << W) - 1), dtype=np.uint64)
    rows[:, 0] ^= np.arange(n, dtype=np.uint64) & np.uint64((1 << W) - 1)  # every board another
    return rows


@pytest.fixture(scope="module")
def batches(gpu):
    """One batch per shape for the cases that only soup and read."""
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _batch(shape)
        return made[shape]

    yield get
    for b in made.values():
        b.close()


@pytest.mark.parametrize("sc", SM.CASES, ids=SM.case_id)
def test_snapshot_equals_the_model(batches, sc):
    shape, case = sc
    W, H, topo, vis, n = shape
    win, density, sym = case
    b = batches(shape)
    b.load(_sentinel(shape))
    b.step(1)
    _soup(b, case)
    got = b.snapshot()
    want = _model(shape, case)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert b.epoch == 0
    x, y, w, h = win or (0, 0, W, H)
    assert SM.invariant(SM.window_cells(got, (x, y, w, h)), sym)
    if density == 128 and SM.distinct_expected(sym, w, h, n):  # the boards of one wave differ from each other
        assert len({r.tobytes() for r in got}) == n
    # the reproducer: gol_soup_batch_rows in this process gives what the device holds
    again = batch.soup_rows(W, H, SM.SEED, [INDEX0 + 1, INDEX0 + n - 1], window=win, density=density, symmetry=sym,
                            topology=topo, vis=vis)
    assert np.array_equal(again, got[[1, n - 1]])


@pytest.mark.parametrize("shape,case", BEHAVIOUR, ids=["big", "mid", "small"])
@pytest.mark.parametrize("first,count", [(3, 2), (0, 1), (2, 3)])
def test_a_part_of_the_batch(gpu, shape, case, first, count):
    n = shape[4]
    if shape == SMALL:
        first, count = first * 3, count * 20  # ranges that start and end inside waves of eight boards
    want = _model(shape, case)
    with _batch(shape) as b:
        sentinel = _sentinel(shape)
        b.load(sentinel)
        b.step(2)
        held = b.snapshot()
        _soup(b, case, first=first, count=count)
        got = b.snapshot()
        assert b.epoch == 0
    part = np.zeros(n, dtype=bool)
    part[first:first + count] = True
    assert np.array_equal(got[part], want[part])  # the boards a whole-batch soup gives them
    assert np.array_equal(got[~part], held[~part])


@pytest.mark.parametrize("shape,case", BEHAVIOUR, ids=["big", "mid", "small"])
def test_behaves_as_load_does(gpu, shape, case):
    """soup leaves a batch exactly where load(the same boards) leaves it: the epoch, the per-board rules, and what
    step, step_cycles and objects then compute."""
    W, H, topo, vis, n = shape
    want = _model(shape, case)
    words = np.array([rule_word(("life", "B36/S23", "ref-effective")[i % 3]) for i in range(n)], dtype=np.uint32)
    with _batch(shape) as a, _batch(shape) as b:
        for x in (a, b):
            x.set_rules(words)
            x.load(_sentinel(shape))
            x.step_cycles(5)  # cycle and settle state of an earlier run
            x.step(3, settled=True)
            assert x.epoch == 8
        _soup(a, case)
        b.load(want)
        assert a.epoch == 0 and b.epoch == 0
        assert np.array_equal(a.rules(), words) and np.array_equal(b.rules(), words)
        pa, sa = a.step(64, populations=True, settled=True)
        pb, sb = b.step(64, populations=True, settled=True)
        assert np.array_equal(pa, pb) and np.array_equal(sa, sb)
        assert np.array_equal(a.hashes(), b.hashes()) and a.epoch == 64
        _soup(a, case)
        b.load(want)
        for got, ref in zip(a.step_cycles(200), b.step_cycles(200)):
            assert np.array_equal(got, ref)
        assert np.array_equal(a.snapshot(), b.snapshot()) and a.epoch == b.epoch == 200
        (ca, oa), (cb, ob) = a.objects(max_objects=32), b.objects(max_objects=32)
        assert np.array_equal(ca, cb) and np.array_equal(oa, ob)
        # objects straight after a soup, too
        _soup(a, case)
        b.load(want)
        (ca, oa), (cb, ob) = a.objects(max_objects=32), b.objects(max_objects=32)
        assert np.array_equal(ca, cb) and np.array_equal(oa, ob) and ca.sum() > 0


def test_step_after_soup_equals_step_after_load(gpu):
    """Under the batch's own rule: soup then step(64) gives the hashes load(model) then step(64) gives."""
    shape, case = BEHAVIOUR[0]
    with _batch(shape) as a, _batch(shape) as b:
        _soup(a, case)
        b.load(_model(shape, case))
        a.step(64)
        b.step(64)
        assert np.array_equal(a.hashes(), b.hashes())
        assert np.array_equal(a.snapshot(), b.snapshot())


def test_a_d8_soup_keeps_its_symmetries(gpu):
    """A centred square window on a 64 x 64 torus: B3/S23 commutes with the board's eight symmetries."""
    case = ((24, 24, 16, 16), 128, "D8")
    with _batch(BIG) as b:
        _soup(b, case)
        b.step(100)
        rows = b.snapshot()
    cells = SM.window_cells(rows, (0, 0, 64, 64))
    assert SM.invariant(cells, "D8") and cells.any()


def test_refusals_change_nothing(gpu):
    W, H, _, _, n = MID
    with _batch(MID) as b:
        b.load(_sentinel(MID))
        b.step(3)
        held = b.snapshot()
        refused = [
            dict(window=(0, 0, 0, 5)), dict(window=(0, 0, 5, 0)), dict(window=(-1, 0, 5, 5)), dict(window=(0, -1, 5, 5)),
            dict(window=(36, 0, 5, 5)), dict(window=(0, 16, 5, 5)), dict(density=0), dict(density=256),
            dict(density=1.0), dict(first=-1, count=1), dict(first=n, count=1), dict(first=1, count=n),
            dict(first=0, count=0),
        ] + [dict(window=(3, 0, 33, 20), symmetry=s) for s in SM.SQUARE]
        for kw in refused:
            with pytest.raises(N.GolError) as e:
                b.soup(SM.SEED, **kw)
            assert e.value.code == N.GOL_EINVAL and "gol_soup_batch" in str(e.value), kw
            assert b.epoch == 3, kw
        spec = N.GolSoupSpec()
        spec.w, spec.h, spec.density, spec.symmetry = 5, 5, 128, 9
        assert N.lib.gol_soup_batch(b._h, N.ctypes.byref(spec), 0, n) == N.GOL_EINVAL
        assert N.lib.gol_soup_batch(b._h, None, 0, n) == N.GOL_EINVAL
        with pytest.raises(ValueError):
            b.soup(SM.SEED, symmetry="D3")
        assert np.array_equal(b.snapshot(), held) and b.epoch == 3
        # ... and the edges are accepted
        b.soup(SM.SEED, window=(35, 15, 5, 5), density=255, symmetry="D8", first=n - 1, count=1)
        assert b.epoch == 0 and np.array_equal(b.snapshot()[:-1], held[:-1])
