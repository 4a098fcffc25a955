"""GPU: active-row stepping (gol_set_active_rows).  The
mode is a knob: per-generation hashes must equal the oracle's and final
snapshots those of an engine with the mode off, exactly, on the smallest
boards tall enough for the row-run branch to run (sparse_passes > 0 is asserted
wherever a case claims it): every device layout, every pass depth family,
patterns at the y seam and the clipped board's sink row, stale planes, the
spare plane used as scratch, mode switches, dense boards, groups."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (topology, W, H): one pair per row; odd word count (row-major); two 16-byte
# chunks per row; the reference's clipped geometry, last word partial
BOARDS = [("torus", 64, 512), ("torus", 96, 512), ("torus", 256, 1024), ("ref-clipped", 70, 600)]
BOARD_IDS = [f"{t}-{w}x{h}" for t, w, h in BOARDS]
DEPTHS = [1, 2, 7, 10, 12, 0]  # gol_set_tuning gens_per_pass; 0: the planner's

GLIDER_DOWN = [[0, 1, 0], [0, 0, 1], [1, 1, 1]]  # heads down and right
GLIDER_UP = GLIDER_DOWN[::-1]                    # heads up and right
BLINKER = [[1, 1, 1]]
R_PENTOMINO = [[0, 1, 1], [1, 1, 0], [0, 1, 0]]

# engine rule name -> the oracle's (birth, survive)
RULES = {"life": O.LIFE, "B36/S23": (0x048, 0x00C), "ref-literal": O.REF_LITERAL, "B0/S23": (0x001, 0x00C)}


def topo(topology):
    return O.TORUS if topology == "torus" else O.REF_CLIPPED


def cells_of(W, H, items):
    c = np.zeros((H, W), dtype=np.uint8)
    for p, x, y in items:
        p = np.asarray(p, dtype=np.uint8)
        for dy, dx in zip(*np.nonzero(p)):
            c[(y + dy) % H, (x + dx) % W] = 1
    return c


def engine(topology, W, H, rule="life", depth=0, active=True):
    from gameoflife.engine import GolEngine
    e = GolEngine(W, H, topology=topology, rule=rule, active_rows=active)
    e.set_tuning(gens_per_pass=depth)
    return e


def seam_items(topology, W, H):
    """A glider two rows below row 0 heading up (across the y seam of a torus,
    into the edge of a clipped board), a blinker on the last row, and on the
    clipped board a glider running into the sink row."""
    items = [(GLIDER_UP, 10, 2), (BLINKER, 30, H - 1)]
    if topology != "torus":
        items.append((GLIDER_DOWN, 5, H - 14))
    return items


def run_both(topology, W, H, rule, depth, items, gens, hashed, expect_sparse=True):
    """The items placed on an empty board, stepped with the mode on and off;
    returns the mode-on engine's stats."""
    want_final, want = O.run_packed(O.pack(cells_of(W, H, items)), W, gens, topo(topology), RULES[rule])
    finals = []
    for active in (True, False):
        with engine(topology, W, H, rule, depth, active) as e:
            for p, x, y in items:
                e.place(p, x, y)
            got = e.step(gens, hashes=hashed)
            if hashed:
                np.testing.assert_array_equal(got, want)
            assert e.epoch == gens
            assert e.hash() == int(want[-1])
            finals.append(e.snapshot())
            if active:
                st = e.active_stats()
                cover(e)
    np.testing.assert_array_equal(finals[0], want_final)
    np.testing.assert_array_equal(finals[0], finals[1])
    if expect_sparse:
        assert st["sparse_passes"] > 0, st
        assert st["rows_stepped"] < st["passes"] * H, st
    return st


def cover(e):
    """active_rows() holds every live row the census sees."""
    runs, box = e.active_rows(), e.census()["bbox"]
    if runs is None or box is None:
        return
    for y in (box[1], box[3]):
        assert any(lo <= y < hi for lo, hi in runs), (runs, box)


@pytest.mark.parametrize("hashed", [True, False], ids=["hashed", "unhashed"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("topology,W,H", BOARDS, ids=BOARD_IDS)
def test_seam_patterns_at_every_depth(gpu, topology, W, H, depth, hashed):
    run_both(topology, W, H, "life", depth, seam_items(topology, W, H), 48, hashed)


@pytest.mark.parametrize("topology,W,H", BOARDS, ids=BOARD_IDS)
def test_two_r_pentominoes_grow_and_merge(gpu, topology, W, H):
    # two patterns need 2 x 3 blocks of rows: only the tallest board can step them as runs
    items = [(R_PENTOMINO, W // 2, 60), (R_PENTOMINO, W // 3, 360)]
    run_both(topology, W, H, "life", 0, items, 200, True, expect_sparse=H >= 1024)


@pytest.mark.parametrize("depth", [1, 7, 0])
@pytest.mark.parametrize("rule", ["B36/S23", "ref-literal"])
@pytest.mark.parametrize("topology,W,H", BOARDS[1:], ids=BOARD_IDS[1:])
def test_other_rules(gpu, topology, W, H, rule, depth):
    items = seam_items(topology, W, H) + ([(R_PENTOMINO, W // 2, H // 2 + 30)] if H >= 1024 else [])
    run_both(topology, W, H, rule, depth, items, 36, True)


@pytest.mark.parametrize("topology,W,H", [BOARDS[1], BOARDS[3]], ids=[BOARD_IDS[1], BOARD_IDS[3]])
def test_birth_on_zero_neighbours_steps_dense(gpu, topology, W, H):
    st = run_both(topology, W, H, "B0/S23", 0, seam_items(topology, W, H), 12, True, expect_sparse=False)
    assert st["sparse_passes"] == 0 and st["scans"] == 0 and st["passes"] > 0, st


@pytest.mark.parametrize("topology,W,H", [BOARDS[0], BOARDS[3]], ids=[BOARD_IDS[0], BOARD_IDS[3]])
def test_stale_planes(gpu, topology, W, H):
    """A pattern killed between passes leaves its last generation but one in
    the spare plane; nothing of it may come back."""
    depth = 6
    with engine(topology, W, H, depth=depth) as e:
        e.place(R_PENTOMINO, 20, 200)
        e.step(3 * depth)
        x0, y0, x1, y1 = e.census()["bbox"]
        e.write_region(x0, y0, np.ones((y1 - y0 + 1, x1 - x0 + 1), dtype=np.uint8), mode="clear")
        got = e.step(2 * depth, hashes=True)
        assert not got.any() and e.hash() == 0 and e.population() == 0
        # until a scan finds the board empty and the passes launch nothing
        e.step(6 * depth)
        assert e.active_rows() == [] and e.population() == 0
        epoch = e.epoch
        # a blinker inside the rows where the old pattern last lived
        items = [(BLINKER, x0, (y0 + y1) // 2)]
        e.place(*items[0])
        got = e.step(4 * depth, hashes=True)
        want_final, want = O.run_packed(O.pack(cells_of(W, H, items)), W, 4 * depth, topo(topology), O.LIFE)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(e.snapshot(), want_final)
        assert e.epoch == epoch + 4 * depth
        assert e.active_stats()["sparse_passes"] > 0


def test_spare_plane_scratch(gpu):
    """snapshot(), checkpoint() and restore() between passes of a pair-layout
    torus go through the spare plane; stepping goes on as if they had not."""
    topology, W, H = BOARDS[0]
    items = seam_items(topology, W, H)
    start = O.pack(cells_of(W, H, items))
    final48, want = O.run_packed(start, W, 48, O.TORUS, O.LIFE)
    at12, _ = O.run_packed(start, W, 12, O.TORUS, O.LIFE)
    with engine(topology, W, H, depth=6) as e:
        for p, x, y in items:
            e.place(p, x, y)
        h1 = e.step(12, hashes=True)
        np.testing.assert_array_equal(e.snapshot(), at12)
        h2 = e.step(12, hashes=True)
        blob = e.checkpoint()
        h3 = e.step(12, hashes=True)
        np.testing.assert_array_equal(np.concatenate([h1, h2, h3]), want[:36])
        e.restore(blob)
        assert e.epoch == 24 and e.active_rows() is None
        h4 = e.step(24, hashes=True)
        np.testing.assert_array_equal(h4, want[24:])
        np.testing.assert_array_equal(e.snapshot(), final48)
        st = e.active_stats()
        assert st["sparse_passes"] > 0 and st["scans"] > 0, st
        cover(e)


@pytest.mark.parametrize("topology,W,H", [BOARDS[2], BOARDS[3]], ids=[BOARD_IDS[2], BOARD_IDS[3]])
def test_load_then_step(gpu, topology, W, H):
    items = seam_items(topology, W, H) + ([(R_PENTOMINO, 40, H // 2 + 30)] if H >= 1024 else [])
    start = O.pack(cells_of(W, H, items))
    final, want = O.run_packed(start, W, 30, topo(topology), O.LIFE)
    with engine(topology, W, H) as e:
        e.load(start)
        assert e.active_rows() is None
        np.testing.assert_array_equal(e.step(30, hashes=True), want)
        np.testing.assert_array_equal(e.snapshot(), final)
        st = e.active_stats()
        assert st["scans"] > 0 and st["sparse_passes"] > 0, st
        cover(e)


def test_mode_switches_between_passes(gpu):
    topology, W, H = BOARDS[2]
    items = seam_items(topology, W, H) + [(R_PENTOMINO, 100, 540)]
    final, want = O.run_packed(O.pack(cells_of(W, H, items)), W, 60, O.TORUS, O.LIFE)
    with engine(topology, W, H, depth=10) as e:
        for p, x, y in items:
            e.place(p, x, y)
        got = []
        for on in (True, False, True, False, False, True):
            e.set_active_rows(on)
            got.append(e.step(10, hashes=True))
        np.testing.assert_array_equal(np.concatenate(got), want)
        np.testing.assert_array_equal(e.snapshot(), final)
        st = e.active_stats()
        assert st["passes"] == 3 and st["sparse_passes"] == 3, st
        cover(e)


def test_enabling_on_a_seeded_board(gpu):
    """Unknown rows -> a scan -> dense: every pass steps the whole plane, and
    scans back off."""
    topology, W, H = BOARDS[2]
    final, want = O.run_packed(O.seed_packed(W, H, 5), W, 120, O.TORUS, O.LIFE)
    with engine(topology, W, H, depth=6, active=False) as e:
        e.seed(5)
        h1 = e.step(12, hashes=True)
        e.set_active_rows(True)
        h2 = e.step(108, hashes=True)
        np.testing.assert_array_equal(np.concatenate([h1, h2]), want)
        np.testing.assert_array_equal(e.snapshot(), final)
        st = e.active_stats()
        assert st["passes"] == 18 and st["sparse_passes"] == 0 and st["rows_stepped"] == 18 * H, st
        assert 1 <= st["scans"] <= 5, st  # the first pass, then after ever longer waits


def test_seeded_soup(gpu):
    topology, W, H = BOARDS[2]
    final, want = O.run_packed(O.seed_packed(W, H, 0x5EED), W, 60, O.TORUS, O.LIFE)
    with engine(topology, W, H) as e:
        e.seed(0x5EED)
        np.testing.assert_array_equal(e.step(60, hashes=True), want)
        np.testing.assert_array_equal(e.snapshot(), final)


def test_work_bound_of_a_lone_glider(gpu):
    """By the policy of DESIGN.md section 5c a launch never exceeds
    2 x (2 blocks) + 4 blocks + 2 G rows, block-rounded: under 600 of 4096."""
    W, H, gens = 256, 4096, 240
    items = [(GLIDER_DOWN, 100, 2000)]
    final, want = O.run_packed(O.pack(cells_of(W, H, items)), W, gens, O.TORUS, O.LIFE)
    with engine("torus", W, H) as e:
        e.place(*items[0])
        np.testing.assert_array_equal(e.step(gens, hashes=True), want)
        np.testing.assert_array_equal(e.snapshot(), final)
        st = e.active_stats()
        assert st["passes"] == len(e.pass_plan(gens, hashes=True)) and st["sparse_passes"] == st["passes"], st
        assert st["rows_stepped"] <= st["passes"] * H // 4, st
        runs, box = e.active_rows(), e.census()["bbox"]
        assert box is not None and any(lo <= box[1] and box[3] < hi for lo, hi in runs), (runs, box)


def test_empty_board(gpu):
    with engine("torus", 64, 512) as e:
        got = e.step(24, hashes=True)
        assert got.shape == (24,) and not got.any()
        assert e.epoch == 24 and e.active_rows() == []
        st = e.active_stats(reset=True)
        assert st["sparse_passes"] == st["passes"] > 0 and st["rows_stepped"] == 0, st
        assert e.active_stats()["passes"] == 0


def test_refusals(gpu):
    from gameoflife import _native as N
    with engine("torus", 64, 512) as e:
        assert N.lib.gol_set_active_rows(e._h, 2) == N.GOL_EINVAL
        assert N.lib.gol_set_active_rows(e._h, -1) == N.GOL_EINVAL
        assert N.lib.gol_active_stats_read(e._h, None, 0) == N.GOL_EINVAL
        assert N.lib.gol_active_rows(e._h, None, 0, None) == N.GOL_EINVAL


def test_grouped_context_steps_dense(gpu):
    """The mode does not reach the sharded path: a two-shard group with it on
    computes what the oracle computes, every pass over whole shards."""
    from gameoflife.engine import GolEngine, ShardGroup
    from gameoflife.shard import shard_rows_py
    W, H, gens = 64, 512, 48
    items = seam_items("torus", W, H) + [(R_PENTOMINO, 20, 250)]
    final, want = O.run_packed(O.pack(cells_of(W, H, items)), W, gens, O.TORUS, O.LIFE)
    shards = []
    for k in range(2):
        r0, rows = shard_rows_py(H, k, 2)
        shards.append(GolEngine(W, H, row0=r0, rows=rows, active_rows=True))
    with ShardGroup(shards) as g:
        for p, x, y in items:
            g.place(p, x, y)
        np.testing.assert_array_equal(g.step(gens, hashes=True), want)
        np.testing.assert_array_equal(g.snapshot(), final)
        for s in shards:
            st = s.active_stats()
            assert st["sparse_passes"] == 0 and st["scans"] == 0, st
            assert s.active_rows() is None
    for s in shards:
        s.close()
