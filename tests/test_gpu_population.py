"""GPU: the fused per-generation population series (gol_step_series,
gol_group_step_series) against the CPU oracle.

Reference of every case: the board stepped generation by generation with
oracle.step_packed and its bits counted with numpy; the hashes, where asked,
are oracle.run_packed's.  Checked per generation: the populations (and the
hashes); at the end the snapshot word for word and population() (gol_census)
against the last entry.  The shapes are the smallest at which each code path
of the series instances can go wrong -- those tests/test_gpu_unhashed_passes.py
uses for the same kernels: every depth on rows under one wave, of an exact
strip and either side of it, of two strips with a short last one, of many
strips and of an odd word count (row-major one-word lanes); whole-row waves;
16-byte lanes; band heights; generic rules; clipped boards; a chunk boundary
of the step; every sharded schedule; active rows."""
import functools
import threading
import uuid

import numpy as np
import pytest

from known_patterns import GOSPER_GUN, R_PENTOMINO, board as centred
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GENERIC = (0x049, 0x16E)
FAMILIES = [False, True]  # population alone; population with the hash
FAMILY_IDS = ["pop", "hash+pop"]


def engine(*a, **k):
    from gameoflife.engine import GolEngine
    return GolEngine(*a, **k)


def rule_obj(rule):
    from gameoflife.rules import Rule
    return Rule(rule[0], rule[1])


def popcount(packed):
    return int(np.unpackbits(np.ascontiguousarray(packed).view(np.uint8)).sum())


def reference(board, W, gens, topo=O.TORUS, rule=O.LIFE, rows=None):
    """(final board, hashes, populations[, populations of rows [lo, hi) per
    (lo, hi) of `rows`]) of `gens` oracle generations."""
    cur = np.ascontiguousarray(board, dtype=np.uint32)
    pops = np.zeros(gens, dtype=np.uint64)
    parts = [np.zeros(gens, dtype=np.uint64) for _ in rows or []]
    for g in range(gens):
        cur = O.step_packed(cur, W, topo, rule)
        pops[g] = popcount(cur)
        for part, (lo, hi) in zip(parts, rows or []):
            part[g] = popcount(cur[lo:hi])
    final, hashes = O.run_packed(board, W, gens, topo, rule)
    assert np.array_equal(final, cur)
    for a in (final, hashes, pops, *parts):
        a.setflags(write=False)
    return (final, hashes, pops, parts) if rows else (final, hashes, pops)


@functools.lru_cache(maxsize=None)
def torus_reference(W, H, gens, seed, rule=O.LIFE):
    board = O.seed_packed(W, H, seed)
    board.setflags(write=False)
    return (board,) + reference(board, W, gens, O.TORUS, rule)


def first_bad(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return f"first mismatch at generation {bad[0] + 1}: {got[bad[0]]} != {want[bad[0]]}" if bad.size else ""


def step_series(e, gens, with_hashes):
    """(hashes or None, populations) of e.step(..., populations=True)."""
    out = e.step(gens, hashes=with_hashes, populations=True)
    if with_hashes:
        assert isinstance(out, tuple) and len(out) == 2
        return out
    return None, out


def check_engine(e, board, W, gens, with_hashes, ref):
    final, hashes, pops = ref
    e.load(board)
    got_h, got_p = step_series(e, gens, with_hashes)
    assert got_p.dtype == np.uint64 and got_p.shape == (gens,)
    assert np.array_equal(got_p, pops), first_bad(got_p, pops)
    if with_hashes:
        assert np.array_equal(got_h, hashes), first_bad(got_h, hashes)
    assert e.epoch == gens
    bad = np.argwhere(e.snapshot() != final)
    assert bad.size == 0, f"first wrong word (row, col) {tuple(bad[0])}"
    assert e.population() == int(pops[-1])


def check_torus(W, H, gens, gpp, with_hashes, seed, rule=O.LIFE, band=0, lane_words=0, expect=None):
    board, *ref = torus_reference(W, H, gens, seed, rule)
    with engine(W, H, rule=rule_obj(rule)) as e:
        e.set_tuning(band_rows=band, gens_per_pass=gpp, words_per_lane=lane_words)
        if expect:
            expect(e)
        check_engine(e, board, W, gens, with_hashes, ref)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("gpp", range(1, 13))
@pytest.mark.parametrize("words", [2, 60, 124, 126, 128, 250, 254, 8190, 8191])
def test_tori_every_depth(gpu, words, gpp, with_hashes):
    check_torus(32 * words, 2 * gpp + 7, 2 * gpp + 1, gpp, with_hashes, seed=words * 13 + gpp)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
def test_whole_row_waves(gpu, with_hashes):
    def whole_row(e):
        assert e.occupancy(10)[1] == 128
    check_torus(4096, 37, 21, 10, with_hashes, seed=4096, expect=whole_row)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("rule,gpp", [(O.LIFE, 1), (O.LIFE, 2), (O.LIFE, 7), (O.LIFE, 12), (GENERIC, 2), (GENERIC, 7)])
def test_sixteen_byte_lanes(gpu, rule, gpp, with_hashes):
    check_torus(32 * 256, 2 * gpp + 7, 2 * gpp + 1, gpp, with_hashes, seed=gpp, rule=rule, lane_words=4)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("gpp", [2, 7, 12])
@pytest.mark.parametrize("band", [1, 3, 16, 1000])
def test_bands(gpu, band, gpp, with_hashes):
    # short bands: the direction switch, and the own_row gate at both ends of a band
    check_torus(32 * 254, 61, 2 * gpp, gpp, with_hashes, seed=band, band=band)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("gpp", [3, 8])
@pytest.mark.parametrize("rule", [GENERIC, O.REF_LITERAL, O.REF_EFFECTIVE])
def test_generic_rules(gpu, rule, gpp, with_hashes):
    check_torus(32 * 380, 29, gpp + 3, gpp, with_hashes, seed=gpp, rule=rule)


@functools.lru_cache(maxsize=None)
def clipped_reference(W, H, gens, seed):
    rng = np.random.default_rng(seed)
    board = O.pack((rng.random((H, W)) < 0.5).astype(np.uint8))
    board.setflags(write=False)
    return (board,) + reference(board, W, gens, O.REF_CLIPPED, O.LIFE)


def check_clipped(W, gpp, with_hashes, lane_words=0):
    """A half-full board, so the sink row and column hold live cells: they are
    stored cells and count, as in the census."""
    H, gens = 23, 2 * gpp + 1
    board, final, hashes, pops = clipped_reference(W, H, gens, W * 3 + gpp)
    assert popcount(board[H - 1]) > 0 and O.unpack(board, W)[:, W - 1].any()  # live sink cells to start from
    with engine(W, H, topology="ref-clipped") as e:
        e.set_tuning(gens_per_pass=gpp, words_per_lane=lane_words)
        check_engine(e, board, W, gens, with_hashes, (final, hashes, pops))
        assert e.census()["population"] == int(pops[-1])
        # generation by generation, the series is the census of that epoch
        e.load(board)
        for g in range(3):
            _, p = step_series(e, 1, with_hashes)
            assert int(p[0]) == e.census()["population"] == int(pops[g])


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("gpp", [1, 2, 5, 8])
@pytest.mark.parametrize("W", [7, 100, 32 * 62 + 5, 32 * 300 + 17])
def test_clipped_boards(gpu, W, gpp, with_hashes):
    check_clipped(W, gpp, with_hashes)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("gpp", [2, 7])  # 7: the deepest clipped 16-byte-lane instance built
@pytest.mark.parametrize("W", [32 * 11 + 5, 32 * 303 + 17])
def test_clipped_boards_sixteen_byte_lanes(gpu, W, gpp, with_hashes):
    # The vertical-first multi-generation kernel's series instances on a clipped
    # board.  A row of 16-byte lanes is a multiple of 4 words (gol_set_tuning
    # refuses others), so: 12 words -- one strip, 3 of its 62 lanes, a partial
    # last word -- and 304 words -- two strips (248 + 56), a partial last word.
    check_clipped(W, gpp, with_hashes, lane_words=4)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
def test_chunk_boundary(gpu, with_hashes):
    # the step plans, accumulates and folds per 1024 generations
    W, H, gens = 128, 64, 1030
    board, *ref = torus_reference(W, H, gens, 1030)
    with engine(W, H) as e:
        check_engine(e, board, W, gens, with_hashes, ref)


def shard_rows_of(H, n):
    from gameoflife.shard import shard_rows_py
    return [shard_rows_py(H, k, n) for k in range(n)]


@functools.lru_cache(maxsize=None)
def sharded_reference(W, H, gens, seed, n):
    board = O.seed_packed(W, H, seed)
    board.setflags(write=False)
    rows = tuple((r0, r0 + rows) for r0, rows in shard_rows_of(H, n))
    return (board,) + reference(board, W, gens, rows=rows)


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("gpp", [2, 12])
def test_shard_group(gpu, n, gpp, with_hashes):
    from gameoflife.engine import ShardGroup
    W, H, gens = 32 * 252, 83, 2 * gpp + 1
    board, final, hashes, pops, _ = sharded_reference(W, H, gens, 21 + n, n)
    shards = []
    for r0, rows in shard_rows_of(H, n):
        e = engine(W, H, row0=r0, rows=rows)
        e.set_tuning(gens_per_pass=gpp)
        e.load(board[r0:r0 + rows])
        shards.append(e)
    g = ShardGroup(shards)
    try:
        with pytest.raises(ValueError):
            g.step(1, partials=True, populations=True)
        assert g.epoch == 0
        got_h, got_p = step_series(g, gens, with_hashes)
        assert np.array_equal(got_p, pops), first_bad(got_p, pops)  # the unsharded series
        if with_hashes:
            assert np.array_equal(got_h, hashes), first_bad(got_h, hashes)
        assert (g.snapshot() == final).all()
        assert g.population() == int(pops[-1])
    finally:
        g.close()
        for s in shards:
            s.close()


def run_threads(engs, fn):
    out, errs = [None] * len(engs), []

    def work(r):
        try:
            out[r] = fn(r, engs[r])
        except Exception as exc:  # noqa: BLE001 -- reported to the test thread
            errs.append(exc)

    ts = [threading.Thread(target=work, args=(r,)) for r in range(len(engs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not any(t.is_alive() for t in ts), "a rank hung"
    if errs:
        raise errs[0]
    return out


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("gpp", [2, 12])
def test_loopback_ring_two_ranks(gpu, gpp, with_hashes):
    """Two loopback ranks on two threads: each rank's series is its own rows'
    population, and the ring's all-reduce of the partials is the board's."""
    W, H, gens, n = 32 * 252, 83, 2 * gpp + 1, 2
    board, final, hashes, pops, parts = sharded_reference(W, H, gens, 21 + n, n)
    key = uuid.uuid4().hex
    engs = []
    for r, (r0, rows) in enumerate(shard_rows_of(H, n)):
        e = engine(W, H, row0=r0, rows=rows)
        e.set_tuning(gens_per_pass=gpp)
        e.load(board[r0:r0 + rows])
        e.comm_init_loopback(key, r, n)
        engs.append(e)

    def work(r, e):
        h, p = step_series(e, gens, with_hashes)
        return p, e.allreduce_u64(p), e.allreduce_u64(h) if with_hashes else None

    try:
        res = run_threads(engs, work)
        for r, (part, total, hsum) in enumerate(res):
            assert np.array_equal(part, parts[r]), (r, first_bad(part, parts[r]))
            assert np.array_equal(total, pops), (r, first_bad(total, pops))
            if with_hashes:
                assert np.array_equal(hsum, hashes), (r, first_bad(hsum, hashes))
        assert (np.vstack([e.snapshot() for e in engs]) == final).all()
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("gpp", [2, 12])
def test_rccl_self_ring(gpu, gpp, with_hashes):
    from gameoflife import _native as N
    W, H, gens = 32 * 252, 83, 2 * gpp + 1
    board, final, hashes, pops, _ = sharded_reference(W, H, gens, 23, 2)
    with engine(W, H) as e:
        e.set_tuning(gens_per_pass=gpp)
        e.comm_init(N.unique_id(), 0, 1)
        check_engine(e, board, W, gens, with_hashes, (final, hashes, pops))


GLIDER = [(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)]


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
def test_active_rows_glider(gpu, with_hashes):
    """The rows a sparse pass does not launch are dead and add 0: a glider has
    5 cells at every generation."""
    W, H, gens = 2048, 512, 200
    cells = np.zeros((H, W), dtype=np.uint8)
    for x, y in GLIDER:
        cells[H // 2 + y, W // 2 + x] = 1
    board = O.pack(cells)
    final, hashes = O.run_packed(board, W, gens)
    with engine(W, H, active_rows=True) as e:
        e.load(board)
        got_h, got_p = step_series(e, gens, with_hashes)
        assert got_p.tolist() == [5] * gens
        if with_hashes:
            assert np.array_equal(got_h, hashes), first_bad(got_h, hashes)
        assert e.active_stats()["sparse_passes"] > 0
        assert (e.snapshot() == final).all()
        assert e.population() == 5


@pytest.mark.parametrize("with_hashes", FAMILIES, ids=FAMILY_IDS)
def test_active_rows_gosper_gun(gpu, with_hashes):
    W, gens = 1024, 240
    board = centred(O.pack, W, GOSPER_GUN)
    final, hashes, pops = reference(board, W, gens)
    assert int(pops[29]) == 41 and int(pops[149]) == 61  # 5 cells more every 30 generations
    runs = {}
    for active in (False, True):
        with engine(W, W, active_rows=active) as e:
            e.load(board)
            runs[active] = step_series(e, gens, with_hashes)
            if active:
                assert e.active_stats()["sparse_passes"] > 0
            assert (e.snapshot() == final).all()
            assert e.population() == int(pops[-1])
    assert np.array_equal(runs[True][1], runs[False][1]), first_bad(runs[True][1], runs[False][1])
    assert np.array_equal(runs[True][1], pops), first_bad(runs[True][1], pops)
    if with_hashes:
        assert np.array_equal(runs[True][0], hashes) and np.array_equal(runs[False][0], hashes)


def test_r_pentomino_known_answer(gpu):
    """1200 generations of the R-pentomino on a 512 x 512 torus against the
    oracle.  The torus is small enough for its gliders to wrap, so the
    open-plane value 116 is asserted only if the oracle's run gives it."""
    W, gens = 512, 1200
    board = centred(O.pack, W, R_PENTOMINO)
    final, hashes, pops = reference(board, W, gens)
    with engine(W, W) as e:
        check_engine(e, board, W, gens, True, (final, hashes, pops))
        e.load(board)
        _, alone = step_series(e, gens, False)
    assert np.array_equal(alone, pops), first_bad(alone, pops)
    if int(pops[1102]) == 116:
        assert int(alone[1102]) == 116


def test_arguments(gpu):
    from gameoflife import _native as N
    W, H = 128, 64
    board, final, hashes, pops = torus_reference(W, H, 1030, 1030)
    u64p = N._u64p
    with engine(W, H) as e:
        e.load(board)
        pop = np.full(8, 77, dtype=np.uint64)
        h = np.full(8, 77, dtype=np.uint64)
        # a short capacity: GOL_EINVAL, the epoch unchanged, nothing written
        for hp, pp in ((None, pop), (h, None), (h, pop)):
            rc = N.lib.gol_step_series(e._h, 8, hp.ctypes.data_as(u64p) if hp is not None else None,
                                       pp.ctypes.data_as(u64p) if pp is not None else None, 7)
            assert rc == N.GOL_EINVAL
            assert e.epoch == 0
        assert pop.tolist() == [77] * 8 and h.tolist() == [77] * 8
        # generations = 0
        assert N.lib.gol_step_series(e._h, 0, None, pop.ctypes.data_as(u64p), 0) == N.GOL_OK
        assert N.lib.gol_step_series(e._h, 0, None, None, 0) == N.GOL_OK
        assert e.epoch == 0 and e.step(0, populations=True).shape == (0,)
        # both arrays null: gol_step(ctx, n, NULL); the capacity is not looked at
        assert N.lib.gol_step_series(e._h, 5, None, None, 0) == N.GOL_OK
        e.sync()
        assert e.epoch == 5 and e.population() == int(pops[4])
        # a capacity larger than the call: only `generations` entries are written
        assert N.lib.gol_step_series(e._h, 3, h.ctypes.data_as(u64p), pop.ctypes.data_as(u64p), 8) == N.GOL_OK
        assert pop.tolist() == pops[5:8].tolist() + [77] * 5
        assert h.tolist() == hashes[5:8].tolist() + [77] * 5
        # hashes alone through the series call is gol_step's hashed step
        assert N.lib.gol_step_series(e._h, 2, h.ctypes.data_as(u64p), None, 8) == N.GOL_OK
        assert h[:2].tolist() == hashes[8:10].tolist() and e.epoch == 10


def test_group_arguments(gpu):
    from gameoflife import _native as N
    from gameoflife.engine import ShardGroup
    W, H = 32 * 252, 83
    board, final, hashes, pops, _ = sharded_reference(W, H, 5, 23, 2)
    shards = []
    for r0, rows in shard_rows_of(H, 2):
        e = engine(W, H, row0=r0, rows=rows)
        e.load(board[r0:r0 + rows])
        shards.append(e)
    g = ShardGroup(shards)
    try:
        pop = np.zeros(5, dtype=np.uint64)
        assert N.lib.gol_group_step_series(g._h, 5, None, pop.ctypes.data_as(N._u64p), 4) == N.GOL_EINVAL
        assert g.epoch == 0
        assert N.lib.gol_group_step_series(g._h, 0, None, None, 0) == N.GOL_OK
        assert N.lib.gol_group_step_series(g._h, 2, None, None, 0) == N.GOL_OK
        g.sync()
        assert g.epoch == 2
        got = g.step(3, populations=True)
        assert got.tolist() == pops[2:5].tolist()
    finally:
        g.close()
        for s in shards:
            s.close()


@pytest.mark.parametrize("gpp", [0, 1, 12])
def test_no_side_effect_on_gol_step(gpu, gpp):
    """After a series call the slots are clean: a hashed gol_step still gives
    the oracle's hashes (its fold reads the hash word of every slot only)."""
    W, H, gens = 32 * 254, 61, 48
    board, final, hashes, pops = torus_reference(W, H, gens, 61)
    with engine(W, H) as e:
        e.set_tuning(gens_per_pass=gpp)
        e.load(board)
        _, p = step_series(e, 12, False)
        h1 = e.step(12, hashes=True)
        h2, p2 = step_series(e, 12, True)
        h3 = e.step(12, hashes=True)
        assert e.hash() == int(hashes[-1])
        assert (e.snapshot() == final).all()
    assert np.array_equal(p, pops[:12]) and np.array_equal(p2, pops[24:36])
    assert np.array_equal(np.concatenate([h1, h2, h3]), hashes[12:]), first_bad(np.concatenate([h1, h2, h3]),
                                                                                hashes[12:])
