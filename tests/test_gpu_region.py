"""GPU: gol_read_region / gol_write_region against the numpy region model
(tests/region_model.py) on the smallest boards that carry each device layout:
every window shape that takes another path through the gather and scatter
kernels (aligned, unaligned, one bit, word-crossing, both seams, as wide as
the board), the four modes, pitch and padding rules, shards, stepping after
an edit, and the refusals."""
import ctypes

import numpy as np
import pytest

import region_model as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (topology, W, H): one pair; three words (row-major torus); pairs; the
# reference's default geometry; three words, the last one partial
BOARDS = [("torus", 64, 8), ("torus", 96, 8), ("torus", 256, 16), ("ref-clipped", 7, 7), ("ref-clipped", 70, 9)]
BOARD_IDS = [f"{t}-{w}x{h}" for t, w, h in BOARDS]
EPOCH = 2  # the boards are stepped before the edits: a reset epoch would show


def windows(topology, W, H):
    """(x0, y0, w, h) of the issue's list that fit the board."""
    torus = topology == "torus"
    cand = [(0, 0, 1, 1), (5, 1, 31, 3), (5, 1, 33, 3), (31, 0, 2, 1), (32, 2, 32, 2), (3, 3, 67, 4), (0, 0, W, H)]
    if torus:
        cand += [(W - 2, H - 2, 5, 5), (5, 0, W, 2), (W - 1, 0, 1, H)]
    else:
        cand += [(2, 1, 4, 3), (W - 3, H - 2, 3, 2)]  # small enough for 7 x 7; flush with the far corner
    fits = [c for c in cand if c[2] <= W and c[3] <= H and c[0] < W and c[1] < H
            and (torus or (c[0] + c[2] <= W and c[1] + c[3] <= H))]
    assert len(fits) >= 4, fits
    return fits


def start(engine_cls, topology, W, H, seed=11, **kw):
    e = engine_cls(W, H, topology=topology, **kw)
    e.seed(seed)
    return e


def check_board(e, model, W, epoch=EPOCH):
    want = O.pack(model)
    np.testing.assert_array_equal(e.snapshot(), want)  # word for word: padding bits included
    assert e.hash() == O.hash_packed(want, W)
    assert e.epoch == epoch


def pattern(rng, w, h):
    return (rng.random((h, w)) < 0.5).astype(np.uint8)


@pytest.mark.parametrize("topology,W,H", BOARDS, ids=BOARD_IDS)
def test_windows_match_the_model(gpu, topology, W, H):
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    torus = topology == "torus"
    rng = np.random.default_rng(W * 100 + H)
    with start(GolEngine, topology, W, H) as e:
        e.step(EPOCH)
        model = codec.unpack(e.snapshot(), W)
        for x0, y0, w, h in windows(topology, W, H):
            np.testing.assert_array_equal(e.read_region(x0, y0, w, h), M.read_region(model, x0, y0, w, h, torus),
                                          err_msg=str((x0, y0, w, h)))
            assert e.epoch == EPOCH
            p = pattern(rng, w, h)
            e.write_region(x0, y0, p)
            model = M.write_region(model, x0, y0, p, "copy", torus)
            check_board(e, model, W)
            np.testing.assert_array_equal(e.read_region(x0, y0, w, h), p)


@pytest.mark.parametrize("topology,W,H", BOARDS, ids=BOARD_IDS)
def test_modes(gpu, topology, W, H):
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    torus = topology == "torus"
    x0, y0, w, h = (5, 1, 33, 3) if W >= 38 else (2, 1, 4, 3)
    rng = np.random.default_rng(7)
    with start(GolEngine, topology, W, H) as e:
        e.step(EPOCH)
        model = codec.unpack(e.snapshot(), W)
        for mode in M.MODES:
            p = pattern(rng, w, h)
            e.write_region(x0, y0, p, mode)
            model = M.write_region(model, x0, y0, p, mode, torus)
            check_board(e, model, W)
        e.set_cell(x0, y0, True)
        e.set_cell(x0 + 1, y0, False)
        model[y0, x0], model[y0, x0 + 1] = 1, 0
        check_board(e, model, W)
        with pytest.raises(ValueError):
            e.write_region(x0, y0, p, "and")


def raw_write(e, x0, y0, w, h, packed, mode=0):
    from gameoflife import _native as N
    return N.lib.gol_write_region(e._h, x0, y0, w, h, packed.ctypes.data_as(N._u32p), packed.shape[1], mode)


def raw_read(e, x0, y0, w, h, packed):
    from gameoflife import _native as N
    return N.lib.gol_read_region(e._h, x0, y0, w, h, packed.ctypes.data_as(N._u32p), packed.shape[1])


@pytest.mark.parametrize("topology,W,H,win", [("torus", 256, 16, (250, 14, 45, 4)), ("torus", 96, 8, (70, 1, 45, 3)),
                                              ("ref-clipped", 70, 9, (40, 1, 30, 3))],
                         ids=["pairs", "row-major", "clipped-flush-right"])
def test_wide_pitch_and_dirty_bits(gpu, topology, W, H, win):
    """A host pitch wider than the window, with every bit past w set: none
    reaches the board (on the clipped board the window ends at the last stored
    column, so they would land in the padding bits), and a read zeroes the
    bits past w of a row's last word and leaves the words after it alone."""
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    torus = topology == "torus"
    x0, y0, w, h = win
    sw, pitch = (w + 31) // 32, (w + 31) // 32 + 2
    rng = np.random.default_rng(3)
    with start(GolEngine, topology, W, H) as e:
        e.step(EPOCH)
        model = codec.unpack(e.snapshot(), W)
        p = pattern(rng, w, h)
        packed = np.full((h, pitch), 0xFFFFFFFF, dtype=np.uint32)
        packed[:, :sw] = codec.pack(p)
        packed[:, sw - 1] |= np.uint32((0xFFFFFFFF << (w % 32)) & 0xFFFFFFFF)  # w % 32 != 0 in every case here
        assert raw_write(e, x0, y0, w, h, packed) == 0
        model = M.write_region(model, x0, y0, p, "copy", torus)
        check_board(e, model, W)
        out = np.full((h, pitch), 0xDEADBEEF, dtype=np.uint32)
        assert raw_read(e, x0, y0, w, h, out) == 0
        np.testing.assert_array_equal(out[:, :sw], codec.pack(p))
        assert (out[:, sw:] == 0xDEADBEEF).all()


def make_group(W, H, blocks, seed):
    from gameoflife.engine import GolEngine, ShardGroup
    shards, r0 = [], 0
    for rows in blocks:
        e = GolEngine(W, H, row0=r0, rows=rows)
        e.seed(seed)
        shards.append(e)
        r0 += rows
    assert r0 == H
    return shards, ShardGroup(shards)


def test_shard_group_fills_and_writes_one_window(gpu):
    """Row blocks of 5, 5 and 6 rows: a window across two shards, and one that
    wraps from the last shard to the first (and across the x seam), give what
    a single context gives; the group steps on from the edited board."""
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    W, H, seed = 256, 16, 5
    rng = np.random.default_rng(9)
    shards, group = make_group(W, H, (5, 5, 6), seed)
    with GolEngine(W, H) as single:
        single.seed(seed)
        group.step(EPOCH)
        single.step(EPOCH)
        model = codec.unpack(single.snapshot(), W)
        for x0, y0, w, h in [(3, 3, 67, 4), (250, 14, 10, 5), (0, 0, W, H)]:
            want = M.read_region(model, x0, y0, w, h)
            np.testing.assert_array_equal(group.read_region(x0, y0, w, h), want)
            np.testing.assert_array_equal(single.read_region(x0, y0, w, h), want)
            p = pattern(rng, w, h)
            for mode in ("xor", "copy"):
                group.write_region(x0, y0, p, mode)
                single.write_region(x0, y0, p, mode)
                model = M.write_region(model, x0, y0, p, mode)
                check_board(single, model, W)
                np.testing.assert_array_equal(group.snapshot(), O.pack(model))
                assert group.hash() == single.hash()
                assert group.epoch == EPOCH
        # halos are exchanged again at the next pass: the edit reaches the neighbours
        np.testing.assert_array_equal(group.step(6, hashes=True), single.step(6, hashes=True))
        np.testing.assert_array_equal(group.snapshot(), single.snapshot())
    group.close()
    for s in shards:
        s.close()


def test_window_that_misses_the_shard(gpu):
    from gameoflife.engine import GolEngine
    W, H = 256, 16
    with GolEngine(W, H, row0=5, rows=5) as e:
        e.seed(5)
        before, snap = e.hash(), e.snapshot()
        ones = np.full((3, 1), 0x3FF, dtype=np.uint32)
        for y0 in (0, 10, 14):  # above, below, and wrapping over the seam: rows 14, 15 and 0
            assert raw_write(e, 0, y0, 10, 3, ones) == 0
            out = np.full((3, 1), 0xDEADBEEF, dtype=np.uint32)
            assert raw_read(e, 0, y0, 10, 3, out) == 0
            assert (out == 0xDEADBEEF).all()
        assert e.hash() == before and e.epoch == 0
        np.testing.assert_array_equal(e.snapshot(), snap)
        # rows 3 .. 6 of the board: only 5 and 6 are this shard's
        assert raw_write(e, 0, 3, 10, 4, np.full((4, 1), 0x3FF, dtype=np.uint32), 0) == 0
        snap[0:2, 0] |= 0x3FF
        np.testing.assert_array_equal(e.snapshot(), snap)
        out = np.full((4, 1), 0xDEADBEEF, dtype=np.uint32)
        assert raw_read(e, 0, 3, 10, 4, out) == 0
        assert out[:, 0].tolist() == [0xDEADBEEF, 0xDEADBEEF, 0x3FF, 0x3FF]


def test_place_then_step_follows_the_oracle(gpu):
    """A glider across the corner seam at epoch 0, a second one at epoch 8:
    every hash and the final board equal the oracle's run of the same edits."""
    from gameoflife.engine import GolEngine
    W = 64
    glider = "bob$2bo$3o!"
    cells = np.zeros((W, W), dtype=np.uint8)
    g = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)
    with GolEngine(W, W) as e:
        e.place(glider, W - 2, W - 2)
        cells = M.write_region(cells, W - 2, W - 2, g, "or")
        assert e.epoch == 0 and e.population() == 5
        got1 = e.step(8, hashes=True)
        board, want1 = O.run_packed(O.pack(cells), W, 8)
        np.testing.assert_array_equal(got1, want1)
        e.place([".O.", "..O", "OOO"], 10, 10, mode="or")
        cells = M.write_region(O.unpack(board, W), 10, 10, g, "or")
        assert e.epoch == 8 and e.population() == 10
        got2 = e.step(8, hashes=True)
        board, want2 = O.run_packed(O.pack(cells), W, 8)
        np.testing.assert_array_equal(got2, want2)
        assert e.epoch == 16
        np.testing.assert_array_equal(e.read_region(0, 0, W, W), O.unpack(board, W))


def test_refusals(gpu):
    from gameoflife import _native as N
    from gameoflife.engine import GolEngine
    buf = np.zeros((16, 8), dtype=np.uint32)
    p = buf.ctypes.data_as(N._u32p)
    null = ctypes.cast(None, N._u32p)

    def refused(e, rc):
        assert rc == N.GOL_EINVAL
        assert N.lib.gol_last_error(e._h if e is not None else None)
        assert N.take_hip_error() == 0

    with GolEngine(256, 16) as e:
        e.seed(3)
        e.step(3)
        before = e.hash()
        bad_windows = [(0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 257, 1), (0, 0, 1, 17), (-1, 0, 1, 1), (256, 0, 1, 1),
                       (0, -1, 1, 1), (0, 16, 1, 1)]
        for x0, y0, w, h in bad_windows:
            refused(e, N.lib.gol_read_region(e._h, x0, y0, w, h, p, 8))
            refused(e, N.lib.gol_write_region(e._h, x0, y0, w, h, p, 8, N.GOL_REGION_OR))
        refused(e, N.lib.gol_read_region(e._h, 0, 0, 8, 8, null, 8))
        refused(e, N.lib.gol_write_region(e._h, 0, 0, 8, 8, null, 8, 0))
        refused(e, N.lib.gol_read_region(e._h, 0, 0, 65, 2, p, 2))   # three words per window row
        refused(e, N.lib.gol_write_region(e._h, 0, 0, 65, 2, p, 2, 0))
        for mode in (-1, 4):
            refused(e, N.lib.gol_write_region(e._h, 0, 0, 8, 8, p, 8, mode))
        refused(e, N.lib.gol_census(e._h, None))
        refused(None, N.lib.gol_read_region(None, 0, 0, 1, 1, p, 8))
        refused(None, N.lib.gol_write_region(None, 0, 0, 1, 1, p, 8, 0))
        refused(None, N.lib.gol_census(None, ctypes.byref(N.GolCensusResult())))
        assert e.hash() == before and e.epoch == 3
    with GolEngine(70, 9, topology="ref-clipped") as e:
        e.seed(3)
        before = e.hash()
        for x0, y0, w, h in [(60, 0, 11, 1), (0, 8, 1, 2), (69, 8, 2, 2)]:  # a clipped board does not wrap
            refused(e, N.lib.gol_read_region(e._h, x0, y0, w, h, p, 8))
            refused(e, N.lib.gol_write_region(e._h, x0, y0, w, h, p, 8, 0))
        assert N.lib.gol_read_region(e._h, 60, 8, 10, 1, p, 8) == N.GOL_OK  # flush with the corner
        assert e.hash() == before


def test_edit_between_asynchronous_steps_and_snapshots(gpu):
    """Ordering: a write queued behind an unhashed (asynchronous) step edits
    the stepped board, and a snapshot in flight keeps the board it was started
    on."""
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    W, H = 256, 64
    rng = np.random.default_rng(12)
    p = pattern(rng, 70, 9)
    board = O.seed_packed(W, H, 21)
    with GolEngine(W, H) as e:
        e.seed(21)
        e.step(13)  # not waited for
        e.write_region(200, 60, p, "xor")
        stepped, _ = O.run_packed(board, W, 13)
        model = M.write_region(codec.unpack(stepped, W), 200, 60, p, "xor")
        check_board(e, model, W, epoch=13)
        buf = e.host_buffer()
        e.snapshot_async(buf)
        e.write_region(0, 0, np.ones((H, W), dtype=np.uint8), "clear")
        assert e.snapshot_wait() == 13
        np.testing.assert_array_equal(buf, O.pack(model))
        assert e.census() == {"population": 0, "bbox": None}


RING = (256, 32, 17)  # W, H, seed of the two ring tests


def ring_case():
    """A pattern across the y seam (and the x seam) at epoch 4, then 9 hashed
    generations: (pattern, edited board as cells, final packed board, hashes)."""
    from gameoflife import codec
    W, H, seed = RING
    p = pattern(np.random.default_rng(13), 40, 6)
    start, _ = O.run_packed(O.seed_packed(W, H, seed), W, 4)
    model = M.write_region(codec.unpack(start, W), 230, H - 3, p, "copy")
    want_board, want = O.run_packed(O.pack(model), W, 9)
    return p, model, want_board, want


def test_edit_on_an_rccl_ring(gpu):
    """With a communicator attached -- a ring of one rank, whose halo rows go
    out and come back through RCCL: the next pass's exchange carries the edit."""
    from gameoflife import _native as N
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    W, H, seed = RING
    p, model, want_board, want = ring_case()
    with GolEngine(W, H) as e:
        e.seed(seed)
        e.comm_init(N.unique_id(), 0, 1)
        e.step(4)
        e.write_region(230, H - 3, p)
        assert e.epoch == 4 and e.hash() == O.hash_packed(O.pack(model), W)
        np.testing.assert_array_equal(e.step(9, hashes=True), want)
        np.testing.assert_array_equal(e.read_region(0, 0, W, H), codec.unpack(want_board, W))


def test_edit_on_a_loopback_ring(gpu):
    """Two loopback ranks of one board: the same call with the same buffer on
    both shards writes and reads a window across the seam between them."""
    import threading
    import uuid

    from gameoflife import codec
    from gameoflife.engine import GolEngine
    W, H, seed = RING
    p, model, want_board, want = ring_case()
    key = uuid.uuid4().hex
    engs = []
    for r in range(2):
        e = GolEngine(W, H, row0=16 * r, rows=16)
        e.seed(seed)
        e.comm_init_loopback(key, r, 2)
        engs.append(e)

    def threads(fn):
        out, errs = [None] * 2, []

        def work(r):
            try:
                out[r] = fn(engs[r])
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)
        ts = [threading.Thread(target=work, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        return out

    try:
        threads(lambda e: (e.step(4), e.sync()))
        packed = np.zeros((6, 2), dtype=np.uint32)
        for e in engs:  # the same call with the same buffer on every shard
            e.write_region(230, H - 3, p)
            e._read_region_into(230, H - 3, 40, 6, packed)
        np.testing.assert_array_equal(codec.unpack(packed, 40), p)
        assert (engs[0].hash() + engs[1].hash()) % 2**64 == O.hash_packed(O.pack(model), W)
        got = threads(lambda e: e.allreduce_u64(e.step(9, hashes=True)))
        np.testing.assert_array_equal(got[0], want)
        np.testing.assert_array_equal(np.vstack([e.snapshot() for e in engs]), want_board)
    finally:
        for e in engs:
            e.close()
