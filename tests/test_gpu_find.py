"""GPU: gol_find against the brute-force model (tests/find_model.py), which
reads the engine's own snapshot.  Every comparison is exact.  The search kernel
runs on the smallest boards of each device layout with patterns cut from the
board (so every case has a match): one cell, boxes inside a word, wider than a
word, as wide as the row, across both seams, past a clipped board's corner,
under a care mask, and all dead; with windows of anchors that are whole,
unaligned, wrapped and flush with the far corner.  Then truncation, known
answers, the live-row shortcut, shards, ordering and the refusals."""
import ctypes

import numpy as np
import pytest

import find_model as F
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPOCH = 2  # boards are seeded and stepped: a search of the seeded plane alone would not show a stale plane
BOARDS = [("torus", 64, 8), ("torus", 96, 8), ("torus", 256, 16), ("ref-clipped", 7, 7), ("ref-clipped", 70, 9)]
BOARD_IDS = [f"{t}-{w}x{h}" for t, w, h in BOARDS]
GLIDER = [".O.", "..O", "OOO"]
BLOCK = ["OO", "OO"]


def stepped(topology, W, H, seed=11, **kw):
    """(engine, its board as cells) after EPOCH generations."""
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    e = GolEngine(W, H, topology=topology, **kw)
    e.seed(seed)
    e.step(EPOCH)
    return e, codec.unpack(e.snapshot(), W)


def cut(board, x, y, pw, ph, torus):
    """The pw x ph box of the board at anchor (x, y): wrapped on a torus,
    padded dead beyond a clipped board."""
    H, W = board.shape
    if torus:
        return board[(y + np.arange(ph)) % H][:, (x + np.arange(pw)) % W].copy()
    out = np.zeros((ph, pw), dtype=np.uint8)
    part = board[y:y + ph, x:x + pw]
    out[:part.shape[0], :part.shape[1]] = part
    return out


def board_patterns(board, topology, W, H):
    """(name, cells, care, anchor it was cut at or None)."""
    torus = topology == "torus"
    full = lambda c: np.ones_like(c)
    pats = [("one-live-cell", np.ones((1, 1), dtype=np.uint8), np.ones((1, 1), dtype=np.uint8), None)]
    c = cut(board, 2, 2, 3, 3, torus)
    pats.append(("box3", c, full(c), (2, 2)))
    if torus:
        c = cut(board, W - 2, H - 2, 5, 5, True)
        pats.append(("box5-both-seams", c, full(c), (W - 2, H - 2)))
    if W >= 40:
        c = cut(board, 3, 1, 40, 3, torus)
        pats.append(("box40x3", c, full(c), (3, 1)))
    if (topology, W, H) == BOARDS[0]:
        c = cut(board, 5, 3, 64, 8, True)
        pats.append(("whole-board", c, full(c), (5, 3)))
    c = np.zeros((3, 3), dtype=np.uint8)
    pats.append(("dead3", c, full(c), None))
    c = cut(board, 0, 1, 6, 5, torus)
    care = (np.random.default_rng(99).random((5, 6)) < 0.5).astype(np.uint8)
    care[2, 3] = 1
    pats.append(("masked6x5", c & care, care, (0, 1)))
    if not torus:
        c = cut(board, W - 2, H - 2, 3, 3, False)
        assert not c[2].any() and not c[:, 2].any()  # the part beyond the board reads dead
        pats.append(("corner-padded", c, full(c), (W - 2, H - 2)))
    return pats


def board_windows(topology, W, H):
    wins = [(0, 0, W, H)]
    if W >= 38 and H >= 4:
        wins.append((5, 1, 33, 3))
    wins.append((W - 2, H - 2, 5, 5) if topology == "torus" else (W - 3, H - 2, 3, 2))
    return wins


def check(e, board, torus, cells, care, win, label):
    H, W = board.shape
    want = F.find(board, cells, care, torus, *win)
    got = e.find(cells, care=care, x=win[0], y=win[1], w=win[2], h=win[3], max_matches=W * H)
    assert got["count"] == len(want), (label, win, got["count"], len(want))
    assert got["matches"].dtype == np.int64
    np.testing.assert_array_equal(got["matches"], want, err_msg=str((label, win)))
    return got


@pytest.mark.parametrize("topology,W,H", BOARDS, ids=BOARD_IDS)
def test_small_boards_match_the_model(gpu, topology, W, H):
    torus = topology == "torus"
    e, board = stepped(topology, W, H)
    with e:
        before = e.hash()
        names = []
        for name, cells, care, anchor in board_patterns(board, topology, W, H):
            names.append(name)
            whole = F.find(board, cells, care, torus)
            if anchor is not None:  # cut from the board: never vacuous
                assert len(whole) >= 1 and list(anchor) in whole.tolist(), name
            for win in board_windows(topology, W, H):
                got = check(e, board, torus, cells, care, win, name)
                if name == "one-live-cell" and win == (0, 0, W, H):
                    assert got["count"] == e.population() == int(board.sum())
        assert len(names) >= 5 and ("box40x3" in names) == (W >= 40)
        assert e.epoch == EPOCH and e.hash() == before


# ---- the raw call ----
def raw(e, win, cells, care, xy, max_matches, res, pitch=None, pw=None, ph=None, null_pattern=False, null_res=False,
        null_ctx=False):
    from gameoflife import _native as N
    from gameoflife import codec
    pat = codec.pack(cells)
    mask = codec.pack(care) if care is not None else None
    return N.lib.gol_find(None if null_ctx else e._h, *win,
                          None if null_pattern else pat.ctypes.data_as(N._u32p),
                          mask.ctypes.data_as(N._u32p) if mask is not None else None,
                          pat.shape[1] if pitch is None else pitch,
                          cells.shape[1] if pw is None else pw, cells.shape[0] if ph is None else ph,
                          xy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if xy is not None else None,
                          max_matches, None if null_res else ctypes.byref(res))


def test_truncation_and_count_only(gpu):
    from gameoflife import _native as N
    W, H = 256, 16
    e, board = stepped("torus", W, H)
    with e:
        one = np.ones((1, 1), dtype=np.uint8)
        want = F.find(board, one, one, True)
        assert len(want) > 5
        got = e.find(one, max_matches=5)
        assert got["count"] == len(want) and got["matches"].shape == (5, 2)
        pairs = [tuple(p) for p in got["matches"].tolist()]
        assert len(set(pairs)) == 5 and pairs == sorted(pairs, key=lambda p: (p[1], p[0]))
        assert set(pairs) <= {tuple(p) for p in want.tolist()}
        # count only: no list at all; a null care mask cares for every cell
        res = N.GolFindResult(9, 9, 9)
        assert raw(e, (0, 0, W, H), one, None, None, 0, res) == N.GOL_OK
        assert (res.count, res.returned, res.rows_searched) == (len(want), 0, H)
        # a wide pattern pitch and dirty bits at k >= pw in both buffers
        cells = cut(board, 3, 1, 5, 3, True)
        pat = np.full((3, 3), 0xFFFFFFE0, dtype=np.uint32)
        pat[:, 0] |= O.pack(cells)[:, 0]
        mask = np.full((3, 3), 0xFFFFFFFF, dtype=np.uint32)
        xy = np.zeros((64, 2), dtype=np.int64)
        rc = N.lib.gol_find(e._h, 0, 0, W, H, pat.ctypes.data_as(N._u32p), mask.ctypes.data_as(N._u32p), 3, 5, 3,
                            xy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 64, ctypes.byref(res))
        assert rc == N.GOL_OK
        want = F.find(board, cells, np.ones_like(cells), True)
        assert 1 <= len(want) <= 64 and res.count == res.returned == len(want)
        np.testing.assert_array_equal(xy[:res.returned], want)
        assert e.epoch == EPOCH


# ---- known answers, no model ----
def test_gliders_and_a_block_are_found_and_move(gpu):
    from gameoflife.engine import GolEngine
    spots = [(10, 10), (60, 20), (30, 90)]
    with GolEngine(128, 128) as e:
        for x, y in spots:
            e.place(GLIDER, x, y)
        e.place(BLOCK, 100, 100)
        for shift in (0, 1):  # the glider moves (+1, +1) every 4 generations
            got = e.find(GLIDER, border=1)
            want = sorted(((x - 1 + shift, y - 1 + shift) for x, y in spots), key=lambda p: (p[1], p[0]))
            assert got["count"] == 3 and [tuple(p) for p in got["matches"].tolist()] == want
            blk = e.find(BLOCK, border=1)
            assert blk["count"] == 1 and blk["matches"].tolist() == [[99, 99]]
            assert e.find(GLIDER)["count"] == 3  # the bare box finds them too
            if shift == 0:
                e.step(4)
        assert e.epoch == 4


# ---- live rows ----
def test_live_rows_narrow_the_search_and_never_the_result(gpu):
    from gameoflife import codec, patterns
    from gameoflife.engine import GolEngine
    W, H = 128, 1024
    with GolEngine(W, H) as e:
        e.place(GLIDER, 20, 512)   # the bordered pattern's anchor row is 511, in the block above the run
        e.place(GLIDER, 50, 1022)  # wraps the seam
        assert e.active_rows() is not None
        known = e.find(GLIDER, border=1)
        assert known["matches"].tolist() == [[19, 511], [49, 1021]] and known["count"] == 2
        assert 0 < known["rows_searched"] < H
        board = codec.unpack(e.snapshot(), W)
        dead = np.zeros((3, 3), dtype=np.uint8)
        got = e.find(dead)  # no live cared cell: every row, whatever is known
        assert got["rows_searched"] == H
        want = F.find(board, dead, np.ones_like(dead), True)
        assert got["count"] == len(want) > 65536 and got["matches"].shape == (65536, 2)
        assert {tuple(p) for p in got["matches"].tolist()} <= {tuple(p) for p in want.tolist()}
        np.testing.assert_array_equal(e.find(dead, x=3, y=500, w=40, h=30)["matches"],
                                      F.find(board, dead, np.ones_like(dead), True, 3, 500, 40, 30))
        # the same board, loaded: nothing is known about its rows
        epoch = e.epoch
        e.load(codec.pack(board))
        assert e.epoch == epoch == 0 and e.active_rows() is None
        unknown = e.find(GLIDER, border=1)
        np.testing.assert_array_equal(unknown["matches"], known["matches"])
        assert unknown["count"] == 2 and unknown["rows_searched"] == H
        cells, care = patterns.as_search(GLIDER, border=1)
        np.testing.assert_array_equal(unknown["matches"], F.find(board, cells, care, True))


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


@pytest.mark.parametrize("topology,W,H,blocks", [("torus", 256, 48, (16, 16, 16)), ("ref-clipped", 70, 9, (5, 4))],
                         ids=["torus-3", "clipped-2"])
def test_shards_and_the_group(gpu, topology, W, H, blocks):
    from gameoflife import _native as N
    from gameoflife import codec
    torus = topology == "torus"
    shards, group = make_group(topology, W, H, blocks)
    try:
        group.step(EPOCH)
        board = codec.unpack(group.snapshot(), W)
        bounds = list(np.cumsum(blocks))  # the rows below each boundary; the last one is the torus seam
        if not torus:
            bounds = bounds[:-1]
        pw, ph = 5, 4
        for b in bounds:
            anchor = (7, b - 2)  # pattern rows b - 2 .. b + 1: across the boundary
            cells = cut(board, *anchor, pw, ph, torus)
            care = np.ones_like(cells)
            whole = F.find(board, cells, care, torus)
            assert list((anchor[0], anchor[1] % H)) in whole.tolist()
            wins = [(0, 0, W, H)] + ([(200, H - 3, 100, 10)] if torus else [(3, 1, 60, 7)])
            for win in wins:
                want = F.find(board, cells, care, torus, *win)
                got = group.find(cells, x=win[0], y=win[1], w=win[2], h=win[3])
                assert got["count"] == len(want)
                np.testing.assert_array_equal(got["matches"], want, err_msg=str((b, win)))
            # the C call of each shard alone: the anchors whose pattern lies in the shard's rows
            examined = set()
            total = 0
            for s in shards:
                rows = F.examined_rows(H, s.row0, s.rows, ph, torus)
                examined |= set(rows)
                res = N.GolFindResult()
                xy = np.zeros((W * H, 2), dtype=np.int64)
                assert raw(s, (0, 0, W, H), cells, care, xy, len(xy), res) == N.GOL_OK
                mine = [p for p in whole.tolist() if p[1] in rows]
                assert res.count == res.returned == len(mine) and res.rows_searched == len(rows)
                assert xy[:res.returned].tolist() == mine
                total += res.count
            straddling = sum(1 for p in whole.tolist() if p[1] not in examined)
            assert straddling > 0 and total == len(whole) - straddling
        # truncated like the single call
        one = np.ones((1, 1), dtype=np.uint8)
        got = group.find(one, max_matches=7)
        assert got["count"] == int(board.sum()) and got["matches"].shape == (7, 2)
        assert group.epoch == EPOCH
    finally:
        group.close()
        for s in shards:
            s.close()


def test_a_window_that_misses_the_shard(gpu):
    from gameoflife import _native as N
    from gameoflife.engine import GolEngine
    W, H = 256, 192
    one = np.ones((1, 1), dtype=np.uint8)
    with GolEngine(W, H, row0=70, rows=61) as e:
        e.seed(3)
        for wy, wh in ((0, 70), (131, 61), (131, 131)):  # above it, below it, over the y seam
            res = N.GolFindResult(9, 9, 9)
            xy = np.full((4, 2), 7, dtype=np.int64)
            assert raw(e, (0, wy, W, wh), one, one, xy, 4, res) == N.GOL_OK
            assert (res.count, res.returned, res.rows_searched) == (0, 0, 0) and (xy == 7).all()
        res = N.GolFindResult()
        assert raw(e, (0, 60, W, 20), one, one, None, 0, res) == N.GOL_OK  # rows 70 .. 79 of the window are its own
        assert res.rows_searched == 10 and res.count > 0


# ---- ordering and purity ----
def test_ordered_after_asynchronous_steps_and_pure(gpu):
    from gameoflife import codec
    from gameoflife.engine import GolEngine
    W, H, seed = 256, 64, 21
    start = O.seed_packed(W, H, seed)
    at3, _ = O.run_packed(start, W, 3)
    at7, want_hashes = O.run_packed(at3, W, 4)
    with GolEngine(W, H) as e:
        e.seed(seed)
        e.step(3)  # not waited for
        b3 = codec.unpack(at3, W)
        cells = cut(b3, 250, 62, 9, 4, True)
        check(e, b3, True, cells, np.ones_like(cells), (0, 0, W, H), "after-step")
        assert e.epoch == 3 and e.hash() == O.hash_packed(at3, W)
        np.testing.assert_array_equal(e.step(4, hashes=True), want_hashes)
        buf = e.host_buffer()
        e.snapshot_async(buf)
        b7 = codec.unpack(at7, W)
        cells = cut(b7, 31, 5, 3, 3, True)
        check(e, b7, True, cells, np.ones_like(cells), (20, 60, 100, 30), "snapshot-in-flight")
        assert e.snapshot_wait() == 7
        np.testing.assert_array_equal(buf, at7)
        assert e.epoch == 7 and e.hash() == O.hash_packed(at7, W)


# ---- refusals ----
def test_refusals(gpu):
    from gameoflife import _native as N
    from gameoflife.engine import GolEngine
    xy = np.full((8, 2), 7, dtype=np.int64)
    res = N.GolFindResult(11, 12, 13)
    box = np.ones((3, 3), dtype=np.uint8)

    def refused(e, rc):
        assert rc == N.GOL_EINVAL
        assert N.lib.gol_last_error(e._h if e is not None else None)
        assert N.take_hip_error() == 0
        assert (xy == 7).all() and (res.count, res.returned, res.rows_searched) == (11, 12, 13)

    W, H = 256, 16
    with GolEngine(W, H) as e:
        e.seed(3)
        e.step(3)
        before = e.hash()
        win = (0, 0, W, H)
        refused(None, raw(None, win, box, box, xy, 8, res, null_ctx=True))
        refused(e, raw(e, win, box, box, xy, 8, res, null_pattern=True))
        refused(e, raw(e, win, box, box, xy, 8, res, null_res=True))
        refused(e, raw(e, win, box, box, xy, -1, res))
        refused(e, raw(e, win, box, box, None, 8, res))
        for pw, ph in ((0, 3), (3, 0), (65, 3), (3, 65), (-1, 3), (3, H + 1)):
            refused(e, raw(e, win, np.ones((3, 3), dtype=np.uint8), None, xy, 8, res, pitch=3, pw=pw, ph=ph))
        wide = np.ones((3, 40), dtype=np.uint8)
        refused(e, raw(e, win, wide, wide, xy, 8, res, pitch=1))  # 40 columns need two words
        refused(e, raw(e, win, box, np.zeros_like(box), xy, 8, res))  # no cared cell
        dirty = np.zeros((1, 40), dtype=np.uint8)
        dirty[0, 35:] = 1
        refused(e, raw(e, win, dirty, dirty, xy, 8, res, pw=35))  # ... none at k < pw
        for x0, y0, w, h in [(0, 0, 0, 1), (0, 0, 1, 0), (W, 0, 1, 1), (0, H, 1, 1), (-1, 0, 1, 1), (0, 0, W + 1, 1),
                             (0, 0, 1, H + 1)]:
            refused(e, raw(e, (x0, y0, w, h), box, box, xy, 8, res))
        assert e.hash() == before and e.epoch == 3
    with GolEngine(32, 16) as e:  # a pattern wider than the board
        e.seed(3)
        wide = np.ones((1, 33), dtype=np.uint8)
        refused(e, raw(e, (0, 0, 32, 16), wide, wide, xy, 8, res))
    with GolEngine(70, 9, topology="ref-clipped") as e:
        e.seed(3)
        for x0, y0, w, h in [(60, 0, 11, 1), (0, 8, 1, 2), (69, 8, 2, 2)]:  # a clipped board does not wrap
            refused(e, raw(e, (x0, y0, w, h), box, box, xy, 8, res))
        ok = N.GolFindResult()
        assert raw(e, (60, 8, 10, 1), box, box, xy.copy(), 8, ok) == N.GOL_OK  # flush with the corner
