"""CPU: the pattern search without a device -- the brute-force model's own
self-checks (tests/find_model.py), patterns.as_search, the host matcher of
ShardGroup.find against the model, gol_find's header, signature and
null-context refusal, and the anchor-row arithmetic of csrc/gol_active.h
(anchor_rows, clip) through tests/find_probe.cpp, built with plain g++, against
a model of sets of rows."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import find_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")

GLIDER = [".O.", "..O", "OOO"]


# ---- the model on hand-made boards ---------------------------------------------

def test_model_finds_a_lone_glider_once():
    from gameoflife import patterns
    cells, care = patterns.as_search(GLIDER, border=1)
    board = np.zeros((16, 32), dtype=np.uint8)
    board[5:8, 9:12] = patterns.from_rows(GLIDER)
    for torus in (True, False):
        np.testing.assert_array_equal(F.find(board, cells, care, torus), [[8, 4]])
    # without the border the bare 3 x 3 box matches at the glider only, too
    cells, care = patterns.as_search(GLIDER)
    np.testing.assert_array_equal(F.find(board, cells, care, True), [[9, 5]])
    # a live cell next to it: the bordered search no longer matches, the bare one does
    board[4, 8] = 1
    cells, care = patterns.as_search(GLIDER, border=1)
    assert F.find(board, cells, care, True).shape == (0, 2)


def test_model_finds_overlapping_candidates():
    """OOO in a row of five live cells: three overlapping matches; with the
    window cut to two anchors, two."""
    board = np.zeros((4, 16), dtype=np.uint8)
    board[1, 3:8] = 1
    cells = np.ones((1, 3), dtype=np.uint8)
    care = np.ones_like(cells)
    np.testing.assert_array_equal(F.find(board, cells, care, True), [[3, 1], [4, 1], [5, 1]])
    np.testing.assert_array_equal(F.find(board, cells, care, True, 4, 0, 5, 2), [[4, 1], [5, 1]])


def test_model_wraps_a_torus_and_pads_a_clipped_board():
    board = np.zeros((4, 8), dtype=np.uint8)
    board[3, 7] = board[0, 0] = 1
    cells = np.array([[1, 0], [0, 1]], dtype=np.uint8)
    care = np.ones_like(cells)
    np.testing.assert_array_equal(F.find(board, cells, care, True), [[7, 3]])
    assert F.find(board, cells, care, False).shape == (0, 2)
    cells = np.array([[1, 0], [0, 0]], dtype=np.uint8)  # beyond the clipped board reads dead
    np.testing.assert_array_equal(F.find(board, cells, care, False), [[0, 0], [7, 3]])


# ---- patterns.as_search ----------------------------------------------------------

def test_as_search_forms():
    from gameoflife import patterns
    cells, care = patterns.as_search(GLIDER)
    np.testing.assert_array_equal(cells, patterns.from_rows(GLIDER))
    assert care.shape == (3, 3) and care.all() and cells.dtype == care.dtype == np.uint8
    cells, care = patterns.as_search(GLIDER, border=2)
    assert cells.shape == (7, 7) and care.all()
    np.testing.assert_array_equal(cells[2:5, 2:5], patterns.from_rows(GLIDER))
    assert cells.sum() == 5
    cells, care = patterns.as_search(["O?.", "?O?"])
    np.testing.assert_array_equal(care, [[1, 0, 1], [0, 1, 0]])
    np.testing.assert_array_equal(cells, [[1, 0, 0], [0, 1, 0]])
    mask = np.array([[1, 1, 0], [0, 0, 0], [1, 0, 1]])
    cells, care = patterns.as_search(GLIDER, care=mask, border=1)
    np.testing.assert_array_equal(care[1:4, 1:4], mask)
    assert care[0].all() and care[-1].all() and care[:, 0].all() and care[:, -1].all()
    np.testing.assert_array_equal(cells[1:4, 1:4], patterns.from_rows(GLIDER) & mask)  # uncared cells read dead
    cells, care = patterns.as_search(np.zeros((3, 3), dtype=np.uint8))  # no live cell: legal
    assert not cells.any() and care.all()
    cells, care = patterns.as_search("bo$2bo$3o!")  # RLE
    np.testing.assert_array_equal(cells, patterns.from_rows(GLIDER))
    assert patterns.as_search(np.ones((64, 64), dtype=np.uint8))[0].shape == (64, 64)
    assert patterns.from_rows(GLIDER).shape == (3, 3)  # from_rows stays as it is ...
    with pytest.raises(ValueError):
        patterns.from_rows(["O?"])  # ... and knows no `?`


def test_as_search_refusals():
    from gameoflife import patterns
    with pytest.raises(ValueError):
        patterns.as_search(np.ones((65, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        patterns.as_search(np.ones((3, 65), dtype=np.uint8))
    with pytest.raises(ValueError):
        patterns.as_search(np.ones((64, 64), dtype=np.uint8), border=1)
    with pytest.raises(ValueError):
        patterns.as_search(GLIDER, care=np.ones((3, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        patterns.as_search(GLIDER, care=np.zeros((3, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        patterns.as_search(["??", "??"])
    with pytest.raises(ValueError):
        patterns.as_search(GLIDER, border=-1)
    assert patterns.as_search(["??", "??"], border=1)[1].sum() == 12  # the border's cells are cared for


# ---- the host matcher of ShardGroup.find -------------------------------------------

def test_host_matcher_agrees_with_the_model_on_random_bands():
    from gameoflife import patterns
    rng = np.random.default_rng(2024)
    nonempty = 0
    for case in range(60):
        ph, pw = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        bh, bw = int(rng.integers(ph, ph + 8)), int(rng.integers(pw, pw + 40))
        band = (rng.random((bh, bw)) < (0.5 if case % 2 else 0.15)).astype(np.uint8)
        care = (rng.random((ph, pw)) < 0.6).astype(np.uint8)
        care[rng.integers(ph), rng.integers(pw)] = 1
        ay, ax = int(rng.integers(0, bh - ph + 1)), int(rng.integers(0, bw - pw + 1))
        cells = band[ay:ay + ph, ax:ax + pw] & care  # cut from the band: at least one match
        got = patterns.match_band(band, cells, care)
        assert got.shape == (bh - ph + 1, bw - pw + 1) and got.dtype == bool
        # the model on the band as a clipped board, its anchors cut to those whose pattern fits
        want = F.match_map(band, cells, care, torus=False)[:bh - ph + 1, :bw - pw + 1]
        np.testing.assert_array_equal(got, want, err_msg=str(case))
        assert got[ay, ax]
        nonempty += int(got.sum() > 1)
    assert nonempty > 5
    assert patterns.match_band(np.zeros((2, 9), dtype=np.uint8), np.zeros((3, 3), dtype=np.uint8),
                               np.ones((3, 3), dtype=np.uint8)).size == 0


# ---- the C ABI, without a device -----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from gameoflife import _native as N
    return N


def test_header_and_signature(lib):
    assert "gol_find" in lib.header_symbols()
    assert hasattr(lib.lib, "gol_find") and "gol_find" in lib._SIGNATURES
    assert [f for f, _ in lib.GolFindResult._fields_] == ["count", "returned", "rows_searched"]
    assert ctypes.sizeof(lib.GolFindResult) == 24
    assert lib.lib.gol_abi_version() == 2 == lib.GOL_ABI_VERSION


def test_null_context_is_refused_without_a_device(lib):
    pat = np.ones((1, 1), dtype=np.uint32)
    xy = np.full((4, 2), 7, dtype=np.int64)
    res = lib.GolFindResult(11, 12, 13)
    rc = lib.lib.gol_find(None, 0, 0, 1, 1, pat.ctypes.data_as(lib._u32p), None, 1, 1, 1,
                          xy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 4, ctypes.byref(res))
    assert rc == lib.GOL_EINVAL
    assert lib.lib.gol_last_error(None)
    assert (xy == 7).all() and (res.count, res.returned, res.rows_searched) == (11, 12, 13)


# ---- anchor rows (csrc/gol_active.h) ----------------------------------------------------

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("find") / "find_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "find_probe.cpp"), "-o", exe], check=True)

    def run(lines):
        p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = [[int(x) for x in l.split()] for l in p.stdout.splitlines()]
        assert len(out) == len(lines)
        return [list(zip(flat[::2], flat[1::2])) for flat in out]
    return run


def fmt(runs):
    return f"{len(runs)} " + " ".join(f"{lo} {hi}" for lo, hi in runs)


def rowset(runs):
    return set(itertools.chain.from_iterable(range(lo, hi) for lo, hi in runs))


def tidy(runs, rows):
    """Sorted, disjoint, not even touching, inside [0, rows)."""
    prev = -1
    for lo, hi in runs:
        assert 0 <= lo < hi <= rows and lo > prev, (runs, rows)
        prev = hi


def run_lists(rows):
    """Run lists as the live-row lists keep them (sorted, disjoint): at row 0,
    ending at `rows`, both (the seam), in the middle, adjacent blocks, all."""
    cases = [[], [(0, 1)], [(rows - 1, rows)], [(0, 1), (rows - 1, rows)], [(0, rows)], [(rows // 2, rows // 2 + 1)]]
    if rows >= 256:
        cases += [[(0, 64)], [(rows - 64, rows)], [(64, 128), (192, 256)], [(0, 64), (128, 192), (rows - 64, rows)],
                  [(64, 128), (130, 140)]]
    return cases


def test_anchor_rows_are_the_rows_with_a_pattern_row_in_a_run(probe):
    keys = [(rows, ph, wrap, runs) for rows in (3, 8, 64, 65, 256, 1024) for ph in (1, 2, 5, 64)
            for wrap in (0, 1) for runs in run_lists(rows)]
    got = probe([f"anchors {rows} {ph} {wrap} {fmt(runs)}" for rows, ph, wrap, runs in keys])
    assert len(keys) > 300
    for (rows, ph, wrap, runs), out in zip(keys, got):
        tidy(out, rows)
        live = rowset(runs)
        want = set()
        for a in range(rows):
            for i in range(ph):
                r = a + i
                if wrap:
                    r %= rows
                if r in live:  # on a clipped board rows past the end are in no run
                    want.add(a)
        assert rowset(out) == want, (rows, ph, wrap, runs, out)


def test_anchor_rows_at_the_seam_at_the_end_and_for_one_row(probe):
    torus0, clipped0, end, one, issue = probe([
        "anchors 1024 5 1 1 0 64",       # a run at row 0 of a torus: wraps and splits at the seam
        "anchors 1024 5 0 1 0 64",       # ... of a clipped board: clamps
        "anchors 1024 5 1 1 960 1024",   # a run ending at `rows`
        "anchors 1024 1 1 2 0 64 512 576",  # ph = 1: the runs themselves
        "anchors 1024 5 1 3 0 64 512 576 960 1024"])  # a glider at y = 512 and one across the seam
    assert torus0 == [(0, 64), (1020, 1024)]
    assert clipped0 == [(0, 64)]
    assert end == [(956, 1024)]
    assert one == [(0, 64), (512, 576)]
    assert issue == [(0, 64), (508, 576), (956, 1024)] and 511 in rowset(issue)


def test_clip_keeps_the_rows_inside(probe):
    lists = [r for rows in (8, 256, 1024) for r in run_lists(rows)]
    keys = [(lo, hi, runs) for runs in lists for lo, hi in ((0, 1024), (0, 1), (60, 70), (64, 128), (100, 100), (500, 2000))]
    got = probe([f"clip {lo} {hi} {fmt(runs)}" for lo, hi, runs in keys])
    for (lo, hi, runs), out in zip(keys, got):
        assert rowset(out) == rowset(runs) & set(range(lo, hi)), (lo, hi, runs, out)
        assert all(a < b for a, b in out) and all(x[1] <= y[0] for x, y in zip(out, out[1:]))
