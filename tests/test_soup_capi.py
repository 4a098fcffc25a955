"""CPU: the soups of a batch without a device (gol_soup_batch*; DESIGN.md
section 5l): the three symbols, their declarations and the binding's
prototypes, gol_soup_spec's layout, what gol_soup_batch_check refuses and the
edge of each refusal, and gol_soup_batch_rows -- the reproducer -- against the
cell-level model of tests/soup_model.py on the shapes the GPU test uses, with
the symmetries checked by numpy flips, the density by a 6 sigma bound, and one
known answer pinned in tests/golden/soup_known.json.  tests/soup_probe.cpp runs
csrc/gol_soup.h alone under the address and undefined-behaviour sanitizers."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import soup_model as SM
from gameoflife import _native as N
from gameoflife import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOUP = ("gol_soup_batch_check", "gol_soup_batch", "gol_soup_batch_rows")
_P = ctypes.POINTER
CTYPES = {"gol_batch*": ctypes.c_void_p, "constgol_batch_config*": _P(N.GolBatchConfig),
          "constgol_soup_spec*": _P(N.GolSoupSpec), "int64_t": ctypes.c_int64, "uint64_t*": _P(ctypes.c_uint64),
          "size_t": ctypes.c_size_t}
INDEX0 = 7


def _declaration(name):
    """Parameter types of `name` as include/gol.h declares it."""
    text = open(N.HEADER_PATH).read()
    m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, text, re.M)
    assert m, f"include/gol.h does not declare int {name}(...)"
    return ["".join(p.replace("*", "* ").split()[:-1]) for p in m.group(1).split(",")]


def _cfg(boards=3, width=64, height=64, topology=N.GOL_TORUS, vis=(0, 0)):
    c = N.GolBatchConfig()
    c.boards, c.width, c.height, c.topology = boards, width, height, topology
    c.birth_mask, c.survive_mask = 0x008, 0x00C
    c.vis_width, c.vis_height = vis
    return c


def _spec(x=0, y=0, w=64, h=64, density=128, symmetry="C1", seed=SM.SEED, index0=0):
    s = N.GolSoupSpec()
    s.seed, s.index0 = seed, index0
    s.x, s.y, s.w, s.h, s.density = x, y, w, h, density
    s.symmetry = N.SOUP_SYMMETRIES[symmetry] if isinstance(symmetry, str) else symmetry
    return s


def _check(cfg, spec, first=0, count=None):
    count = cfg.boards if count is None else count
    return N.lib.gol_soup_batch_check(ctypes.byref(cfg), ctypes.byref(spec) if spec is not None else None, first, count)


def _error():
    return N.lib.gol_batch_last_error(None).decode()


def _rows(shape, case, index0=INDEX0, first=0, count=None):
    """gol_soup_batch_rows for boards first .. first + count - 1 of a batch of the shape."""
    W, H, topo, vis, n = shape
    win, density, sym = case
    count = n - first if count is None else count
    cfg = _cfg(n, W, H, {"torus": N.GOL_TORUS, "ref-clipped": N.GOL_REF_CLIPPED}[topo], vis or (0, 0))
    x, y, w, h = win or (0, 0, W, H)
    out = np.zeros((count, H), dtype=np.uint64)
    rc = N.lib.gol_soup_batch_rows(ctypes.byref(cfg), ctypes.byref(_spec(x, y, w, h, density, sym, index0=index0)),
                                   first, count, out.ctypes.data_as(N._u64p), out.size)
    assert rc == N.GOL_OK, _error()
    return out


def test_declared_exported_and_bound():
    syms = N.header_symbols()
    for name in SOUP:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name
    assert sorted(s for s in syms if s.startswith("gol_soup_batch")) == sorted(SOUP)
    assert sorted(s for s in N._SIGNATURES if s.startswith("gol_soup")) == sorted(SOUP)


def test_prototypes_match_header():
    for name in SOUP:
        res, args = N._SIGNATURES[name]
        assert res is ctypes.c_int and args == [CTYPES[t] for t in _declaration(name)], name
        fn = getattr(N.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _declaration("gol_soup_batch_check") == ["constgol_batch_config*", "constgol_soup_spec*", "int64_t", "int64_t"]
    assert _declaration("gol_soup_batch") == ["gol_batch*", "constgol_soup_spec*", "int64_t", "int64_t"]
    assert _declaration("gol_soup_batch_rows") == ["constgol_batch_config*", "constgol_soup_spec*", "int64_t",
                                                   "int64_t", "uint64_t*", "size_t"]
    assert N.lib.gol_abi_version() == 2


def test_spec_layout_and_constants_match_header(tmp_path):
    fields = [f for f, _ in N.GolSoupSpec._fields_]
    names = list(batch.SOUP_SYMMETRIES)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gol.h"\nint main(void){\n'
                   'printf("%zu ", sizeof(gol_soup_spec));\n'
                   + "".join(f'printf("%zu ", offsetof(gol_soup_spec, {f}));\n' for f in fields)
                   + "".join(f'printf("%d ", GOL_SOUP_{n});\n' for n in names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(N.GolSoupSpec) == 40
    assert got[1:1 + len(fields)] == [getattr(N.GolSoupSpec, f).offset for f in fields]
    assert got[1 + len(fields):] == [N.SOUP_SYMMETRIES[n] for n in names] == list(range(9))
    assert names == list(SM.SYMMETRIES)


# each refusal with the message it gives, next to the nearest arguments that are accepted
REFUSALS = [
    ("w 0", dict(w=0), "w and h must be at least 1", dict(w=1)),
    ("h 0", dict(h=0), "w and h must be at least 1", dict(h=1)),
    ("w -3", dict(w=-3), "w and h must be at least 1", dict(w=1)),
    ("x -1", dict(x=-1, w=8), "inside the stored board", dict(x=0, w=8)),
    ("y -1", dict(y=-1, h=8), "inside the stored board", dict(y=0, h=8)),
    ("x + w = width + 1", dict(x=25, w=16), "inside the stored board", dict(x=24, w=16)),
    ("y + h = height + 1", dict(y=15, h=16), "inside the stored board", dict(y=14, h=16)),
    ("x + w wraps int32", dict(x=2**31 - 1, w=2**31 - 1), "inside the stored board", dict(x=39, w=1)),
    ("density 0", dict(density=0), "density must be 1 .. 255", dict(density=1)),
    ("density 256", dict(density=256), "density must be 1 .. 255", dict(density=255)),
    ("symmetry -1", dict(symmetry=-1), "unknown symmetry", dict(symmetry=0)),
    ("symmetry 9", dict(symmetry=9), "unknown symmetry", dict(symmetry=8, w=30, h=30)),
] + [(f"{s} on 20 x 9", dict(w=20, h=9, symmetry=s), "needs a square window", dict(w=9, h=9, symmetry=s))
     for s in SM.SQUARE]


@pytest.mark.parametrize("what,bad,message,good", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_refuses_and_accepts_the_edge(what, bad, message, good):
    base = dict(x=0, y=0, w=40, h=30)  # on boards of 40 x 30
    cfg = _cfg(3, 40, 30)
    assert _check(cfg, _spec(**{**base, **bad})) == N.GOL_EINVAL, what
    assert message in _error() and "gol_soup_batch_check" in _error(), (what, _error())
    assert _check(cfg, _spec(**{**base, **good})) == N.GOL_OK, (what, _error())


def test_check_refuses_bad_ranges_and_nulls():
    cfg, spec = _cfg(3, 40, 30), _spec(w=40, h=30)
    for what, (first, count) in {"first -1": (-1, 1), "count 0": (0, 0), "count -1": (0, -1), "first = boards": (3, 1),
                                 "past the end": (1, 3), "count 2^62": (1, 1 << 62)}.items():
        assert _check(cfg, spec, first, count) == N.GOL_EINVAL, what
        assert "outside the batch" in _error(), (what, _error())
    for first, count in ((0, 3), (2, 1), (1, 2), (0, 1)):
        assert _check(cfg, spec, first, count) == N.GOL_OK, _error()
    assert _check(cfg, None) == N.GOL_EINVAL and "spec is null" in _error()
    assert N.lib.gol_soup_batch_check(None, ctypes.byref(spec), 0, 1) == N.GOL_EINVAL
    # the groups without a T or an R take any window
    for s in SM.ANY:
        assert _check(cfg, _spec(x=20, y=21, w=20, h=9, symmetry=s)) == N.GOL_OK, s
    # a geometry gol_batch_create refuses is refused here alike
    assert _check(_cfg(3, 65, 30), _spec(w=40, h=30)) == N.GOL_EINVAL
    assert _check(_cfg(3, 2, 30), _spec(w=2, h=30)) == N.GOL_EINVAL
    assert N.lib.gol_soup_batch(None, ctypes.byref(spec), 0, 1) == N.GOL_EINVAL and "null handle" in _error()


def test_rows_refuses_and_writes_nothing():
    cfg, spec = _cfg(3, 40, 30), _spec(w=40, h=30)
    out = np.full((3, 30), 0xDEAD, dtype=np.uint64)
    ptr = out.ctypes.data_as(N._u64p)
    assert N.lib.gol_soup_batch_rows(ctypes.byref(cfg), ctypes.byref(spec), 0, 3, None, 90) == N.GOL_EINVAL
    assert "rows_out is null" in _error()
    assert N.lib.gol_soup_batch_rows(ctypes.byref(cfg), ctypes.byref(spec), 0, 3, ptr, 89) == N.GOL_EINVAL
    assert "holds 89 entries" in _error() and "need 90" in _error(), _error()
    for bad in (dict(w=0), dict(density=0), dict(symmetry=9), dict(w=41), dict(w=20, h=9, symmetry="D8")):
        s = _spec(**{**dict(w=40, h=30), **bad})
        assert N.lib.gol_soup_batch_rows(ctypes.byref(cfg), ctypes.byref(s), 0, 3, ptr, 90) == N.GOL_EINVAL, bad
    assert N.lib.gol_soup_batch_rows(ctypes.byref(cfg), ctypes.byref(spec), 1, 3, ptr, 90) == N.GOL_EINVAL
    assert N.lib.gol_soup_batch_rows(ctypes.byref(cfg), None, 0, 3, ptr, 90) == N.GOL_EINVAL
    assert N.lib.gol_soup_batch_rows(None, ctypes.byref(spec), 0, 3, ptr, 90) == N.GOL_EINVAL
    assert (out == 0xDEAD).all()
    assert N.lib.gol_soup_batch_rows(ctypes.byref(cfg), ctypes.byref(spec), 0, 3, ptr, 90) == N.GOL_OK
    assert not (out == 0xDEAD).any()


@pytest.mark.parametrize("sc", SM.CASES, ids=SM.case_id)
def test_rows_equal_the_model_and_have_the_symmetry(sc):
    shape, case = sc
    W, H, _, _, n = shape
    win, density, sym = case
    got = _rows(shape, case)
    assert np.array_equal(got, SM.boards(W, H, SM.SEED, INDEX0, n, win, density, sym))
    window = win or (0, 0, W, H)
    assert SM.invariant(SM.window_cells(got, window), sym)
    # nothing lives outside the window, and the boards differ from each other
    x, y, w, h = window
    inside = np.zeros(H, dtype=np.uint64)
    inside[y:y + h] = np.uint64(((1 << w) - 1) << x)
    assert not (got & ~inside).any()
    if density == 128 and SM.distinct_expected(sym, w, h, n):
        assert len({r.tobytes() for r in got}) == n
    # a part of the batch is that part of the whole batch
    if n > 4:
        assert np.array_equal(_rows(shape, case, first=3, count=2), got[3:5])


def test_the_flips_can_fail():
    """SM.invariant is no tautology: a C1 soup has none of the symmetries."""
    shape = (64, 64, "torus", None, 5)
    got = _rows(shape, ((24, 24, 16, 16), 128, "C1"))
    for s in SM.SYMMETRIES[1:]:
        assert not SM.invariant(SM.window_cells(got, (24, 24, 16, 16)), s), s


@pytest.mark.parametrize("density", [1, 96, 128, 255])
def test_density_within_six_sigma(density):
    shape = (64, 64, "torus", None, 256)
    got = _rows(shape, (None, density, "C1"), index0=1000)
    cells, p = 256 * 64 * 64, density / 256
    live = int(batch.unpack_rows(got, 64).sum())
    assert abs(live - cells * p) <= 6 * math.sqrt(cells * p * (1 - p)), (live, cells * p)


def test_consecutive_soups_differ_and_the_index_wraps():
    shape = (64, 64, "torus", None, 4)
    case = ((24, 24, 16, 16), 128, "D8")
    a = _rows(shape, case, index0=0)
    assert all(not np.array_equal(a[i], a[i + 1]) for i in range(3))
    assert np.array_equal(_rows(shape, case, index0=1)[:3], a[1:])
    # index0 = 2^64 - 2: boards 0 .. 3 hold soups 2^64 - 2, 2^64 - 1, 0 and 1
    wrapped = _rows(shape, case, index0=2**64 - 2)
    assert np.array_equal(wrapped[2:], a[:2])
    assert np.array_equal(wrapped, SM.boards(64, 64, SM.SEED, 2**64 - 2, 4, *case))
    assert not np.array_equal(wrapped[0], wrapped[1]) and not np.array_equal(wrapped[1], wrapped[2])


def test_known_answer():
    """Pinned when the definition was written (from tests/soup_model.py): it cannot drift silently."""
    known = json.load(open(os.path.join(ROOT, "tests", "golden", "soup_known.json")))
    assert (known["seed"], known["soup"], known["width"], known["height"], known["density"]) == (0x5EED, 0, 8, 8, 128)
    for sym in ("C1", "D8"):
        want = np.array([int(r, 16) for r in known[sym]], dtype=np.uint64)
        got = batch.soup_rows(8, 8, 0x5EED, 0, density=128, symmetry=sym)
        assert got.shape == (1, 8) and np.array_equal(got[0], want), sym
        assert np.array_equal(SM.board(8, 8, 0x5EED, 0, None, 128, sym), want), sym
    assert SM.mix(0x5EED, 0) == int(known["mix_seed_0"], 16)


def test_python_soup_rows():
    W, H = 40, 20
    win = (31, 11, 9, 9)
    got = batch.soup_rows(W, H, SM.SEED, [9, 7, 2**64 - 1], window=win, density=0.5, symmetry="C4")
    assert got.dtype == np.uint64 and got.shape == (3, H)
    for row, n in zip(got, (9, 7, 2**64 - 1)):
        assert np.array_equal(row, SM.board(W, H, SM.SEED, n, win, 128, "C4"))
    # a float is rounded to n / 256, an int is n
    assert np.array_equal(batch.soup_rows(W, H, 1, 0, density=96 / 256), batch.soup_rows(W, H, 1, 0, density=96))
    with pytest.raises(ValueError):
        batch.soup_rows(W, H, 1, 0, symmetry="D3")
    with pytest.raises(N.GolError) as e:
        batch.soup_rows(W, H, 1, 0, density=1.0)
    assert "density must be 1 .. 255" in str(e.value)
    assert callable(batch.GolBatch.soup)


def test_probe_under_the_sanitizers(tmp_path):
    """csrc/gol_soup.h alone in a program of its own, with -fsanitize=address,undefined: the generator called
    three ways, and against the kernel's plan (domain masks, then an image per step) carried out on the host."""
    exe = tmp_path / "soup_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "soup_probe.cpp"), "-o", str(exe)],
                   check=True)
    args = []
    for (W, H, _, _, n), (win, density, sym) in SM.CASES:
        x, y, w, h = win or (0, 0, W, H)
        args += [W, H, min(n, 9), x, y, w, h, density, N.SOUP_SYMMETRIES[sym]]
    for index0 in (INDEX0, 2**64 - 2):
        p = subprocess.run([str(exe), hex(SM.SEED), str(index0)] + [str(a) for a in args], capture_output=True,
                           text=True)
        assert p.returncode == 0 and p.stdout.strip() == f"ok {len(SM.CASES)}", (p.stdout, p.stderr)
