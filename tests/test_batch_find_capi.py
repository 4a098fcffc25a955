"""CPU: the C ABI of the pattern search on a batch (gol_find_batch*; DESIGN.md
section 5h).  No device is touched: the symbols, their declarations and the
binding's prototypes, the struct layout, and what gol_find_batch_check accepts
and refuses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from gameoflife import _native as N
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIND = ("gol_find_batch_check", "gol_find_batch", "gol_find_batch_set_cut", "gol_find_batch_stats")
_P = ctypes.POINTER
CTYPES = {"gol_batch*": ctypes.c_void_p, "constgol_batch_config*": _P(N.GolBatchConfig),
          "constgol_batch_pattern*": _P(N.GolBatchPattern), "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
          "size_t": ctypes.c_size_t, "uint32_t*": _P(ctypes.c_uint32), "uint64_t*": _P(ctypes.c_uint64)}


def _declaration(name):
    """Parameter types of `name` as include/gol.h declares it."""
    text = open(N.HEADER_PATH).read()
    m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, text, re.M)
    assert m, f"include/gol.h does not declare int {name}(...)"
    return ["".join(p.replace("*", "* ").split()[:-1]) for p in m.group(1).split(",")]


def _cfg(width=8, height=8, topology=N.GOL_TORUS, boards=3, vis=(0, 0)):
    c = N.GolBatchConfig()
    c.boards, c.width, c.height, c.topology = boards, width, height, topology
    c.birth_mask, c.survive_mask = O.LIFE
    c.vis_width, c.vis_height = vis
    return c


def _patterns(*specs):
    """A gol_batch_pattern array of (pw, ph, cells rows or None, care rows or None); the arrays kept alive with it."""
    table, keep = (N.GolBatchPattern * max(len(specs), 1))(), []
    for t, (pw, ph, cells, care) in zip(table, specs):
        t.pw, t.ph = pw, ph
        for field, rows in (("cells", cells), ("care", care)):
            if rows is not None:
                a = np.asarray(rows, dtype=np.uint64)
                keep.append(a)
                setattr(t, field, a.ctypes.data_as(N._u64p))
    return table, keep


def _check(cfg, specs, n=None):
    table, keep = _patterns(*specs)
    return N.lib.gol_find_batch_check(ctypes.byref(cfg), table, len(specs) if n is None else n)


def test_declared_exported_and_bound():
    syms = N.header_symbols()
    for name in FIND:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name
    assert sorted(s for s in syms if s.startswith("gol_find_batch")) == sorted(FIND)


def test_prototypes_match_header():
    for name in FIND:
        res, args = N._SIGNATURES[name]
        assert res is ctypes.c_int and args == [CTYPES[t] for t in _declaration(name)], name
        fn = getattr(N.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _declaration("gol_find_batch") == ["gol_batch*", "constgol_batch_pattern*", "int32_t", "uint32_t*", "size_t",
                                              "uint64_t*", "size_t"]
    assert _declaration("gol_find_batch_check") == ["constgol_batch_config*", "constgol_batch_pattern*", "int32_t"]


def test_pattern_struct_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gol.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(gol_batch_pattern),'
                   ' offsetof(gol_batch_pattern, pw), offsetof(gol_batch_pattern, ph),'
                   ' offsetof(gol_batch_pattern, cells), offsetof(gol_batch_pattern, care)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S = N.GolBatchPattern
    assert got == [ctypes.sizeof(S), S.pw.offset, S.ph.offset, S.cells.offset, S.care.offset]


def test_abi_version_stays_2_and_constants_match_header():
    assert N.lib.gol_abi_version() == 2 and N.GOL_ABI_VERSION == 2
    text = open(N.HEADER_PATH).read()
    assert f"npatterns outside 1 .. {N.GOL_FIND_BATCH_MAX_PATTERNS}" in text
    assert re.search(r"0 = the automatic value,\s*\*?\s*%d \(DESIGN.md section 5h" % N.GOL_FIND_BATCH_AUTO_CUT, text)


def test_check_accepts_the_legal_extremes():
    full = [2**64 - 1] * 64
    assert _check(_cfg(64, 64), [(64, 64, full, None)]) == N.GOL_OK            # pw = width = 64, ph = height
    assert _check(_cfg(64, 64, N.GOL_REF_CLIPPED, vis=(64, 63)), [(64, 64, full, full)]) == N.GOL_OK
    assert _check(_cfg(), [(1, 1, [1], None)]) == N.GOL_OK                       # a 1 x 1 pattern
    assert _check(_cfg(), [(3, 3, [0, 0, 0], [7, 7, 7])]) == N.GOL_OK            # an empty cared 3 x 3 box
    assert _check(_cfg(), [(3, 3, [0, 0, 0], None)]) == N.GOL_OK
    assert _check(_cfg(3, 3), [(3, 3, [5, 2, 5], [7, 5, 7])]) == N.GOL_OK        # a 3 x 3 torus
    assert _check(_cfg(), [(2, 2, [3, 3], [0, 1])]) == N.GOL_OK                  # one cared cell is enough
    assert _check(_cfg(), [(1, 1, [1], None)] * 256) == N.GOL_OK
    # bits at k >= pw are ignored: a care mask with bits only there cares for nothing (below), cells there are fine
    assert _check(_cfg(), [(2, 1, [0xFF], None)]) == N.GOL_OK


@pytest.mark.parametrize("topology,vis", [(N.GOL_TORUS, (0, 0)), (N.GOL_REF_CLIPPED, (0, 0))])
def test_check_refuses_with_a_message(topology, vis):
    cfg = _cfg(8, 8, topology, vis=vis)
    ok = (2, 2, [3, 3], None)
    refusals = {
        "pw > width": ([ok, (9, 2, [3, 3], None)], None, b"pattern 1"),
        "ph > height": ([(2, 9, [3] * 9, None)], None, b"pattern 0"),
        "pw = 0": ([(0, 2, [3, 3], None)], None, b"pattern 0"),
        "npatterns 0": ([ok], 0, b"npatterns"),
        "npatterns 257": ([ok] * 257, None, b"npatterns"),
        "null cells": ([ok, ok, (2, 2, None, None)], None, b"pattern 2: cells is null"),
        "all-zero care": ([(2, 2, [3, 3], [0, 0])], None, b"cares for no cell"),
        "care beyond pw only": ([(2, 2, [3, 3], [4, 8])], None, b"cares for no cell"),
    }
    for what, (specs, n, word) in refusals.items():
        assert _check(cfg, specs, n) == N.GOL_EINVAL, what
        assert word in N.lib.gol_batch_last_error(None), (what, N.lib.gol_batch_last_error(None))
    table, keep = _patterns(ok)
    assert N.lib.gol_find_batch_check(None, table, 1) == N.GOL_EINVAL
    assert N.lib.gol_find_batch_check(ctypes.byref(cfg), None, 1) == N.GOL_EINVAL
    # a geometry gol_batch_create refuses is refused here alike
    assert N.lib.gol_find_batch_check(ctypes.byref(_cfg(65, 8, topology)), table, 1) == N.GOL_EINVAL


def test_null_handle_is_einval_and_writes_nothing():
    table, keep = _patterns((2, 2, [3, 3], None))
    counts = (ctypes.c_uint32 * 4)(*([9] * 4))
    planes = (ctypes.c_uint64 * 8)(*([7] * 8))
    assert N.lib.gol_find_batch(None, table, 1, counts, 4, planes, 8) == N.GOL_EINVAL
    assert N.lib.gol_find_batch(None, None, 0, None, 0, None, 0) == N.GOL_EINVAL
    assert N.lib.gol_find_batch_set_cut(None, 5) == N.GOL_EINVAL
    launches = ctypes.c_uint64(11)
    assert N.lib.gol_find_batch_stats(None, ctypes.byref(launches), None) == N.GOL_EINVAL
    assert N.lib.gol_batch_last_error(None)
    assert list(counts) == [9] * 4 and list(planes) == [7] * 8 and launches.value == 11


def test_python_wrapper_has_the_calls():
    from gameoflife import batch
    assert callable(batch.GolBatch.find) and callable(batch.match_positions)
    rows = np.array([[0, 0b101], [0b10, 0]], dtype=np.uint64)
    assert batch.match_positions(rows, 3).tolist() == [[0, 0, 1], [0, 2, 1], [1, 1, 0]]
