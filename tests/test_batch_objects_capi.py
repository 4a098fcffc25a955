"""CPU: the C ABI of the objects of a batch's boards (gol_objects_batch*;
DESIGN.md section 5i).  No device is touched: the symbols, their declarations
and the binding's prototypes, the record's layout in C, ctypes and numpy, and
what gol_objects_batch_check accepts and refuses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from gameoflife import _native as N
from gameoflife import batch
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS = ("gol_objects_batch_check", "gol_objects_batch", "gol_objects_batch_stats")
_P = ctypes.POINTER
CTYPES = {"gol_batch*": ctypes.c_void_p, "constgol_batch_config*": _P(N.GolBatchConfig),
          "gol_batch_object*": _P(N.GolBatchObject), "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
          "size_t": ctypes.c_size_t, "uint32_t*": _P(ctypes.c_uint32), "uint64_t*": _P(ctypes.c_uint64)}
FIELDS = ("hash", "x", "y", "w", "h", "population", "reserved")


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


def _check(cfg, first=0, count=1, reach=1, max_objects=64):
    return N.lib.gol_objects_batch_check(ctypes.byref(cfg), first, count, reach, max_objects)


def test_declared_exported_and_bound():
    syms = N.header_symbols()
    for name in OBJECTS:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name
    assert sorted(s for s in syms if s.startswith("gol_objects_batch")) == sorted(OBJECTS)


def test_prototypes_match_header():
    for name in OBJECTS:
        res, args = N._SIGNATURES[name]
        assert res is ctypes.c_int and args == [CTYPES[t] for t in _declaration(name)], name
        fn = getattr(N.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _declaration("gol_objects_batch") == ["gol_batch*", "int64_t", "int64_t", "int32_t", "int32_t", "uint32_t*",
                                                 "size_t", "gol_batch_object*", "size_t"]
    assert _declaration("gol_objects_batch_check") == ["constgol_batch_config*", "int64_t", "int64_t", "int32_t",
                                                       "int32_t"]
    assert _declaration("gol_objects_batch_stats") == ["gol_batch*", "uint64_t*", "uint64_t*", "uint64_t*"]


def test_record_layout_is_the_same_in_c_ctypes_and_numpy(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gol.h"\n'
                   'int main(void){printf("%zu", sizeof(gol_batch_object));\n'
                   + "".join(f'printf(" %zu", offsetof(gol_batch_object, {f}));\n' for f in FIELDS)
                   + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S, D = N.GolBatchObject, batch.OBJECT_DTYPE
    assert got[0] == 16
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
    assert got == [D.itemsize] + [D.fields[f][1] for f in FIELDS]
    assert [f for f, _ in S._fields_] == list(FIELDS) == list(D.names)
    assert [ctypes.sizeof(t) for _, t in S._fields_] == [D.fields[f][0].itemsize for f in FIELDS]


def test_abi_version_stays_2_and_the_limit_matches_the_header():
    assert N.lib.gol_abi_version() == 2 and N.GOL_ABI_VERSION == 2
    assert f"max_objects outside\n * 1 .. {N.GOL_OBJECTS_BATCH_MAX}" in open(N.HEADER_PATH).read()


def test_check_accepts_the_legal_extremes():
    assert _check(_cfg()) == N.GOL_OK
    assert _check(_cfg(), 0, 3, 2, 1024) == N.GOL_OK            # every board, reach 2, the most records
    assert _check(_cfg(), 2, 1, 1, 1) == N.GOL_OK               # the last board alone, one record
    assert _check(_cfg(64, 64, boards=1 << 22), (1 << 22) - 1, 1) == N.GOL_OK
    assert _check(_cfg(64, 64, N.GOL_REF_CLIPPED, vis=(64, 63)), 0, 3, 2, 128) == N.GOL_OK
    assert _check(_cfg(3, 3), 0, 3, 2, 9) == N.GOL_OK           # a 3 x 3 torus


@pytest.mark.parametrize("topology", [N.GOL_TORUS, N.GOL_REF_CLIPPED])
def test_check_refuses_with_a_message(topology):
    cfg = _cfg(8, 8, topology)
    refusals = {
        "reach 0": ((0, 3, 0, 64), b"reach must be 1 or 2"),
        "reach 3": ((0, 3, 3, 64), b"reach must be 1 or 2"),
        "reach -1": ((0, 3, -1, 64), b"reach must be 1 or 2"),
        "max_objects 0": ((0, 3, 1, 0), b"max_objects must be 1 .. 1024"),
        "max_objects 1025": ((0, 3, 1, 1025), b"max_objects must be 1 .. 1024"),
        "first -1": ((-1, 1, 1, 64), b"outside the batch"),
        "first = boards": ((3, 1, 1, 64), b"outside the batch"),
        "count 0": ((0, 0, 1, 64), b"outside the batch"),
        "count past the end": ((1, 3, 1, 64), b"outside the batch"),
        "count 2^62": ((1, 1 << 62, 1, 64), b"outside the batch"),
    }
    for what, (args, word) in refusals.items():
        assert _check(cfg, *args) == N.GOL_EINVAL, what
        assert word in N.lib.gol_batch_last_error(None), (what, N.lib.gol_batch_last_error(None))
    assert N.lib.gol_objects_batch_check(None, 0, 1, 1, 64) == N.GOL_EINVAL
    # a geometry gol_batch_create refuses is refused here alike
    assert _check(_cfg(65, 8, topology)) == N.GOL_EINVAL
    assert _check(_cfg(2, 8, N.GOL_TORUS)) == N.GOL_EINVAL


def test_null_handle_is_einval_and_writes_nothing():
    counts = (ctypes.c_uint32 * 4)(*([9] * 4))
    objs = np.full(8, 0x77, dtype=np.uint8).repeat(16).view(batch.OBJECT_DTYPE)
    before = objs.tobytes()
    assert N.lib.gol_objects_batch(None, 0, 4, 1, 2, counts, 4, objs.ctypes.data_as(_P(N.GolBatchObject)),
                                   8) == N.GOL_EINVAL
    assert N.lib.gol_objects_batch(None, 0, 0, 0, 0, None, 0, None, 0) == N.GOL_EINVAL
    launches = ctypes.c_uint64(11)
    assert N.lib.gol_objects_batch_stats(None, ctypes.byref(launches), None, None) == N.GOL_EINVAL
    assert N.lib.gol_batch_last_error(None)
    assert list(counts) == [9] * 4 and objs.tobytes() == before and launches.value == 11


def test_python_wrapper_has_the_calls():
    assert callable(batch.GolBatch.objects) and callable(batch.GolBatch.objects_stats) and callable(batch.tally)
    counts = np.array([2, 3], dtype=np.uint32)
    objs = np.zeros((2, 2), dtype=batch.OBJECT_DTYPE)
    for rec, key in zip(objs.reshape(-1), [(5, 2, 2, 4), (6, 3, 1, 3), (5, 2, 2, 4), (9, 1, 1, 1)]):
        rec["hash"], rec["w"], rec["h"], rec["population"] = key
    table = {(5, 2, 2, 4): "block", (6, 3, 1, 3): "blinker", (6, 1, 3, 3): "blinker"}
    # board 1 has three objects and room for two: only the records present count
    assert batch.tally(counts, objs, table) == {"block": 2, "blinker": 1, None: 1}
