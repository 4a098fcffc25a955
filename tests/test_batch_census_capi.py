"""CPU: the C ABI of the census of a batch's objects (gol_census_batch*;
DESIGN.md section 5j).  No device is touched: the symbols, their declarations
and the binding's prototypes, the entry's layout in C, ctypes and numpy, what
gol_census_batch_check accepts and refuses, and the refusals of the pure
validator (csrc/gol_batch.h batch_census_args) that a call could reach only
after 2^24 others, through tests/census_probe.cpp built with plain g++."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gameoflife import _native as N
from gameoflife import batch
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = ("gol_census_batch_check", "gol_census_batch_begin", "gol_census_batch_add",
          "gol_census_batch_add_records", "gol_census_batch_read", "gol_census_batch_stats")
_P = ctypes.POINTER
CTYPES = {"gol_batch*": ctypes.c_void_p, "constgol_batch_config*": _P(N.GolBatchConfig),
          "constgol_batch_object*": _P(N.GolBatchObject), "gol_census_entry*": _P(N.GolCensusEntry),
          "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
          "size_t*": _P(ctypes.c_size_t), "uint32_t*": _P(ctypes.c_uint32), "uint64_t*": _P(ctypes.c_uint64)}
FIELDS = ("hash", "w", "h", "population", "first_call", "count", "first_board", "first_x", "first_y", "reserved")
DECLARED = {
    "gol_census_batch_check": ["constgol_batch_config*", "int32_t", "int32_t", "int64_t"],
    "gol_census_batch_begin": ["gol_batch*", "int64_t"],
    "gol_census_batch_add": ["gol_batch*", "int32_t", "int32_t", "uint32_t*"],
    "gol_census_batch_add_records": ["gol_batch*", "constgol_batch_object*", "size_t", "uint32_t", "uint32_t*"],
    "gol_census_batch_read": ["gol_batch*", "gol_census_entry*", "size_t", "size_t*"],
    "gol_census_batch_stats": ["gol_batch*"] + ["uint64_t*"] * 6,
}


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


def _check(cfg, reach=1, max_objects=128, max_keys=4096):
    return N.lib.gol_census_batch_check(ctypes.byref(cfg), reach, max_objects, max_keys)


def test_declared_exported_and_bound():
    syms = N.header_symbols()
    for name in CENSUS:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name
    assert sorted(s for s in syms if s.startswith("gol_census_batch")) == sorted(CENSUS)


def test_prototypes_match_header():
    for name in CENSUS:
        res, args = N._SIGNATURES[name]
        assert _declaration(name) == DECLARED[name], name
        assert res is ctypes.c_int and args == [CTYPES[t] for t in DECLARED[name]], name
        fn = getattr(N.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_entry_layout_is_the_same_in_c_ctypes_and_numpy(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gol.h"\n'
                   'int main(void){printf("%zu", sizeof(gol_census_entry));\n'
                   + "".join(f'printf(" %zu", offsetof(gol_census_entry, {f}));\n' for f in FIELDS)
                   + 'printf(" %d", GOL_CENSUS_BATCH_MAX_KEYS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got.pop() == N.GOL_CENSUS_BATCH_MAX_KEYS == 1 << 20
    S, D = N.GolCensusEntry, batch.CENSUS_DTYPE
    assert got[0] == 32 and got[1:] == [0, 8, 9, 10, 12, 16, 24, 28, 29, 30]
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
    assert got == [D.itemsize] + [D.fields[f][1] for f in FIELDS]
    assert [f for f, _ in S._fields_] == list(FIELDS) == list(D.names)
    assert [ctypes.sizeof(t) for _, t in S._fields_] == [D.fields[f][0].itemsize for f in FIELDS]


def test_abi_version_stays_2():
    assert N.lib.gol_abi_version() == 2 and N.GOL_ABI_VERSION == 2
    assert "#define GOL_ABI_VERSION 2\n" in open(N.HEADER_PATH).read()


def test_check_accepts_the_legal_extremes():
    assert _check(_cfg()) == N.GOL_OK
    assert _check(_cfg(), 1, 1, 1) == N.GOL_OK                      # one record per board, a table of two slots
    assert _check(_cfg(), 2, 1024, 1 << 20) == N.GOL_OK             # reach 2, the most records, the most keys
    assert _check(_cfg(64, 64, boards=1 << 22), 1, 1024, 1 << 20) == N.GOL_OK
    assert _check(_cfg(64, 64, N.GOL_REF_CLIPPED, vis=(64, 63)), 2, 128, 65536) == N.GOL_OK
    assert _check(_cfg(3, 3), 2, 9, 5) == N.GOL_OK                  # a 3 x 3 torus


@pytest.mark.parametrize("topology", [N.GOL_TORUS, N.GOL_REF_CLIPPED])
def test_check_refuses_with_a_message(topology):
    cfg = _cfg(8, 8, topology)
    refusals = {
        "reach 0": ((0, 128, 4096), b"reach must be 1 or 2"),
        "reach 3": ((3, 128, 4096), b"reach must be 1 or 2"),
        "reach -1": ((-1, 128, 4096), b"reach must be 1 or 2"),
        "max_objects 0": ((1, 0, 4096), b"max_objects must be 1 .. 1024"),
        "max_objects 1025": ((1, 1025, 4096), b"max_objects must be 1 .. 1024"),
        "max_keys 0": ((1, 128, 0), b"max_keys must be 1 .. 2^20"),
        "max_keys -1": ((1, 128, -1), b"max_keys must be 1 .. 2^20"),
        "max_keys 2^20 + 1": ((1, 128, (1 << 20) + 1), b"max_keys must be 1 .. 2^20"),
        "max_keys 2^40": ((1, 128, 1 << 40), b"max_keys must be 1 .. 2^20"),
    }
    for what, (args, word) in refusals.items():
        assert _check(cfg, *args) == N.GOL_EINVAL, what
        msg = N.lib.gol_batch_last_error(None)
        assert word in msg and b"gol_census_batch_check" in msg, (what, msg)
    assert N.lib.gol_census_batch_check(None, 1, 128, 4096) == N.GOL_EINVAL
    # a geometry gol_batch_create refuses is refused here alike
    assert _check(_cfg(65, 8, topology)) == N.GOL_EINVAL
    assert _check(_cfg(2, 8, N.GOL_TORUS)) == N.GOL_EINVAL


def test_null_handle_is_einval_and_writes_nothing():
    call, n = ctypes.c_uint32(77), ctypes.c_size_t(78)
    entries = np.full(4 * 32, 0x5A, dtype=np.uint8).view(batch.CENSUS_DTYPE)
    before = entries.tobytes()
    recs = np.zeros(2, dtype=batch.OBJECT_DTYPE)
    stats = [ctypes.c_uint64(79) for _ in range(6)]
    for rc in (N.lib.gol_census_batch_begin(None, 16),
               N.lib.gol_census_batch_add(None, 1, 128, ctypes.byref(call)),
               N.lib.gol_census_batch_add_records(None, recs.ctypes.data_as(_P(N.GolBatchObject)), 2, 0,
                                                  ctypes.byref(call)),
               N.lib.gol_census_batch_read(None, entries.ctypes.data_as(_P(N.GolCensusEntry)), 4, ctypes.byref(n)),
               N.lib.gol_census_batch_stats(None, *[ctypes.byref(s) for s in stats])):
        assert rc == N.GOL_EINVAL
        assert b"null handle" in N.lib.gol_batch_last_error(None)
    assert call.value == 77 and n.value == 78 and entries.tobytes() == before and {s.value for s in stats} == {79}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/census_probe.cpp over csrc/gol_batch.h: host code, plain g++ with the HIP headers on its path."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = tmp_path_factory.mktemp("census_probe") / "census_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", include,
                    os.path.join(ROOT, "tests", "census_probe.cpp"), "-o", str(exe)], check=True)

    def ask(call, begun=1, next_call=0, reach=1, max_objects=128, max_keys=4096, records_null=0, n=0, board=0,
            geometry=(3, 8, 8)):
        args = [*geometry, call, begun, next_call, reach, max_objects, max_keys, records_null, n, board]
        return subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True,
                              check=True).stdout.strip()
    return ask


CHECK, BEGIN, ADD, ADD_RECORDS, READ = range(5)


def test_validator_refuses_the_call_after_ordinal_2_to_24_minus_1(probe):
    last = (1 << 24) - 1
    assert probe(ADD, next_call=last) == "ok" and probe(ADD_RECORDS, next_call=last, n=0) == "ok"
    for call in (ADD, ADD_RECORDS):
        assert "ordinals stop at 2^24 - 1" in probe(call, next_call=last + 1)
        assert "ordinals stop at 2^24 - 1" in probe(call, next_call=1 << 40)
    # reading and beginning again are not calls that take an ordinal
    assert probe(READ, next_call=last + 1) == "ok" and probe(BEGIN, next_call=last + 1) == "ok"


def test_validator_states_every_other_refusal(probe):
    for call in (ADD, ADD_RECORDS, READ):
        assert "no census has begun" in probe(call, begun=0)
    assert probe(BEGIN, begun=0) == "ok" and probe(CHECK, begun=0) == "ok"
    assert probe(ADD, reach=3) == "reach must be 1 or 2" and probe(ADD, max_objects=1025) == "max_objects must be 1 .. 1024"
    assert probe(BEGIN, max_keys=0) == "max_keys must be 1 .. 2^20" == probe(BEGIN, max_keys=(1 << 20) + 1)
    assert probe(BEGIN, max_keys=1) == "ok" == probe(BEGIN, max_keys=1 << 20)
    assert probe(ADD_RECORDS, n=1 << 22) == "ok" and probe(ADD_RECORDS, n=(1 << 22) + 1) == "n must be at most 2^22"
    assert probe(ADD_RECORDS, n=1, records_null=1) == "records is null" and probe(ADD_RECORDS, records_null=1) == "ok"
    assert probe(ADD_RECORDS, board=(1 << 22) - 1) == "ok" and probe(ADD_RECORDS, board=1 << 22) == "board must be below 2^22"
    # what a call does not take is not looked at
    assert probe(READ, reach=9, max_objects=0, max_keys=0, n=1 << 30) == "ok"


def test_python_wrapper_has_the_calls():
    for name in ("census_begin", "census_add", "census_add_records", "census_read", "census_stats"):
        assert callable(getattr(batch.GolBatch, name)), name
    assert callable(batch.census_names) and batch.CENSUS_DTYPE.itemsize == 32
