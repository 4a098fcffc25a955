"""CPU: the C ABI of cycle detection on a batch (gol_cycle_*; DESIGN.md section
5g).  No device is touched: the symbols, their declarations and the binding's
prototypes, the schedule function against the model's formula, and the
refusals that come before device work."""
import ctypes
import re

from gameoflife import _native as N

import cycle_model as C

CYCLE = ("gol_cycle_step", "gol_cycle_snapshot_generation", "gol_cycle_stats")
_P = ctypes.POINTER
CTYPES = {"gol_batch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint32_t*": _P(ctypes.c_uint32),
          "uint64_t*": _P(ctypes.c_uint64)}


def _declaration(name):
    """(result type, parameter types) of `name` as include/gol.h declares it."""
    text = open(N.HEADER_PATH).read()
    m = re.search(r"^(int|void|const char\*)\s+%s\s*\(([^)]*)\)\s*;" % name, text, re.M)
    assert m, f"include/gol.h does not declare {name}(...)"
    params = []
    for p in m.group(2).split(","):
        words = p.replace("*", "* ").split()
        params.append("".join(words[:-1]))  # drop the parameter's name
    return m.group(1), params


def test_declared_exported_and_bound():
    syms = N.header_symbols()
    for name in CYCLE:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name
    assert sorted(s for s in syms if s.startswith("gol_cycle_")) == sorted(CYCLE)


def test_prototypes_match_header():
    for name in CYCLE:
        res_c, params = _declaration(name)
        res, args = N._SIGNATURES[name]
        assert res_c == "int" and res is ctypes.c_int, name
        assert args == [CTYPES[t] for t in params], (name, params)
        fn = getattr(N.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _declaration("gol_cycle_step")[1] == ["gol_batch*", "uint32_t", "uint32_t*", "uint32_t*"]
    assert _declaration("gol_cycle_snapshot_generation")[1] == ["uint32_t", "uint32_t*"]
    assert _declaration("gol_cycle_stats")[1] == ["gol_batch*", "uint64_t*", "uint64_t*", "uint32_t*"]


def _snapshot_generation(g):
    out = ctypes.c_uint32(0xDEAD)
    assert N.lib.gol_cycle_snapshot_generation(g, ctypes.byref(out)) == N.GOL_OK, g
    return out.value


def test_snapshot_generation_equals_the_model():
    for g in list(range(1, 5001)) + [2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1]:
        assert _snapshot_generation(g) == C.snapshot_generation(g), g
    assert _snapshot_generation(2**32 - 1) == 2**31 - 1 and _snapshot_generation(2**31 - 1) == 2**30 - 1


def test_refusals_before_device_work():
    out = ctypes.c_uint32(0xDEAD)
    assert N.lib.gol_cycle_snapshot_generation(0, ctypes.byref(out)) == N.GOL_EINVAL
    assert out.value == 0xDEAD
    assert N.lib.gol_cycle_snapshot_generation(5, None) == N.GOL_EINVAL
    period = (ctypes.c_uint32 * 4)(*([9] * 4))
    seen = (ctypes.c_uint32 * 4)(*([7] * 4))
    assert N.lib.gol_cycle_step(None, 3, period, seen) == N.GOL_EINVAL
    assert N.lib.gol_cycle_step(None, 0, None, None) == N.GOL_EINVAL
    launches, boards, longest = ctypes.c_uint64(11), ctypes.c_uint64(12), ctypes.c_uint32(13)
    assert N.lib.gol_cycle_stats(None, ctypes.byref(launches), ctypes.byref(boards),
                                 ctypes.byref(longest)) == N.GOL_EINVAL
    assert N.lib.gol_batch_last_error(None)
    assert list(period) == [9] * 4 and list(seen) == [7] * 4
    assert (launches.value, boards.value, longest.value) == (11, 12, 13)


def test_abi_version_stays_2():
    assert N.lib.gol_abi_version() == 2 and N.GOL_ABI_VERSION == 2


def test_python_wrapper_has_the_calls():
    from gameoflife.batch import GolBatch
    assert callable(GolBatch.step_cycles) and callable(GolBatch.cycle_stats)
