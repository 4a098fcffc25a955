"""CPU: the C ABI of the fused population series (gol_step_series,
gol_group_step_series).  No device is touched: the
symbols, their declarations, the binding's prototypes and the null-context
refusal."""
import ctypes
import re

from gameoflife import _native as N

SERIES = ("gol_step_series", "gol_group_step_series")

# C parameter type -> the ctypes type the binding must declare
CTYPES = {"gol_ctx*": ctypes.c_void_p, "gol_group*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32,
          "uint64_t*": ctypes.POINTER(ctypes.c_uint64), "size_t": ctypes.c_size_t}


def _declaration(name):
    text = open(N.HEADER_PATH).read()
    m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, text, re.M)
    assert m, f"include/gol.h does not declare int {name}(...)"
    params = []
    for p in m.group(1).split(","):
        words = p.replace("*", "* ").split()
        params.append("".join(words[:-1]))  # drop the parameter's name
    return params


def test_library_exports_and_header_declares_both():
    syms = N.header_symbols()
    for name in SERIES:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name


def test_abi_version_stays_2():
    assert N.lib.gol_abi_version() == 2
    assert N.GOL_ABI_VERSION == 2
    assert re.search(r"^#define GOL_ABI_VERSION 2$", open(N.HEADER_PATH).read(), re.M)


def test_prototypes_match_header():
    want_ctx = ["gol_ctx*", "uint32_t", "uint64_t*", "uint64_t*", "size_t"]
    assert _declaration("gol_step_series") == want_ctx
    assert _declaration("gol_group_step_series") == ["gol_group*"] + want_ctx[1:]
    for name in SERIES:
        res, args = N._SIGNATURES[name]
        assert res is ctypes.c_int
        assert args == [CTYPES[t] for t in _declaration(name)], name
        fn = getattr(N.lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args


def test_null_context_is_einval():
    pop = (ctypes.c_uint64 * 4)()
    h = (ctypes.c_uint64 * 4)()
    for name in SERIES:
        fn = getattr(N.lib, name)
        assert fn(None, 4, h, pop, 4) == N.GOL_EINVAL, name
        assert fn(None, 0, None, None, 0) == N.GOL_EINVAL, name
    assert list(pop) == [0, 0, 0, 0] and list(h) == [0, 0, 0, 0]
