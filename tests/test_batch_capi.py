"""CPU: the C ABI of the batch engine (gol_batch_*).  No
device is touched: the symbols, their declarations and the binding's
prototypes, the struct layouts, the lane mapping gol_batch_geometry_get
reports, and every refusal that comes before device work."""
import ctypes
import os
import re
import subprocess

import pytest

from gameoflife import _native as N
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH = ("gol_batch_geometry_get", "gol_batch_create", "gol_batch_destroy", "gol_batch_last_error", "gol_batch_seed",
         "gol_batch_load", "gol_batch_snapshot", "gol_batch_step", "gol_batch_hashes", "gol_batch_epoch",
         "gol_batch_set_chunk")

_P = ctypes.POINTER
# C parameter type -> the ctypes type the binding must declare
CTYPES = {"gol_batch*": ctypes.c_void_p, "constgol_batch*": ctypes.c_void_p, "gol_batch**": _P(ctypes.c_void_p),
          "constgol_batch_config*": _P(N.GolBatchConfig), "gol_batch_geometry*": _P(N.GolBatchGeometry),
          "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64,
          "size_t": ctypes.c_size_t, "uint32_t*": _P(ctypes.c_uint32), "uint64_t*": _P(ctypes.c_uint64),
          "constuint64_t*": _P(ctypes.c_uint64)}
RESULT = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p}


def _declaration(name):
    """(result type, parameter types) of `name` as include/gol.h declares it."""
    text = open(N.HEADER_PATH).read()
    m = re.search(r"^(int|void|const char\*)\s+%s\s*\(([^)]*)\)\s*;" % name, text, re.M)
    assert m, f"include/gol.h does not declare {name}(...)"
    params = []
    for p in m.group(2).split(","):
        words = p.replace("*", "* ").split()
        params.append("".join(words[:-1]).replace("* *", "**"))  # drop the parameter's name
    return m.group(1), params


def _cfg(boards=1, width=8, height=8, topology=N.GOL_TORUS, rule=O.LIFE, vis=(0, 0)):
    c = N.GolBatchConfig()
    c.boards, c.width, c.height, c.topology = boards, width, height, topology
    c.birth_mask, c.survive_mask = rule
    c.device = 0
    c.vis_width, c.vis_height = vis
    return c


def _geometry(cfg):
    g = N.GolBatchGeometry()
    rc = N.lib.gol_batch_geometry_get(ctypes.byref(cfg), ctypes.byref(g))
    return rc, g


def test_library_exports_header_declares_binding_signs():
    syms = N.header_symbols()
    for name in BATCH:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name
    # ... and the header declares no batch entry point this list misses
    assert sorted(s for s in syms if s.startswith("gol_batch_")) == sorted(BATCH)


def test_prototypes_match_header():
    for name in BATCH:
        res_c, params = _declaration(name)
        res, args = N._SIGNATURES[name]
        assert res is RESULT[res_c], name
        assert args == [CTYPES[t] for t in params], (name, params)
        fn = getattr(N.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _declaration("gol_batch_step")[1] == ["gol_batch*", "uint32_t", "uint32_t*", "size_t", "uint32_t*"]
    assert _declaration("gol_batch_hashes")[1] == ["gol_batch*", "int64_t", "int64_t", "uint64_t*", "uint32_t*"]


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gol.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gol_batch_config),'
                   ' offsetof(gol_batch_config, width), offsetof(gol_batch_config, topology),'
                   ' offsetof(gol_batch_config, survive_mask), offsetof(gol_batch_config, device),'
                   ' offsetof(gol_batch_config, vis_height), sizeof(gol_batch_geometry),'
                   ' offsetof(gol_batch_geometry, boards_per_wave), offsetof(gol_batch_geometry, waves),'
                   ' offsetof(gol_batch_geometry, device_bytes)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    C, G = N.GolBatchConfig, N.GolBatchGeometry
    assert got == [ctypes.sizeof(C), C.width.offset, C.topology.offset, C.survive_mask.offset, C.device.offset,
                   C.vis_height.offset, ctypes.sizeof(G), G.boards_per_wave.offset, G.waves.offset,
                   G.device_bytes.offset]


def test_abi_version_stays_2():
    assert N.lib.gol_abi_version() == 2
    assert N.GOL_ABI_VERSION == 2
    assert re.search(r"^#define GOL_ABI_VERSION 2$", open(N.HEADER_PATH).read(), re.M)


@pytest.mark.parametrize("H,k", [(64, 1), (33, 1), (21, 3), (8, 8), (7, 9), (3, 21)])
def test_boards_per_wave_and_waves(H, k):
    for boards in sorted({1, max(k - 1, 1), k, k + 1, 4 * k + 1, 1000}):
        rc, g = _geometry(_cfg(boards, 8, H))
        assert rc == N.GOL_OK
        assert g.boards_per_wave == k
        assert g.waves == -(-boards // k), (H, boards)
        assert g.device_bytes >= boards * H * 8


def test_geometry_accepts_the_shapes_the_gpu_tests_use():
    for (W, H, topo, vis) in ((64, 64, N.GOL_TORUS, (0, 0)), (64, 64, N.GOL_REF_CLIPPED, (64, 63)),
                              (63, 64, N.GOL_REF_CLIPPED, (0, 0)), (8, 8, N.GOL_REF_CLIPPED, (0, 0)),
                              (5, 7, N.GOL_TORUS, (0, 0)), (33, 21, N.GOL_TORUS, (0, 0)),
                              (32, 33, N.GOL_REF_CLIPPED, (0, 0)), (64, 3, N.GOL_TORUS, (0, 0)),
                              (3, 3, N.GOL_TORUS, (0, 0)), (20, 64, N.GOL_TORUS, (0, 0))):
        assert _geometry(_cfg(4, W, H, topo, vis=vis))[0] == N.GOL_OK, (W, H, topo, vis)
    assert _geometry(_cfg(1 << 22))[0] == N.GOL_OK


@pytest.mark.parametrize("kw", [
    dict(width=65), dict(height=65), dict(width=65, topology=N.GOL_REF_CLIPPED),
    dict(height=65, topology=N.GOL_REF_CLIPPED), dict(width=2), dict(height=2), dict(width=0), dict(boards=0),
    dict(boards=-1), dict(boards=(1 << 22) + 1), dict(topology=2), dict(topology=-1), dict(rule=(0x200, 0x00C)),
    dict(width=10, height=10, topology=N.GOL_REF_CLIPPED, vis=(7, 9)),
    dict(width=10, height=10, topology=N.GOL_REF_CLIPPED, vis=(9, 7)),
    # found by tests/test_sweep_cases.py: visible extents beyond the stored board still leave one visible cell
    dict(width=1, height=1, topology=N.GOL_REF_CLIPPED, vis=(2, 2)),
    dict(width=2, height=1, topology=N.GOL_REF_CLIPPED, vis=(1, 2)),
    dict(width=1, height=2, topology=N.GOL_REF_CLIPPED, vis=(2, 1)),
])
def test_geometry_refusals(kw):
    rc, _ = _geometry(_cfg(**kw))
    assert rc == N.GOL_EINVAL, kw
    assert N.lib.gol_batch_last_error(None)
    # gol_batch_create refuses alike, before it looks for a device
    h = ctypes.c_void_p()
    cfg = _cfg(**kw)
    assert N.lib.gol_batch_create(ctypes.byref(h), ctypes.byref(cfg)) == N.GOL_EINVAL
    assert not h.value


@pytest.mark.parametrize("w", range(0, 5))
@pytest.mark.parametrize("h", range(0, 5))
def test_clipped_boards_the_reference_stalls_on_are_refused(w, h):
    # the boards of tests/test_degenerate_geometry.py: stored (w + 1) x (h + 1), default visible extents
    rc, _ = _geometry(_cfg(3, w + 1, h + 1, N.GOL_REF_CLIPPED))
    assert rc == (N.GOL_OK if O.reference_completes(w, h) else N.GOL_EINVAL)


def test_visible_extents_that_strand_cells_are_refused_as_gol_create_refuses_them():
    # 64 x 64 stored cells with visible extents (40, 50): columns 42 .. 63 see no visible cell, so the board is one
    # gol_create refuses -- and the batch refuses it the same way (it cannot be a GPU test shape)
    from gameoflife.engine import GolEngine
    with pytest.raises(N.GolError) as ei:
        GolEngine(64, 64, topology="ref-clipped", vis=(40, 50))
    assert ei.value.code == N.GOL_EINVAL
    assert _geometry(_cfg(1, 64, 64, N.GOL_REF_CLIPPED, vis=(40, 50)))[0] == N.GOL_EINVAL
    for vis in ((63, 63), (64, 63), (63, 64), (64, 64)):
        assert _geometry(_cfg(1, 64, 64, N.GOL_REF_CLIPPED, vis=vis))[0] == N.GOL_OK, vis


def test_clipped_refusal_cites_the_reference():
    rc, _ = _geometry(_cfg(1, 2, 2, N.GOL_REF_CLIPPED))
    assert rc == N.GOL_EINVAL
    assert b"NextStateCellGathererActor.scala" in N.lib.gol_batch_last_error(None)
    assert _geometry(_cfg(1, 10, 10, N.GOL_REF_CLIPPED, vis=(9, 9)))[0] == N.GOL_OK


def test_null_arguments_are_einval():
    L = N.lib
    cfg, g, h = _cfg(), N.GolBatchGeometry(), ctypes.c_void_p()
    assert L.gol_batch_geometry_get(None, ctypes.byref(g)) == N.GOL_EINVAL
    assert L.gol_batch_geometry_get(ctypes.byref(cfg), None) == N.GOL_EINVAL
    assert L.gol_batch_create(None, ctypes.byref(cfg)) == N.GOL_EINVAL
    assert L.gol_batch_create(ctypes.byref(h), None) == N.GOL_EINVAL
    rows = (ctypes.c_uint64 * 8)(*([7] * 8))
    pops = (ctypes.c_uint32 * 8)(*([9] * 8))
    hs = (ctypes.c_uint64 * 8)(*([5] * 8))
    e = ctypes.c_uint64(11)
    assert L.gol_batch_seed(None, 1) == N.GOL_EINVAL
    assert L.gol_batch_load(None, 0, 1, rows) == N.GOL_EINVAL
    assert L.gol_batch_snapshot(None, 0, 1, rows) == N.GOL_EINVAL
    assert L.gol_batch_step(None, 2, pops, 8, pops) == N.GOL_EINVAL
    assert L.gol_batch_step(None, 0, None, 0, None) == N.GOL_EINVAL
    assert L.gol_batch_hashes(None, 0, 1, hs, pops) == N.GOL_EINVAL
    assert L.gol_batch_epoch(None, ctypes.byref(e)) == N.GOL_EINVAL
    assert L.gol_batch_set_chunk(None, 7) == N.GOL_EINVAL
    L.gol_batch_destroy(None)  # nothing happens
    assert L.gol_batch_last_error(None)  # the process-wide message of the last refusal
    assert list(rows) == [7] * 8 and list(pops) == [9] * 8 and list(hs) == [5] * 8 and e.value == 11


def test_create_without_a_device_is_enodev():
    h = ctypes.c_void_p()
    cfg = _cfg(3, 8, 8, N.GOL_REF_CLIPPED)
    rc = N.lib.gol_batch_create(ctypes.byref(h), ctypes.byref(cfg))
    if N.device_count() != 0:  # with a device the same call succeeds (tests/test_gpu_batch.py goes on from there)
        assert rc == N.GOL_OK and h.value
        N.lib.gol_batch_destroy(h)
        return
    assert rc == N.GOL_ENODEV
    assert not h.value
    assert b"no CPU fallback" in N.lib.gol_batch_last_error(None)
    from gameoflife.batch import GolBatch
    with pytest.raises(N.GolError) as ei:
        GolBatch(3, 8, 8, topology="ref-clipped")
    assert ei.value.code == N.GOL_ENODEV


def test_python_wrapper_is_exported():
    import gameoflife
    from gameoflife.batch import GolBatch
    assert gameoflife.GolBatch is GolBatch and "GolBatch" in gameoflife.__all__
