"""The seeded boards the object tests share (tests/test_objects_host.py on the
CPU, tests/test_gpu_batch_objects.py on the device) -- test infrastructure.
The nine shapes of tests/test_gpu_batch_cycles.py::CASES with its seed, each
as the raw soup and after the generations listed here, stepped by the model of
tests/batch_model.py; the objects are those of tests/objects_model.py.
Everything is computed once per session and shared read-only."""
import functools

import batch_model as M
import objects_model as OM
from test_gpu_batch_cycles import CASES, SEED

MAX_OBJECTS = 128
REACHES = (1, 2)
# generations after which each shape is checked, next to the raw soup (0)
GENERATIONS = {
    (64, 64, "torus"): (0, 64, 1024),       # rotates, one board per wave; raw: one object of about 2000 cells
    (64, 64, "ref-clipped"): (0, 1024),
    (8, 8, "torus"): (0, 512),              # k = 8, a short last wave, permutes
    (8, 8, "ref-clipped"): (0, 64),
    (5, 7, "torus"): (0, 64),               # k = 9 with an idle lane
    (33, 21, "torus"): (0, 512),            # rows across the dword boundary
    (20, 64, "torus"): (0, 512),            # rotates on a narrow board
    (64, 3, "torus"): (0, 64),              # k = 21
    (3, 3, "torus"): (0,),                  # every object goes round both axes
}
SHAPES = [(shape, boards) for shape, boards, _, _ in CASES]
assert len(SHAPES) == 9 and {s[:3] for s, _ in SHAPES} == set(GENERATIONS)


def shape_id(case):
    (W, H, topo, vis), boards = case
    return f"{W}x{H}-{topo}-{boards}b"


def generations(shape):
    return GENERATIONS[shape[:3]]


@functools.lru_cache(maxsize=None)
def states(shape, boards):
    """{generation: uint64 [boards][H] rows} of the seeded boards at the shape's generations."""
    W, H, topo, vis = shape
    gens = generations(shape)
    hist = M.run_history(M.seed_rows(boards, W, H, SEED), W, max(gens), topo, vis=vis)[0]
    out = {g: hist[g].copy() for g in gens}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(shape, boards, generation, reach, max_objects=MAX_OBJECTS):
    """(counts, objects) of the model for the seeded boards after `generation`."""
    W, H, topo, vis = shape
    out = OM.batch_objects(states(shape, boards)[generation], W, topo == "torus", reach, max_objects)
    for a in out:
        a.setflags(write=False)
    return out
