"""The boards and patterns of the batch pattern search's tests
(tests/test_batch_find_model.py on the CPU, tests/test_gpu_batch_find.py on the
device): the shapes of tests/test_gpu_batch_cycles.py, seeded alike, and per
shape the pattern lists and the cell-level answer of tests/find_model.py,
computed once and shared read-only."""
import functools

import numpy as np

import batch_model as M
import cycle_model as C
import find_model as F
from gameoflife import patterns as P

SEED = 0xBA7C4

# (W, H, topology, vis), boards, generations the ash cases step first
SHAPES = [
    ((64, 64, "torus", None), 5, 1024),                 # one board per wave, rotate distance 64
    ((64, 64, "ref-clipped", (64, 63)), 5, 1024),
    ((8, 8, "torus", None), 33, 64),                    # 8 boards per wave, short last wave
    ((8, 8, "ref-clipped", None), 33, 64),
    ((5, 7, "torus", None), 37, 64),                    # an idle lane
    ((33, 21, "torus", None), 13, 512),                 # a row across the dword boundary
    ((20, 64, "torus", None), 5, 512),                  # narrow
    ((64, 3, "torus", None), 85, 64),                   # 21 boards per wave
    ((3, 3, "torus", None), 85, 64),
]

BLOCK = ["OO", "OO"]
BLINKER_H = ["OOO"]
BLINKER_V = ["O", "O", "O"]
BEEHIVE = [".OO.", "O..O", ".OO."]
GLIDER = [".O.", "..O", "OOO"]
OBJECTS = [BLOCK, BLINKER_H, BLINKER_V, BEEHIVE]
# the shapes the ash cases run on: a board of 3 rows holds no bordered object but the horizontal blinker, and the
# seeded 64 x 3 boards have none after 64 generations
ASH_SHAPES = slice(0, 7)


def shape_id(case):
    (W, H, topo, vis), boards = case[:2]
    return f"{W}x{H}-{topo}" + (f"-vis{vis[0]}x{vis[1]}" if vis else "") + f"-{boards}b"


def fits(shape, cells):
    return cells.shape[1] <= shape[0] and cells.shape[0] <= shape[1]


@functools.lru_cache(maxsize=None)
def boards_after(shape, boards, gens):
    """uint64 [boards][H]: the seeded boards after `gens` generations of B3/S23; read-only."""
    W, H, topo, vis = shape
    rows = M.seed_rows(boards, W, H, SEED)
    if gens:
        rows = C.run(rows, W, gens, topo, vis=vis)[0]
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    rows.setflags(write=False)
    return rows


def soup_patterns(shape, boards):
    """The (cells, care) list searched on the raw seeded soup: the 1 x 1 live
    cell, the bare block, a care mask with holes, the empty cared 3 x 3 box,
    board 0 itself (pw = width, ph = height) and, on 64 columns, a pattern with
    a cared column 63 -- each where it fits the board."""
    W, H = shape[0], shape[1]
    board0 = M.unpack(boards_after(shape, boards, 0), W)[0]
    out = [P.as_search(["O"]), P.as_search(BLOCK), P.as_search(["O?O", "?.?"]), P.as_search(["...", "...", "..."]),
           P.as_search(board0)]
    if W == 64:
        # columns 0, 31, 32 and 63 of board 0's row 1, nothing between: a row of four cared cells, two in each dword
        care = np.zeros((1, 64), dtype=np.uint8)
        care[0, [0, 31, 32, 63]] = 1
        out.append(P.as_search(board0[1:2], care))
    return [pc for pc in out if fits(shape, pc[0])]


def ash_patterns(shape):
    """Block, both blinker phases and beehive standing alone (border=1), then a glider (of which ash that old holds
    few: every 64 x 64 torus board has each of the four), where they fit."""
    return [pc for pc in (P.as_search(o, border=1) for o in OBJECTS + [GLIDER]) if fits(shape, pc[0])]


def nine_patterns(shape, boards):
    """A list of 9 for one call: the soup list, then the ash list, then the bare objects, cut to 9."""
    out = soup_patterns(shape, boards) + ash_patterns(shape) + [pc for pc in (P.as_search(o) for o in OBJECTS)
                                                                if fits(shape, pc[0])]
    out += [P.as_search(["O"])] * 9  # 3 x 3 boards hold few of the above
    return out[:9]


def reference(rows, shape, patterns):
    """(counts uint32 [boards][P], planes uint64 [P][boards][H]) by tests/find_model.py on the unpacked cells."""
    W, H, topo, _ = shape
    cells = M.unpack(rows, W)
    maps = np.array([[F.match_map(b, c, m, topo == "torus") for b in cells] for c, m in patterns], dtype=np.uint8)
    planes = M.pack(maps.reshape(-1, H, W)).reshape(len(patterns), len(cells), H)
    counts = maps.reshape(len(patterns), len(cells), -1).sum(axis=2).T.astype(np.uint32)
    return counts, planes


@functools.lru_cache(maxsize=None)
def reference_for(shape, boards, gens, which):
    """reference() of the `which` list ("soup", "ash", "nine") on boards_after(shape, boards, gens); read-only."""
    patterns = {"soup": lambda: soup_patterns(shape, boards), "ash": lambda: ash_patterns(shape),
                "nine": lambda: nine_patterns(shape, boards)}[which]()
    out = reference(boards_after(shape, boards, gens), shape, patterns)
    for a in out:
        a.setflags(write=False)
    return patterns, out[0], out[1]
