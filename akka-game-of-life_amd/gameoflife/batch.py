"""Batch engine: many independent small boards stepped by one launch.

Where the reference runs one BoardCreator -- one actor system -- per board
(BoardCreator.scala:18-23), a ``GolBatch`` holds ``boards`` boards of one
geometry, each at most 64 x 64 stored cells, under one rule or a rule per
board (set_rules: a rule sweep), and advances all of them per launch through libgol's gol_batch_* entry points: random soups until
they settle, one pattern under many perturbations, or many copies of the
reference's own 7 x 7 board.  A board's row is one uint64 (bit x = cell x).
GolBatch.soup generates the soups on the device (a window of any density,
nine symmetries, soup number n a function of the seed and n alone), and
soup_rows gives any one of them back on the host.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from . import patterns as P
from .rules import Rule, rule_by_name, rule_word

# gol_batch_object as a numpy record (N.GolBatchObject's fields in its order, 16 bytes)
OBJECT_DTYPE = P.OBJECT_DTYPE
# gol_census_entry as a numpy record (N.GolCensusEntry's fields in its order, 32 bytes)
CENSUS_DTYPE = np.dtype([("hash", "<u8"), ("w", "u1"), ("h", "u1"), ("population", "<u2"), ("first_call", "<u4"),
                         ("count", "<u8"), ("first_board", "<u4"), ("first_x", "u1"), ("first_y", "u1"),
                         ("reserved", "<u2")])
# the symmetries GolBatch.soup and soup_rows take (include/gol.h GOL_SOUP_*), in their order
SOUP_SYMMETRIES = tuple(N.SOUP_SYMMETRIES)


class GolBatch:
    """A batch of boards on one GPU (gol_batch_create .. gol_batch_destroy)."""

    def __init__(self, boards: int, width: int, height: int, *, topology: str = "torus",
                 rule: Rule | str = "life", vis: tuple[int, int] | None = None, device: int = 0):
        self.rule = rule_by_name(rule) if isinstance(rule, str) else rule
        self.topology = topology
        cfg = N.GolBatchConfig()
        cfg.boards, cfg.width, cfg.height = boards, width, height
        cfg.topology = {"torus": N.GOL_TORUS, "ref-clipped": N.GOL_REF_CLIPPED}[topology]
        cfg.birth_mask, cfg.survive_mask = self.rule.birth, self.rule.survive
        cfg.device = device
        cfg.vis_width, cfg.vis_height = vis if vis is not None else (0, 0)
        self._cfg = cfg
        h = ctypes.c_void_p()
        N.check_batch(N.lib.gol_batch_create(ctypes.byref(h), ctypes.byref(cfg)))
        self._h = h
        self.boards, self.width, self.height = boards, width, height
        self.device = device

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib.gol_batch_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int) -> None:
        N.check_batch(rc, self._h)

    def geometry(self) -> dict:
        """The lane mapping: boards per 64-lane wave, waves, device bytes."""
        g = N.GolBatchGeometry()
        N.check_batch(N.lib.gol_batch_geometry_get(ctypes.byref(self._cfg), ctypes.byref(g)))
        return {"boards_per_wave": g.boards_per_wave, "waves": g.waves, "device_bytes": g.device_bytes}

    # -- state -------------------------------------------------------------
    def seed(self, seed: int = 0x5EED) -> None:
        self._chk(N.lib.gol_batch_seed(self._h, seed))

    def soup(self, seed: int, *, window: tuple[int, int, int, int] | None = None, density: float | int = 0.5,
             symmetry: str = "C1", index0: int = 0, first: int = 0, count: int | None = None) -> None:
        """Boards first .. first + count - 1 become random soups, generated
        on the device (gol_soup_batch): board b holds soup number index0 + b,
        a pure function of (seed, that number) which soup_rows reproduces
        anywhere.  `window` is (x, y, w, h) in stored cells, the rest of the
        board dead (None: the whole stored board); `density` the probability
        of a live cell, a float rounded to n / 256 or an int taken as n, n in
        1 .. 255; `symmetry` one of SOUP_SYMMETRIES (C4, D2_DIAG, D4_DIAG and
        D8 need a square window).  The other boards keep their cells; the
        epoch goes to 0 as after load, per-board rules stay."""
        spec = _soup_spec(self.width, self.height, seed, index0, window, density, symmetry)
        count = self.boards - first if count is None else count
        self._chk(N.lib.gol_soup_batch(self._h, ctypes.byref(spec), first, count))

    def load(self, x, first: int = 0) -> None:
        """Boards first .. first + n - 1 from uint64 [n][H] rows or uint8
        [n][H][W] cells; resets the epoch."""
        a = np.asarray(x)
        if a.ndim == 3:
            a = pack_rows(a)
        a = np.ascontiguousarray(a, dtype=np.uint64)
        if a.ndim != 2 or a.shape[1] != self.height:
            raise ValueError(f"boards must be uint64 [n][{self.height}] rows or uint8 [n][{self.height}]"
                             f"[{self.width}] cells, not {a.shape}")
        self._chk(N.lib.gol_batch_load(self._h, first, a.shape[0], a.ctypes.data_as(N._u64p)))

    def snapshot(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """uint64 [n][H] rows of boards first .. first + count - 1."""
        count = self.boards - first if count is None else count
        out = np.zeros((max(count, 0), self.height), dtype=np.uint64)
        self._chk(N.lib.gol_batch_snapshot(self._h, first, count, out.ctypes.data_as(N._u64p)))
        return out

    def cells(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """uint8 [n][H][W] cells of boards first .. first + count - 1."""
        return unpack_rows(self.snapshot(first, count), self.width)

    def step(self, generations: int = 1, populations: bool = False, settled: bool = False):
        """Advance every board.  populations=True: uint32 [boards][generations],
        the live stored cells of each board after each generation; settled=True:
        uint32 [boards], the first generation g >= 2 of this call at which the
        board equals itself two generations earlier (0: none).  Returns the one
        asked for, (populations, settled) for both, else None."""
        pop = np.zeros((self.boards, generations), dtype=np.uint32) if populations else None
        st = np.zeros(self.boards, dtype=np.uint32) if settled else None
        self._chk(N.lib.gol_batch_step(self._h, generations, pop.ctypes.data_as(N._u32p) if populations else None,
                                       pop.size if populations else 0,
                                       st.ctypes.data_as(N._u32p) if settled else None))
        if populations and settled:
            return pop, st
        return pop if populations else st

    def step_cycles(self, generations: int = 1) -> tuple[np.ndarray, np.ndarray]:
        """Advance every board exactly as step(generations) does, with cycle
        detection (gol_cycle_step): (period, seen), uint32 [boards] each -- the
        board's exact minimal period and the generation of this call at which
        its cycle was seen (Brent's schedule: snapshots at generations 2^k - 1),
        0 and 0 where none was.  A board whose cycle has been seen costs at
        most one period of stepping per launch."""
        period = np.zeros(self.boards, dtype=np.uint32)
        seen = np.zeros(self.boards, dtype=np.uint32)
        self._chk(N.lib.gol_cycle_step(self._h, generations, period.ctypes.data_as(N._u32p),
                                       seen.ctypes.data_as(N._u32p)))
        return period, seen

    def cycle_stats(self) -> dict:
        """The last step_cycles call: launches, boards with a period, the largest period."""
        launches, cycled, longest = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._chk(N.lib.gol_cycle_stats(self._h, ctypes.byref(launches), ctypes.byref(cycled), ctypes.byref(longest)))
        return {"launches": launches.value, "boards_cycled": cycled.value, "max_period": longest.value}

    def hashes(self) -> np.ndarray:
        """Each board's state hash (what GolEngine.hash() gives for the same cells)."""
        out = np.zeros(self.boards, dtype=np.uint64)
        self._chk(N.lib.gol_batch_hashes(self._h, 0, self.boards, out.ctypes.data_as(N._u64p), None))
        return out

    def populations(self) -> np.ndarray:
        """Each board's live stored cells."""
        out = np.zeros(self.boards, dtype=np.uint32)
        self._chk(N.lib.gol_batch_hashes(self._h, 0, self.boards, None, out.ctypes.data_as(N._u32p)))
        return out

    def find(self, patterns, care=None, border: int = 0, orientations: bool = False, matches: bool = False):
        """Count, and locate, patterns on every board, searched on the device
        (gol_find_batch): uint32 [boards][P] -- entry [b][p] is the number of
        anchors of board b at which pattern p matches.  `patterns` is one
        pattern or a list of P; each, with `care` (one mask, or a list of P
        with None where there is none) and `border`, is what patterns.as_search
        takes (RLE text, O/. rows, a cell array; border=1: the object standing
        alone).  An anchor is the board cell under the pattern's top-left
        cell; the pattern wraps on a torus and reads dead beyond a clipped
        board, as GolEngine.find.  matches=True: also uint64 [P][boards][H],
        bit x of [p][b][y] set iff anchor (x, y) of board b matches pattern p
        (match_positions lists them).  orientations=True: each pattern stands
        for its distinct rotations and reflections (patterns.orientations):
        its count is their sum and its match plane their OR, an anchor being
        the top-left cell of the image that matched.  Changes nothing."""
        one = isinstance(patterns, (str, P.Pattern)) or (
            isinstance(patterns, (list, tuple)) and len(patterns) > 0 and all(isinstance(r, str) for r in patterns)) or (
            isinstance(patterns, np.ndarray) and patterns.ndim == 2)
        plist = [patterns] if one else list(patterns)
        cares = [care] * len(plist) if one or care is None else list(care)
        if not plist or len(cares) != len(plist):
            raise ValueError("find takes at least one pattern, and one care mask per pattern if any")
        images, owner = [], []  # the patterns the device searches for, and the asked pattern each stands for
        for i, (pat, msk) in enumerate(zip(plist, cares)):
            cells, mask = P.as_search(pat, msk, border)
            for img in (P.orientations(cells, mask) if orientations else [(cells, mask)]):
                if img[0].shape[1] > self.width or img[0].shape[0] > self.height:
                    if orientations and img[0].shape != cells.shape:
                        continue  # a turned image that does not fit the board matches nowhere
                    raise ValueError(f"pattern {i} ({img[0].shape[1]} x {img[0].shape[0]}, border included) does not "
                                     f"fit a {self.width} x {self.height} board")
                images.append(img)
                owner.append(i)
        n = len(images)
        if n > N.GOL_FIND_BATCH_MAX_PATTERNS:
            raise ValueError(f"{n} patterns (orientations included) in one call; at most "
                             f"{N.GOL_FIND_BATCH_MAX_PATTERNS}")
        rows = [(pack_rows(c[None])[0], pack_rows(m[None])[0]) for c, m in images]  # kept alive through the call
        table = (N.GolBatchPattern * n)()
        for t, (c, _), (rc, rm) in zip(table, images, rows):
            t.ph, t.pw = c.shape
            t.cells, t.care = rc.ctypes.data_as(N._u64p), rm.ctypes.data_as(N._u64p)
        counts = np.zeros((self.boards, n), dtype=np.uint32)
        planes = np.zeros((n, self.boards, self.height), dtype=np.uint64) if matches else None
        self._chk(N.lib.gol_find_batch(self._h, table, n, counts.ctypes.data_as(N._u32p), counts.size,
                                       planes.ctypes.data_as(N._u64p) if matches else None,
                                       planes.size if matches else 0))
        if orientations:  # fold the images back into the patterns asked for
            own = np.asarray(owner)
            counts = np.stack([counts[:, own == i].sum(axis=1, dtype=np.uint32) for i in range(len(plist))], axis=1)
            if matches:
                planes = np.stack([np.bitwise_or.reduce(planes[own == i], axis=0) if (own == i).any()
                                   else np.zeros((self.boards, self.height), dtype=np.uint64)
                                   for i in range(len(plist))])
        return (counts, planes) if matches else counts

    def set_find_cut(self, cared_cells: int) -> None:
        """Knob: cared cells per launch of find (0: automatic); results never depend on it."""
        self._chk(N.lib.gol_find_batch_set_cut(self._h, cared_cells))

    def find_stats(self) -> dict:
        """The last find call: its launches and the cared cells of its patterns."""
        launches, cared = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._chk(N.lib.gol_find_batch_stats(self._h, ctypes.byref(launches), ctypes.byref(cared)))
        return {"launches": launches.value, "cared_cells": cared.value}

    def objects(self, reach: int = 1, max_objects: int = 64, first: int = 0, count: int | None = None):
        """Every board cut into its objects on the device (gol_objects_batch):
        (counts uint32 [n], objects OBJECT_DTYPE [n][max_objects]) for boards
        first .. first + n - 1.  Two live cells belong to one object iff a
        chain of live cells joins them whose steps have Chebyshev distance at
        most `reach` (1: 8-connectivity; 2: islands that can influence a
        common cell), cyclic on a torus; what find(..., border=reach) reports
        is such an object.  counts[b] is exact; objects[b][j] holds object j
        for j < min(counts[b], max_objects) in the order of the objects' first
        cells (row-major), zeros beyond: a translation-invariant hash
        (patterns.object_hash of the object's cells), the bounding box x, y,
        w, h (w == width on a torus: the object goes round) and the
        population.  Changes nothing."""
        count = self.boards - first if count is None else count
        counts = np.zeros(max(count, 0), dtype=np.uint32)
        objs = np.zeros((max(count, 0), max(max_objects, 0)), dtype=OBJECT_DTYPE)
        self._chk(N.lib.gol_objects_batch(self._h, first, count, reach, max_objects, counts.ctypes.data_as(N._u32p),
                                          counts.size, objs.ctypes.data_as(ctypes.POINTER(N.GolBatchObject)),
                                          objs.size))
        return counts, objs

    def objects_stats(self) -> dict:
        """The last objects call: its launches, its objects in all, the boards with more than max_objects."""
        launches, total, cut = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._chk(N.lib.gol_objects_batch_stats(self._h, ctypes.byref(launches), ctypes.byref(total),
                                                ctypes.byref(cut)))
        return {"launches": launches.value, "objects": total.value, "boards_truncated": cut.value}

    def census_begin(self, max_keys: int = 65536) -> None:
        """Begin, or begin again, a census of this batch's objects on the
        device (gol_census_batch_begin): an empty table with room for
        `max_keys` distinct keys (hash, w, h, population), call ordinal 0."""
        self._chk(N.lib.gol_census_batch_begin(self._h, max_keys))

    def census_add(self, reach: int = 1, max_objects: int = 128) -> int:
        """Tally the objects every board holds now (what objects(reach,
        max_objects) would return: the records present, min(count, max_objects)
        per board) into the census, on the device; nothing comes back but this
        call's ordinal -- 0, 1, ... since census_begin -- which the entries'
        first_call refers to.  Changes nothing else."""
        call = ctypes.c_uint32(0)
        self._chk(N.lib.gol_census_batch_add(self._h, reach, max_objects, ctypes.byref(call)))
        return call.value

    def census_add_records(self, records, board: int = 0) -> int:
        """Tally OBJECT_DTYPE records of the caller's (those with population 0
        are skipped) as if they were board `board`'s: censuses of other
        handles, processes or GPUs merged into this one.  Returns the call's
        ordinal."""
        recs = np.ascontiguousarray(records, dtype=OBJECT_DTYPE).reshape(-1)
        call = ctypes.c_uint32(0)
        self._chk(N.lib.gol_census_batch_add_records(self._h, recs.ctypes.data_as(ctypes.POINTER(N.GolBatchObject)),
                                                     recs.size, board, ctypes.byref(call)))
        return call.value

    def census_read(self) -> np.ndarray:
        """The census so far, CENSUS_DTYPE [distinct keys]: per key its count
        and its earliest occurrence (first_call, first_board, first_y, first_x:
        the minimum in that order), sorted by (count descending, hash, w, h,
        population).  Does not clear the census."""
        n = ctypes.c_size_t(0)
        out = np.zeros(self.census_stats()["distinct"], dtype=CENSUS_DTYPE)
        self._chk(N.lib.gol_census_batch_read(self._h, out.ctypes.data_as(ctypes.POINTER(N.GolCensusEntry)), out.size,
                                              ctypes.byref(n)))
        return out[:n.value]

    def census_stats(self) -> dict:
        """The census since census_begin: its calls, and the objects seen,
        tallied, truncated (beyond max_objects on their board) and overflowed
        (no room in the table: begin again with more max_keys), seen = tallied
        + truncated + overflowed, and the distinct keys."""
        v = [ctypes.c_uint64(0) for _ in range(6)]
        self._chk(N.lib.gol_census_batch_stats(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("calls", "seen", "tallied", "truncated", "overflowed", "distinct"), (x.value for x in v)))

    def set_rules(self, rules, first: int = 0) -> None:
        """Boards first .. first + n - 1 take rules of their own
        (gol_rules_batch_set), and from then on step and step_cycles advance
        board i under rule i, exactly as a batch created with that rule
        would.  `rules` is a uint32 array of rule words (rules.rule_word,
        rule_sweep_words) or a sequence of Rule, names or notations
        ("B36/S23") or (birth, survive) pairs; the boards never named keep
        the batch's rule.  None: every board back to the batch's rule.
        Changes neither the boards nor the epoch."""
        if rules is None:
            self._chk(N.lib.gol_rules_batch_set(self._h, 0, self.boards, None))
            return
        if isinstance(rules, np.ndarray) and rules.dtype.kind in "ui":
            if rules.size and (int(rules.min()) < 0 or int(rules.max()) > 0xFFFFFFFF):
                raise ValueError("rule words are uint32")
            words = np.ascontiguousarray(rules, dtype=np.uint32).reshape(-1)
        else:
            words = np.array([rule_word(r) for r in rules], dtype=np.uint32)
        self._chk(N.lib.gol_rules_batch_set(self._h, first, words.size, words.ctypes.data_as(N._u32p)))

    def rules(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """uint32 [n]: the rule words in force for boards first .. first +
        count - 1 (rules.rule_from_word turns one into a Rule) -- the batch's
        own rule where none was set."""
        count = self.boards - first if count is None else count
        out = np.zeros(max(count, 0), dtype=np.uint32)
        self._chk(N.lib.gol_rules_batch_get(self._h, first, count, out.ctypes.data_as(N._u32p)))
        return out

    @property
    def epoch(self) -> int:
        e = ctypes.c_uint64(0)
        self._chk(N.lib.gol_batch_epoch(self._h, ctypes.byref(e)))
        return e.value

    def set_chunk(self, n: int) -> None:
        """Generations per launch (0: automatic); results never depend on it."""
        self._chk(N.lib.gol_batch_set_chunk(self._h, n))


def _soup_spec(width, height, seed, index0, window, density, symmetry) -> N.GolSoupSpec:
    if symmetry not in N.SOUP_SYMMETRIES:
        raise ValueError(f"symmetry must be one of {', '.join(SOUP_SYMMETRIES)}, not {symmetry!r}")
    spec = N.GolSoupSpec()
    spec.seed, spec.index0 = seed & 0xFFFFFFFFFFFFFFFF, index0 & 0xFFFFFFFFFFFFFFFF
    spec.x, spec.y, spec.w, spec.h = (0, 0, width, height) if window is None else window
    spec.density = density if isinstance(density, (int, np.integer)) else int(round(float(density) * 256))
    spec.symmetry = N.SOUP_SYMMETRIES[symmetry]
    return spec


def soup_rows(width: int, height: int, seed: int, index, *, window=None, density=0.5, symmetry: str = "C1",
              topology: str = "torus", vis: tuple[int, int] | None = None) -> np.ndarray:
    """uint64 [n][H]: the boards GolBatch.soup gives soups number `index` (one
    number or n of them) on boards of this geometry, computed on the host
    (gol_soup_batch_rows: no device, no handle).  The reproducer: the soup
    behind a census entry is number index0 + first_board of the soup call
    that preceded census call first_call."""
    cfg = N.GolBatchConfig()
    cfg.boards, cfg.width, cfg.height = 1, width, height
    cfg.topology = {"torus": N.GOL_TORUS, "ref-clipped": N.GOL_REF_CLIPPED}[topology]
    cfg.vis_width, cfg.vis_height = vis if vis is not None else (0, 0)
    numbers = [int(i) for i in np.atleast_1d(np.asarray(index, dtype=object)).reshape(-1)]
    out = np.zeros((len(numbers), height), dtype=np.uint64)
    for i, n in enumerate(numbers):
        spec = _soup_spec(width, height, seed, n, window, density, symmetry)
        N.check_batch(N.lib.gol_soup_batch_rows(ctypes.byref(cfg), ctypes.byref(spec), 0, 1,
                                                out[i].ctypes.data_as(N._u64p), height))
    return out


def rule_sweep_words(births, survives) -> np.ndarray:
    """uint32 [len(births) * len(survives)]: the rule words (rules.rule_word)
    of the cross product of two lists of 9-bit masks, births outermost --
    word [i * len(survives) + j] is (births[i], survives[j]).
    rule_sweep_words(range(512), range(512)) is every Life-like rule."""
    b = np.asarray(list(births), dtype=np.int64).reshape(-1)
    s = np.asarray(list(survives), dtype=np.int64).reshape(-1)
    if (b & ~0x1FF).any() or (s & ~0x1FF).any():
        raise ValueError("rule masks must fit in 9 bits")
    return (b[:, None] | (s[None, :] << 16)).astype(np.uint32).reshape(-1)


def tally(counts, objects, table) -> dict:
    """A census of what GolBatch.objects returned: name -> number of objects,
    over all boards, by `table` (patterns.object_table: (hash, w, h,
    population) -> name); the objects the table does not name are counted
    under None.  Only the records present count (min(count, max_objects) per
    board)."""
    counts = np.asarray(counts)
    objects = np.asarray(objects)
    kept = np.arange(objects.shape[1])[None, :] < counts[:, None]
    recs = objects[kept]
    cols = np.stack([recs[f].astype(np.uint64) for f in ("hash", "w", "h", "population")], axis=1)
    keys, n = np.unique(cols, axis=0, return_counts=True)
    out: dict = {}
    for k, c in zip(keys.tolist(), n.tolist()):
        name = table.get(tuple(k))
        out[name] = out.get(name, 0) + c
    return out


def census_names(entries, table) -> dict:
    """A census GolBatch.census_read returned by name: name -> number of
    objects, by `table` (patterns.object_table), the keys the table does not
    name under None -- tally's keys and meaning."""
    out: dict = {}
    for e in np.asarray(entries).reshape(-1):
        name = table.get((int(e["hash"]), int(e["w"]), int(e["h"]), int(e["population"])))
        out[name] = out.get(name, 0) + int(e["count"])
    return out


def pack_rows(cells) -> np.ndarray:
    """uint8 [n][H][W] cells (W <= 64) -> uint64 [n][H] rows, bit x = cell x."""
    c = np.asarray(cells)
    if c.ndim != 3 or c.shape[2] > 64:
        raise ValueError(f"cells must be [n][H][W] with W <= 64, not {c.shape}")
    weights = np.uint64(1) << np.arange(c.shape[2], dtype=np.uint64)
    return ((c != 0).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)


def match_positions(rows, width: int) -> np.ndarray:
    """One pattern's match plane (GolBatch.find(..., matches=True)[1][p]: uint64
    [boards][H]) as int64 [n][3] of (board, x, y), sorted by (board, y, x)."""
    bits = unpack_rows(rows, width)
    b, y, x = np.nonzero(bits)  # row-major: sorted by (board, y, x)
    return np.stack([b, x, y], axis=1).astype(np.int64)


def unpack_rows(rows, width: int) -> np.ndarray:
    """uint64 [n][H] rows -> uint8 [n][H][width] cells."""
    r = np.asarray(rows, dtype=np.uint64)
    return ((r[:, :, None] >> np.arange(width, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
