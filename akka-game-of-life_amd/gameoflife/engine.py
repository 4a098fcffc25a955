"""Shard engine: one libgol context = one backend worker owning a row block.

The reference's backend hosts cell actors (CellActor.scala:10-102), each
holding its own history and computing its next state by messaging its
neighbours.  Here a backend worker owns a contiguous row block of the board in
HBM and advances all of it per generation through libgol.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from . import codec, patterns
from .rules import Rule, rule_by_name


class GolEngine:
    """A shard context on one GPU (gol_create .. gol_destroy)."""

    def __init__(self, width: int, height: int, *, topology: str = "torus",
                 rule: Rule | str = "life", device: int = 0, row0: int = 0,
                 rows: int | None = None, vis: tuple[int, int] | None = None, active_rows: bool = False):
        self.rule = rule_by_name(rule) if isinstance(rule, str) else rule
        self.topology = topology
        topo = {"torus": N.GOL_TORUS, "ref-clipped": N.GOL_REF_CLIPPED}[topology]
        cfg = N.GolConfig()
        cfg.width = width
        cfg.height = height
        cfg.row0 = row0
        cfg.rows = (height - row0) if rows is None else rows
        cfg.topology = topo
        cfg.birth_mask = self.rule.birth
        cfg.survive_mask = self.rule.survive
        cfg.device = device
        cfg.vis_width, cfg.vis_height = vis if vis is not None else (0, 0)
        h = ctypes.c_void_p()
        N.check(N.lib.gol_create(ctypes.byref(h), ctypes.byref(cfg)))
        self._h = h
        self.width, self.height = width, height
        self.row0, self.rows = row0, cfg.rows
        self.wwords = (width + 31) // 32
        self.device = device
        if active_rows:
            self.set_active_rows(True)

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib.gol_destroy(self._h)
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
        N.check(rc, self._h)

    # -- state -------------------------------------------------------------
    def seed(self, seed: int = 0x5EED) -> None:
        self._chk(N.lib.gol_seed(self._h, seed))

    def load(self, packed: np.ndarray) -> None:
        a = np.ascontiguousarray(packed, dtype=np.uint32)
        assert a.shape[0] == self.rows and a.shape[1] >= self.wwords, a.shape
        self._chk(N.lib.gol_load(self._h, a.ctypes.data_as(N._u32p), a.shape[1]))

    def snapshot(self, out: np.ndarray | None = None) -> np.ndarray:
        """Current board, row-major host layout.  `out`: a caller-owned
        (rows, wwords) uint32 C-contiguous buffer to fill -- reusing one (or a
        pinned one) avoids first-touch page faults on every snapshot."""
        if out is None:
            out = np.zeros((self.rows, self.wwords), dtype=np.uint32)
        elif out.dtype != np.uint32 or out.shape != (self.rows, self.wwords) or not out.flags.c_contiguous:
            raise ValueError(f"snapshot buffer must be a C-contiguous uint32 array of shape {(self.rows, self.wwords)}")
        self._chk(N.lib.gol_snapshot(self._h, out.ctypes.data_as(N._u32p), self.wwords))
        return out

    def snapshot_async(self, out: np.ndarray) -> None:
        """Start copying the current board into `out` (as snapshot()'s
        buffer; a page-locked one from host_buffer() keeps the call from
        blocking) while later steps run; snapshot_wait() finishes it."""
        if out.dtype != np.uint32 or out.shape != (self.rows, self.wwords) or not out.flags.c_contiguous:
            raise ValueError(f"snapshot buffer must be a C-contiguous uint32 array of shape {(self.rows, self.wwords)}")
        self._chk(N.lib.gol_snapshot_async(self._h, out.ctypes.data_as(N._u32p), self.wwords))
        self._snap_out = out  # keep the buffer alive while the copy is in flight

    def snapshot_wait(self) -> int:
        """Finish the snapshot started by snapshot_async; returns its epoch."""
        e = ctypes.c_uint64(0)
        try:
            self._chk(N.lib.gol_snapshot_wait(self._h, ctypes.byref(e)))
        finally:
            self._snap_out = None
        return e.value

    def snapshot_landed(self) -> bool:
        """Has the snapshot started by snapshot_async reached its buffer?
        (gol_snapshot_query: non-blocking; snapshot_wait still ends it)."""
        d = ctypes.c_int(0)
        self._chk(N.lib.gol_snapshot_query(self._h, ctypes.byref(d)))
        return bool(d.value)

    def host_buffer(self) -> np.ndarray:
        """A page-locked (rows, wwords) uint32 buffer for snapshots / loads."""
        return host_array((self.rows, self.wwords))

    def step(self, generations: int = 1, hashes: bool = False, populations: bool = False):
        """Advance; returns the per-generation partial hashes (uint64) if asked.
        populations=True: the per-generation populations of this shard's rows
        (uint64, gol_step_series: counted inside the step kernels, what
        population() would give after each generation), or (hashes,
        populations) when both are asked."""
        if populations:
            pop = np.zeros(generations, dtype=np.uint64)
            out = np.zeros(generations, dtype=np.uint64) if hashes else None
            self._chk(N.lib.gol_step_series(self._h, generations, out.ctypes.data_as(N._u64p) if hashes else None,
                                            pop.ctypes.data_as(N._u64p), pop.size))
            return (out, pop) if hashes else pop
        if hashes:
            out = np.zeros(generations, dtype=np.uint64)
            self._chk(N.lib.gol_step_ex(self._h, generations, out.ctypes.data_as(N._u64p), out.size))
            return out
        self._chk(N.lib.gol_step(self._h, generations, None))
        return None

    def sync(self) -> None:
        self._chk(N.lib.gol_sync(self._h))

    @property
    def epoch(self) -> int:
        e = ctypes.c_uint64(0)
        self._chk(N.lib.gol_epoch(self._h, ctypes.byref(e)))
        return e.value

    def hash(self) -> int:
        h = ctypes.c_uint64(0)
        self._chk(N.lib.gol_hash(self._h, ctypes.byref(h)))
        return h.value

    def get_cell(self, x: int, y: int) -> bool:
        s = ctypes.c_int(0)
        self._chk(N.lib.gol_get_cell(self._h, x, y, ctypes.byref(s)))
        return bool(s.value)

    # -- patterns, windows and census (DESIGN.md "Patterns, windows and census")
    def _census_raw(self) -> tuple[int, int, int, int, int]:
        """(population, min_x, max_x, min_y, max_y) of this shard's rows, with
        gol_census's sentinels when nothing is alive."""
        r = N.GolCensusResult()
        self._chk(N.lib.gol_census(self._h, ctypes.byref(r)))
        return r.population, r.min_x, r.max_x, r.min_y, r.max_y

    def census(self) -> dict:
        """Live cells of this shard's rows and their bounding box, counted on
        the device: {"population": n, "bbox": (min_x, min_y, max_x, max_y)},
        inclusive global coordinates, bbox None when nothing is alive."""
        return _census_dict(*self._census_raw())

    def population(self) -> int:
        return self._census_raw()[0]

    def _read_region_into(self, x: int, y: int, w: int, h: int, packed: np.ndarray) -> None:
        self._chk(N.lib.gol_read_region(self._h, x, y, w, h, packed.ctypes.data_as(N._u32p), packed.shape[1]))

    def read_region(self, x: int, y: int, w: int, h: int) -> np.ndarray:
        """The w x h window at (x, y) as a uint8 [h][w] cell array (a torus
        wraps it).  Rows this shard does not own come back dead: the same call
        on every shard of a board fills one buffer (ShardGroup.read_region)."""
        packed = _window_buffer(w, h)
        self._read_region_into(x, y, w, h, packed)
        return codec.unpack(packed, w)

    def _write_region_packed(self, x: int, y: int, w: int, h: int, packed: np.ndarray, mode: str) -> None:
        if mode not in N.REGION_MODES:
            raise ValueError(f"mode must be one of {sorted(N.REGION_MODES)}, not {mode!r}")
        self._chk(N.lib.gol_write_region(self._h, x, y, w, h, packed.ctypes.data_as(N._u32p), packed.shape[1],
                                         N.REGION_MODES[mode]))

    def write_region(self, x: int, y: int, cells, mode: str = "copy") -> None:
        """Combine a [h][w] cell array into the window at (x, y): mode "copy"
        replaces the window, "or" adds the live cells, "xor" toggles them,
        "clear" kills them.  The epoch stays; rows this shard does not own are
        skipped."""
        c = patterns.as_cells(cells)
        self._write_region_packed(x, y, c.shape[1], c.shape[0], codec.pack(c), mode)

    def set_cell(self, x: int, y: int, alive: bool = True) -> None:
        self.write_region(x, y, np.ones((1, 1), dtype=np.uint8), "or" if alive else "clear")

    def place(self, pattern, x: int, y: int, mode: str = "or") -> None:
        """Drop a pattern -- RLE text, a list of O/. rows, or a cell array
        (gameoflife.patterns) -- with its top-left cell at (x, y)."""
        self.write_region(x, y, patterns.as_cells(pattern), mode)

    def _density_into(self, x: int, y: int, w: int, h: int, log2_tile: int, counts: np.ndarray) -> None:
        self._chk(N.lib.gol_density(self._h, x, y, w, h, log2_tile, counts.ctypes.data_as(N._u32p), counts.shape[1]))

    def density(self, tile: int, x: int = 0, y: int = 0, w: int | None = None, h: int | None = None) -> np.ndarray:
        """The zoomed-out view, counted on the device: a uint32 [th][tw] map
        of the live cells per tile x tile block of the w x h window at (x, y),
        tiles anchored at the window origin, the last one in each direction
        possibly partial.  `tile` is a power of two from 1 to 32768; w and h
        default to the rest of the board from (x, y) -- on a torus, which
        wraps the window, to the whole width and height.  Rows this shard
        does not own count nothing (ShardGroup.density sums the shards)."""
        lg = _log2_tile(tile)
        w, h = _density_window(self, x, y, w, h)
        counts = _density_buffer(w, h, lg)
        self._density_into(x, y, w, h, lg, counts)
        return counts

    def _find_raw(self, cells: np.ndarray, care: np.ndarray, x: int, y: int, w: int, h: int,
                  max_matches: int) -> tuple[int, np.ndarray, int]:
        """gol_find with a prepared pattern (patterns.as_search): (count,
        int64 [m][2] matches sorted by (y, x), rows searched) of this shard."""
        pat, mask = codec.pack(cells), codec.pack(care)
        xy = np.zeros((max(int(max_matches), 0), 2), dtype=np.int64)
        res = N.GolFindResult()
        self._chk(N.lib.gol_find(self._h, x, y, w, h, pat.ctypes.data_as(N._u32p), mask.ctypes.data_as(N._u32p),
                                 pat.shape[1], cells.shape[1], cells.shape[0],
                                 xy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if xy.size else None,
                                 max_matches, ctypes.byref(res)))
        return int(res.count), xy[:res.returned], int(res.rows_searched)

    def find(self, pattern, care=None, border: int = 0, x: int = 0, y: int = 0, w: int | None = None,
             h: int | None = None, max_matches: int = 65536) -> dict:
        """Every occurrence of a pattern, searched on the device (gol_find):
        {"count": n, "matches": int64 [m][2] of (x, y), "rows_searched": r}.
        `pattern`, `care` and `border` as patterns.as_search takes them
        (border=1: the object standing alone).  (x, y, w, h) is a window of
        anchors -- the board cells under the pattern's top-left cell -- with
        density()'s defaults; the pattern may reach past it, wrapping on a
        torus and reading dead beyond a clipped board.  `count` is exact;
        `matches` holds min(count, max_matches) of them in global
        coordinates, sorted by (y, x).  A shard of a larger board examines only
        the anchors whose pattern lies in its own rows (ShardGroup.find
        completes the rest)."""
        cells, mask = patterns.as_search(pattern, care, border)
        w, h = _density_window(self, x, y, w, h)
        n, xy, rows = self._find_raw(cells, mask, x, y, w, h, max_matches)
        return {"count": n, "matches": xy, "rows_searched": rows}

    def checkpoint(self) -> np.ndarray:
        """gol_checkpoint into a new uint8 array (a bytes-like buffer: file
        writes, parse_checkpoint and restore take it as is).  No zero-fill and
        no bytes copy: at 0.5 GiB per shard that was ~0.3 s per checkpoint."""
        n = self.checkpoint_bytes()
        out = np.empty(n, dtype=np.uint8)
        self._chk(N.lib.gol_checkpoint(self._h, out.ctypes.data_as(ctypes.c_void_p), n))
        return out

    def checkpoint_bytes(self) -> int:
        n = ctypes.c_size_t(0)
        self._chk(N.lib.gol_checkpoint_bytes(self._h, ctypes.byref(n)))
        return n.value

    def checkpoint_async(self, out: np.ndarray) -> None:
        """Start a checkpoint into `out` (uint8, checkpoint_bytes() long; a
        page-locked one from host_array keeps the call from blocking); finish
        it with snapshot_wait()."""
        if out.dtype != np.uint8 or out.size < self.checkpoint_bytes() or not out.flags.c_contiguous:
            raise ValueError("checkpoint buffer must be a C-contiguous uint8 array of checkpoint_bytes()")
        self._chk(N.lib.gol_checkpoint_async(self._h, out.ctypes.data_as(ctypes.c_void_p), out.size))
        self._snap_out = out

    def restore(self, blob) -> None:
        """Restore a checkpoint (bytes, or any buffer such as a uint8 array)."""
        arr = np.frombuffer(blob, dtype=np.uint8)
        self._chk(N.lib.gol_restore(self._h, arr.ctypes.data_as(ctypes.c_void_p), arr.size))

    # -- multi-GPU -----------------------------------------------------------
    def comm_init(self, uid: bytes, rank: int, nranks: int) -> None:
        arr = (ctypes.c_uint8 * N.GOL_UNIQUE_ID_BYTES).from_buffer_copy(uid)
        self._chk(N.lib.gol_comm_init(self._h, arr, rank, nranks))

    def comm_init_loopback(self, key: str, rank: int, nranks: int) -> None:
        """Join the in-process loopback ring `key` (gol_comm_init_loopback, a
        test transport running the RCCL schedule's exact halo operations
        between contexts of this process, one thread each)."""
        self._chk(N.lib.gol_comm_init_loopback(self._h, key.encode(), rank, nranks))

    def comm_abort(self) -> None:
        """Leave the ring (gol_comm_abort); comm_init may join a new one."""
        self._chk(N.lib.gol_comm_abort(self._h))

    def replay(self, generations: int, above: np.ndarray, below: np.ndarray, hashes: bool = True):
        """Light-cone replay (gol_replay): advance this shard `generations`
        generations alone from the `generations` rows above and below it at
        its current epoch.  Returns the shard's per-generation partial hashes."""
        a = np.ascontiguousarray(above, dtype=np.uint32)
        b = np.ascontiguousarray(below, dtype=np.uint32)
        if a.shape != (generations, self.wwords) or b.shape != a.shape:
            raise ValueError(f"light-cone rows must be ({generations}, {self.wwords}) arrays")
        out = np.zeros(generations, dtype=np.uint64) if hashes else None
        self._chk(N.lib.gol_replay(self._h, generations, a.ctypes.data_as(N._u32p), b.ctypes.data_as(N._u32p),
                                   self.wwords, out.ctypes.data_as(N._u64p) if hashes else None))
        return out

    def allreduce_u64(self, values: np.ndarray) -> np.ndarray:
        v = np.ascontiguousarray(values, dtype=np.uint64).copy()
        self._chk(N.lib.gol_comm_allreduce_u64(self._h, v.ctypes.data_as(N._u64p), v.size))
        return v

    # -- timing / tuning -----------------------------------------------------
    def profile(self, enable: bool = True) -> None:
        self._chk(N.lib.gol_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self) -> tuple[float, int, int]:
        """(kernel ms, launches, generations advanced by those launches)."""
        ms, n, g = ctypes.c_double(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._chk(N.lib.gol_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(g)))
        return ms.value, n.value, g.value

    def profile_reset(self) -> None:
        self._chk(N.lib.gol_profile_reset(self._h))

    def profile_clock(self) -> float:
        """GHz the GPU held during the profiled launches since the reset
        (in-kernel clock probe, gol_profile_clock); 0.0 if none."""
        g = ctypes.c_double(0)
        self._chk(N.lib.gol_profile_clock(self._h, ctypes.byref(g)))
        return g.value

    def profile_stats(self) -> dict:
        """gol_profile_stats_read: the profiled passes since the reset split
        into the dominant launch, the halo exchange on the comm stream and the
        boundary launches, with the halo bytes posted to the ring."""
        st = N.GolProfileStats()
        self._chk(N.lib.gol_profile_stats_read(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in N.GolProfileStats._fields_}

    def occupancy(self, gens_per_pass: int) -> tuple[int, int]:
        """(resident waves per CU, strip width in words) of a G-generation pass."""
        w, s = ctypes.c_int32(0), ctypes.c_int32(0)
        self._chk(N.lib.gol_occupancy(self._h, gens_per_pass, ctypes.byref(w), ctypes.byref(s)))
        return w.value, s.value

    def pass_plan(self, generations: int, hashes: bool = False) -> list[int]:
        """Pass depths gol_step would use for `generations` (<= 1024) generations."""
        buf = (ctypes.c_int32 * max(generations, 1))()
        n = ctypes.c_int32(0)
        self._chk(N.lib.gol_pass_plan(self._h, generations, int(hashes), buf, len(buf), ctypes.byref(n)))
        return list(buf[:n.value])

    def set_tuning(self, band_rows: int = 0, gens_per_pass: int = 0, words_per_lane: int = 0) -> None:
        """Performance knobs only (gol_set_tuning): rows per band, generations
        per HBM pass (1..12), words per lane (1/2/4, 0 = auto)."""
        self._chk(N.lib.gol_set_tuning(self._h, band_rows, gens_per_pass, words_per_lane))

    def set_active_rows(self, enable: bool = True) -> None:
        """Active-row stepping (gol_set_active_rows): step only the row runs
        that can hold a live cell.  A performance knob: results never depend
        on it.  With it on, an unhashed step() may wait for a device scan."""
        self._chk(N.lib.gol_set_active_rows(self._h, 1 if enable else 0))

    def active_stats(self, reset: bool = False) -> dict:
        """gol_active_stats_read: passes run with the mode on, how many of
        them stepped row runs, and the rows stepped, cleared and scanned."""
        st = N.GolActiveStats()
        self._chk(N.lib.gol_active_stats_read(self._h, ctypes.byref(st), 1 if reset else 0))
        return {k: getattr(st, k) for k, _ in N.GolActiveStats._fields_}

    def active_rows(self) -> list[tuple[int, int]] | None:
        """The runs [lo, hi) of global rows outside which the current board is
        known dead (gol_active_rows); None when nothing is known."""
        n = ctypes.c_int32(0)
        self._chk(N.lib.gol_active_rows(self._h, None, 0, ctypes.byref(n)))
        if n.value < 0:
            return None
        buf = (ctypes.c_int64 * (2 * max(n.value, 1)))()
        self._chk(N.lib.gol_active_rows(self._h, buf, n.value, ctypes.byref(n)))
        return [(buf[2 * k], buf[2 * k + 1]) for k in range(n.value)]


class ShardGroup:
    """In-process group of shard engines of one board (gol_group_*): stepped
    in lockstep with device-to-device halo copies.  Engines must be given in
    row order and cover the board; they stay owned by the caller."""

    def __init__(self, shards: list[GolEngine]):
        self.shards = list(shards)
        arr = (ctypes.c_void_p * len(shards))(*[s._h.value for s in shards])
        h = ctypes.c_void_p()
        N.check(N.lib.gol_group_create(ctypes.byref(h), arr, len(shards)))
        self._h = h

    def _chk(self, rc: int) -> None:
        if rc != N.GOL_OK:
            raise N.GolError(rc, (N.lib.gol_group_last_error(self._h) or b"").decode())

    def step(self, generations: int = 1, hashes: bool = False, partials: bool = False, populations: bool = False):
        """Advance every shard; returns the global per-generation hashes if
        asked, and with partials=True also every shard's partials as a
        (shards, generations) array (gol_group_step_partials).
        populations=True: the board's per-generation populations
        (gol_group_step_series), or (hashes, populations) when both are asked;
        not together with partials."""
        if partials and populations:
            raise ValueError("ShardGroup.step: partials and populations cannot be asked together")
        if populations:
            pop = np.zeros(generations, dtype=np.uint64)
            out = np.zeros(generations, dtype=np.uint64) if hashes else None
            self._chk(N.lib.gol_group_step_series(self._h, generations,
                                                  out.ctypes.data_as(N._u64p) if hashes else None,
                                                  pop.ctypes.data_as(N._u64p), pop.size))
            return (out, pop) if hashes else pop
        if partials:
            out = np.zeros(generations, dtype=np.uint64)
            part = np.zeros((len(self.shards), generations), dtype=np.uint64)
            self._chk(N.lib.gol_group_step_partials(self._h, generations, out.ctypes.data_as(N._u64p),
                                                    part.ctypes.data_as(N._u64p)))
            return out, part
        if hashes:
            out = np.zeros(generations, dtype=np.uint64)
            self._chk(N.lib.gol_group_step(self._h, generations, out.ctypes.data_as(N._u64p)))
            return out
        self._chk(N.lib.gol_group_step(self._h, generations, None))
        return None

    def sync(self) -> None:
        self._chk(N.lib.gol_group_sync(self._h))

    @property
    def epoch(self) -> int:
        return self.shards[0].epoch

    def snapshot(self) -> np.ndarray:
        return np.vstack([s.snapshot() for s in self.shards])

    # -- patterns, windows and census: the same call on every shard ----------
    def census(self) -> dict:
        """The board's census: populations summed, boxes combined by min / max."""
        raw = [s._census_raw() for s in self.shards]
        return _census_dict(sum(r[0] for r in raw), min(r[1] for r in raw), max(r[2] for r in raw),
                            min(r[3] for r in raw), max(r[4] for r in raw))

    def population(self) -> int:
        return sum(s._census_raw()[0] for s in self.shards)

    def read_region(self, x: int, y: int, w: int, h: int) -> np.ndarray:
        """The window, each shard filling the rows it owns of one buffer."""
        packed = _window_buffer(w, h)
        for s in self.shards:
            s._read_region_into(x, y, w, h, packed)
        return codec.unpack(packed, w)

    def write_region(self, x: int, y: int, cells, mode: str = "copy") -> None:
        c = patterns.as_cells(cells)
        packed = codec.pack(c)
        for s in self.shards:
            s._write_region_packed(x, y, c.shape[1], c.shape[0], packed, mode)

    def set_cell(self, x: int, y: int, alive: bool = True) -> None:
        self.write_region(x, y, np.ones((1, 1), dtype=np.uint8), "or" if alive else "clear")

    def place(self, pattern, x: int, y: int, mode: str = "or") -> None:
        self.write_region(x, y, patterns.as_cells(pattern), mode)

    def density(self, tile: int, x: int = 0, y: int = 0, w: int | None = None, h: int | None = None) -> np.ndarray:
        """The board's density map (GolEngine.density): every shard adds the
        cells of its own rows to one zeroed buffer."""
        lg = _log2_tile(tile)
        w, h = _density_window(self.shards[0], x, y, w, h)
        counts = _density_buffer(w, h, lg)
        for s in self.shards:
            s._density_into(x, y, w, h, lg, counts)
        return counts

    def _band(self, x: int, y: int, w: int, h: int) -> np.ndarray:
        """Board cells (x + j, y + i), j < w, i < h, with y inside the board:
        wrapped on a torus (however often), dead beyond a clipped board."""
        e = self.shards[0]
        if e.topology == "torus":
            base = self.read_region(x % e.width, y, min(w, e.width), min(h, e.height))
            return base[np.arange(h) % base.shape[0]][:, np.arange(w) % base.shape[1]]
        band = np.zeros((h, w), dtype=np.uint8)
        sw, sh = min(w, e.width - x), min(h, e.height - y)
        if sw > 0 and sh > 0:
            band[:sh, :sw] = self.read_region(x, y, sw, sh)
        return band

    def find(self, pattern, care=None, border: int = 0, x: int = 0, y: int = 0, w: int | None = None,
             h: int | None = None, max_matches: int = 65536) -> dict:
        """The board's matches (GolEngine.find): the same search on every
        shard, the counts summed, the matches merged and sorted.  The anchors
        no shard examines -- those of the window in the last ph - 1 rows above
        a shard boundary (the torus seam between the last and the first shard
        included), whose pattern straddles it -- are matched here on the host,
        in the band of rows around the boundary read with read_region."""
        cells, mask = patterns.as_search(pattern, care, border)
        ph, pw = cells.shape
        e0 = self.shards[0]
        torus = e0.topology == "torus"
        w, h = _density_window(e0, x, y, w, h)
        count = rows = 0
        found = []
        for s in self.shards:
            n, xy, r = s._find_raw(cells, mask, x, y, w, h, max_matches)
            count, rows = count + n, rows + r
            found.append(xy)
        for s in self.shards:
            end = s.row0 + s.rows
            if ph == 1 or (s.rows == e0.height if torus else end == e0.height):
                continue  # the shard examines every anchor row it owns
            first = max(s.row0, end - (ph - 1))  # its anchor rows [first, end) were left out
            ys = np.arange(first, end)
            ys = ys[((ys - y) % e0.height < h) if torus else ((ys >= y) & (ys < y + h))]
            if not ys.size:
                continue
            band = self._band(x, first, w + pw - 1, end - first + ph - 1)
            hit = patterns.match_band(band, cells, mask)[ys - first]
            j, i = np.nonzero(hit)
            xs = (x + i) % e0.width if torus else x + i
            count += int(j.size)
            found.append(np.stack([xs, ys[j]], axis=1).astype(np.int64).reshape(-1, 2))
        xy = np.concatenate(found) if found else np.zeros((0, 2), dtype=np.int64)
        xy = xy[np.lexsort((xy[:, 0], xy[:, 1]))][:max(int(max_matches), 0)]
        return {"count": count, "matches": xy, "rows_searched": rows}

    def hash(self) -> int:
        """The board's state hash: the shards' partials summed mod 2^64."""
        return sum(s.hash() for s in self.shards) & 0xFFFFFFFFFFFFFFFF

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib.gol_group_destroy(self._h)
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


def _census_dict(population: int, min_x: int, max_x: int, min_y: int, max_y: int) -> dict:
    bbox = (min_x, min_y, max_x, max_y) if population else None
    return {"population": int(population), "bbox": bbox}


def _window_buffer(w: int, h: int) -> np.ndarray:
    """A zeroed packed buffer for a w x h window (gol_read_region fills the
    rows a shard owns and leaves the others as they are)."""
    return np.zeros((max(int(h), 1), max(codec.words_per_row(int(w)), 1)), dtype=np.uint32)


def _log2_tile(tile: int) -> int:
    """log2 of a density tile edge; ValueError unless it is a power of two
    from 1 to 32768 (gol_density's log2_tile 0 .. 15)."""
    if not isinstance(tile, (int, np.integer)) or isinstance(tile, bool) or not 1 <= tile <= 32768 or tile & (tile - 1):
        raise ValueError(f"tile must be a power of two from 1 to 32768, not {tile!r}")
    return int(tile).bit_length() - 1


def _density_window(e: GolEngine, x: int, y: int, w: int | None, h: int | None) -> tuple[int, int]:
    torus = e.topology == "torus"
    return (int((e.width if torus else e.width - x) if w is None else w),
            int((e.height if torus else e.height - y) if h is None else h))


def _density_buffer(w: int, h: int, log2_tile: int) -> np.ndarray:
    """A zeroed [th][tw] map for a w x h window (gol_density adds to it)."""
    t = 1 << log2_tile
    return np.zeros((max(-(-h // t), 1), max(-(-w // t), 1)), dtype=np.uint32)


class _HostBlock:
    """Owner of one gol_host_alloc block; freed when the last array viewing
    it is garbage-collected."""

    def __init__(self, nbytes: int):
        self.ptr = ctypes.c_void_p()
        N.check(N.lib.gol_host_alloc(nbytes, ctypes.byref(self.ptr)))

    def __del__(self):
        try:
            if getattr(self, "ptr", None) is not None and self.ptr.value:
                N.lib.gol_host_free(self.ptr)
                self.ptr = None
        except Exception:  # interpreter shutdown: the library may be gone already
            pass


def host_array(shape, dtype=np.uint32) -> np.ndarray:
    """A numpy array over page-locked host memory (gol_host_alloc); the block
    is freed when the array (and every view of it) is garbage-collected."""
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dt.itemsize
    block = _HostBlock(max(1, nbytes))
    buf = (ctypes.c_char * max(1, nbytes)).from_address(block.ptr.value)
    buf._gol_block = block  # array -> buf -> block
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def selftest(device: int = 0) -> np.ndarray:
    rep = np.zeros(256, dtype=np.uint32)
    N.check(N.lib.gol_selftest(device, rep.ctypes.data_as(N._u32p)))
    return rep
