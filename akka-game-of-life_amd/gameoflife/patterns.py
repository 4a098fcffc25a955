"""Life patterns as cell arrays: the run-length encoded (RLE) form pattern
collections publish, and the O/. row form of tests/known_patterns.py.

A pattern is a uint8 [h][w] array (1 = alive), the form GolEngine.place and
write_region take.  The reference draws its initial state at random
(BoardCreator.scala:23); a user who wants a glider gun at (x, y) starts here.
"""
from __future__ import annotations

import re
from typing import NamedTuple

import numpy as np


class Pattern(NamedTuple):
    cells: np.ndarray   # uint8 [height][width]
    width: int
    height: int
    rule: str | None    # the header's rule string, as written, if any


_HEADER = re.compile(r"^\s*x\s*=\s*(\d+)\s*,\s*y\s*=\s*(\d+)\s*(?:,\s*rule\s*=\s*(\S+)\s*)?$", re.I)
_TOKEN = re.compile(r"(\d*)([bo$!])")


def parse_rle(text: str) -> Pattern:
    """Parse an RLE pattern: `#` comment lines, an optional
    `x = .., y = .., rule = ..` header, then runs `<count><tag>` with tag b
    (dead), o (alive), $ (end of row; a count skips rows) and ! (end).  The
    header's extents size the array when present (the body must fit them);
    otherwise the body's own extents do.  Anything else raises ValueError."""
    width = height = None
    rule = None
    body = []
    for line in text.splitlines():
        s = line.strip()
        if not s or s.startswith("#"):
            continue
        if not body and width is None:
            m = _HEADER.match(s)
            if m:
                width, height, rule = int(m.group(1)), int(m.group(2)), m.group(3)
                continue
        body.append(s)
    data = "".join("".join(body).split())
    end = data.find("!")
    if end >= 0:
        data = data[:end + 1]
    live = []          # (x, y) of live cells
    x = y = 0
    xmax = 0           # widest row, dead runs included
    pos = 0
    while pos < len(data):
        m = _TOKEN.match(data, pos)
        if not m:
            raise ValueError(f"RLE: unexpected {data[pos:pos + 8]!r} at offset {pos}")
        pos = m.end()
        n = int(m.group(1)) if m.group(1) else 1
        tag = m.group(2)
        if n == 0:
            raise ValueError("RLE: zero run count")
        if tag == "b":
            x += n
        elif tag == "o":
            live.extend((x + k, y) for k in range(n))
            x += n
        elif tag == "$":
            xmax = max(xmax, x)
            x = 0
            y += n
        else:  # "!"
            if m.group(1):
                raise ValueError("RLE: a run count before '!'")
            break
    xmax = max(xmax, x)
    rows = y + 1
    if width is None:
        width, height = max(xmax, 1), rows
    elif xmax > width or any(cy >= height for _, cy in live):
        raise ValueError(f"RLE: the body does not fit the header's {width} x {height}")
    if width < 1 or height < 1:
        raise ValueError("RLE: empty extents")
    cells = np.zeros((height, width), dtype=np.uint8)
    for cx, cy in live:
        cells[cy, cx] = 1
    return Pattern(cells, width, height, rule)


def to_rle(cells, rule: str | None = "B3/S23") -> str:
    """RLE text of a cell array, with the header that restores its extents
    (trailing dead columns and rows are not written in the body)."""
    c = np.asarray(cells, dtype=np.uint8) & 1
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError("to_rle takes a non-empty [h][w] cell array")
    h, w = c.shape
    tokens = []
    pending = 0  # row ends not yet written
    for row in c:
        alive = np.flatnonzero(row)
        if alive.size:
            if pending:
                tokens.append(("$", pending))
                pending = 0
            r = row[:alive[-1] + 1]
            cuts = np.flatnonzero(np.diff(r)) + 1
            for seg in np.split(r, cuts):
                tokens.append(("o" if seg[0] else "b", len(seg)))
        pending += 1
    out = [f"x = {w}, y = {h}" + (f", rule = {rule}" if rule else "")]
    line = ""
    for tag, n in tokens + [("!", 1)]:
        t = (str(n) if n > 1 else "") + tag
        if len(line) + len(t) > 70:
            out.append(line)
            line = ""
        line += t
    out.append(line)
    return "\n".join(out) + "\n"


def from_rows(rows) -> np.ndarray:
    """Cell array of a list of strings, `O` alive and `.` dead (short rows are
    padded with dead cells)."""
    rows = list(rows)
    if not rows:
        raise ValueError("from_rows takes at least one row")
    w = max(max(len(r) for r in rows), 1)
    cells = np.zeros((len(rows), w), dtype=np.uint8)
    for y, r in enumerate(rows):
        for x, ch in enumerate(r):
            if ch == "O":
                cells[y, x] = 1
            elif ch != ".":
                raise ValueError(f"from_rows: unexpected {ch!r} in row {y}")
    return cells


def as_cells(pattern) -> np.ndarray:
    """A pattern in any accepted form -- RLE text, a list of O/. rows, a
    Pattern, or a cell array -- as a uint8 [h][w] array."""
    if isinstance(pattern, Pattern):
        return pattern.cells
    if isinstance(pattern, str):
        return parse_rle(pattern).cells
    if isinstance(pattern, (list, tuple)) and pattern and all(isinstance(r, str) for r in pattern):
        return from_rows(pattern)
    c = np.asarray(pattern, dtype=np.uint8) & 1
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError("a pattern is a non-empty [h][w] cell array")
    return c


SEARCH_MAX = 64  # gol_find: a pattern of at most 64 x 64 cells, border included


def as_search(pattern, care=None, border: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """A pattern to search for (GolEngine.find) as (cells, care): two uint8
    [h][w] arrays, care 1 where the board must equal the pattern and 0 where
    anything goes.  `pattern` is any form as_cells takes; a list of rows may
    also use `?` for a cell that is not cared for.  `care` (optional) is a cell
    array of the pattern's shape.  border=n surrounds the pattern with n rings
    of cared dead cells: the search for the object standing alone.  ValueError
    for a result outside 64 x 64, a care array of another shape and a pattern
    with no cared cell."""
    asked = None
    if isinstance(pattern, (list, tuple)) and pattern and all(isinstance(r, str) for r in pattern):
        rows = list(pattern)
        cells = from_rows([r.replace("?", ".") for r in rows])
        asked = np.ones_like(cells)
        for y, r in enumerate(rows):
            for x, ch in enumerate(r):
                if ch == "?":
                    asked[y, x] = 0
    else:
        cells = as_cells(pattern)
    if care is not None:
        c = np.asarray(care)
        if c.shape != cells.shape:
            raise ValueError(f"the care mask's shape {c.shape} is not the pattern's {cells.shape}")
        c = (c != 0).astype(np.uint8)
        asked = c if asked is None else asked & c
    if asked is None:
        asked = np.ones_like(cells)
    if not isinstance(border, (int, np.integer)) or isinstance(border, bool) or border < 0:
        raise ValueError(f"border must be a ring count >= 0, not {border!r}")
    if border:
        cells = np.pad(cells, border, constant_values=0)
        asked = np.pad(asked, border, constant_values=1)
    if cells.shape[0] > SEARCH_MAX or cells.shape[1] > SEARCH_MAX:
        raise ValueError(f"a search pattern is at most {SEARCH_MAX} x {SEARCH_MAX} cells, border included; "
                         f"this one is {cells.shape[1]} x {cells.shape[0]}")
    if not asked.any():
        raise ValueError("the search pattern cares for no cell")
    return np.ascontiguousarray(cells & asked, dtype=np.uint8), np.ascontiguousarray(asked, dtype=np.uint8)


def orientations(cells, care=None) -> list[tuple[np.ndarray, np.ndarray]]:
    """The distinct images of a search pattern under the 8 symmetries of the
    square (4 rotations, each also mirrored), as (cells, care) pairs of uint8
    arrays in the order they are first met, the pattern itself first.  `care`
    (default: every cell) turns with the cells; two images are the same when
    their shapes, care masks and cared cells are equal.  A block has 1, a
    blinker 2, a glider 8.  Turning commutes with as_search's border."""
    c = np.asarray(cells, dtype=np.uint8) & 1
    m = np.ones_like(c) if care is None else (np.asarray(care) != 0).astype(np.uint8)
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1 or m.shape != c.shape:
        raise ValueError("orientations takes a non-empty [h][w] cell array and a care mask of its shape")
    c = c & m
    out, seen = [], set()
    for flip in (False, True):
        fc, fm = (c[:, ::-1], m[:, ::-1]) if flip else (c, m)
        for turns in range(4):
            ic = np.ascontiguousarray(np.rot90(fc, turns))
            im = np.ascontiguousarray(np.rot90(fm, turns))
            key = (ic.shape, ic.tobytes(), im.tobytes())
            if key not in seen:
                seen.add(key)
                out.append((ic, im))
    return out


def match_band(band, cells, care) -> np.ndarray:
    """Host matcher for the few anchors a device search leaves to its caller
    (ShardGroup.find): bool [bh - ph + 1][bw - pw + 1], entry (j, i) true iff
    the [bh][bw] cell array `band` equals the pattern at its rows j .. j + ph - 1
    and columns i .. i + pw - 1 in every cared cell.  The caller has wrapped or
    padded the band."""
    band = np.asarray(band, dtype=np.uint8)
    ph, pw = cells.shape
    nh, nw = band.shape[0] - ph + 1, band.shape[1] - pw + 1
    if nh < 1 or nw < 1:
        return np.zeros((max(nh, 0), max(nw, 0)), dtype=bool)
    ok = np.ones((nh, nw), dtype=bool)
    for i, k in zip(*np.nonzero(care)):
        ok &= band[i:i + nh, k:k + nw] == cells[i, k]
    return ok


# ---------------------------------------------------------------- objects
# gol_batch_object (include/gol.h) as a numpy record: what GolBatch.objects
# returns and label_objects computes on the host
OBJECT_DTYPE = np.dtype([("hash", "<u8"), ("x", "u1"), ("y", "u1"), ("w", "u1"), ("h", "u1"),
                         ("population", "<u2"), ("reserved", "<u2")])

_M32 = np.uint64(0xFFFFFFFF)


def _hash_cells(c: np.ndarray) -> int:
    """The state hash (DESIGN.md section 5, row0 = 0) of a uint8 [h][w] cell
    array as it stands: per row y and column group g (columns 64 g ..
    64 g + 63) the words E (even columns) and O (odd columns) contribute
    (E A(y, 0) + O A(y, 1)) B(g) modulo 2^64."""
    h, w = c.shape
    groups = (w + 63) // 64
    bits = np.zeros((h, groups * 64), dtype=np.uint64)
    bits[:, :w] = c != 0
    bits = bits.reshape(h, groups, 32, 2)
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    even = (bits[..., 0] * weights).sum(axis=2, dtype=np.uint64)
    odd = (bits[..., 1] * weights).sum(axis=2, dtype=np.uint64)
    with np.errstate(over="ignore"):
        t = (np.arange(h, dtype=np.uint64) * np.uint64(0x9E3779B1)) & _M32
        a0 = (((t ^ (t >> np.uint64(15))) << np.uint64(1)) | np.uint64(1)) & _M32
        a1 = (a0 + np.uint64(0x6A09E666)) & _M32
        k = (np.arange(groups, dtype=np.uint64) + np.uint64(0x7F4A7C15)) & _M32
        k ^= k >> np.uint64(16)
        k = (k * np.uint64(0x85EBCA6B)) & _M32
        k ^= k >> np.uint64(13)
        k = (k * np.uint64(0xC2B2AE35)) & _M32
        k ^= k >> np.uint64(16)
        k |= np.uint64(1)
        terms = (even * a0[:, None] + odd * a1[:, None]) * k[None, :]
        return int(terms.sum(dtype=np.uint64))


def _trimmed(pattern) -> np.ndarray:
    """A pattern's cells without its dead outer rows and columns ([0][0] if none lives)."""
    c = as_cells(pattern)
    ys, xs = np.nonzero(c)
    if ys.size == 0:
        return np.zeros((0, 0), dtype=np.uint8)
    return c[ys.min():ys.max() + 1, xs.min():xs.max() + 1]


def object_hash(pattern) -> int:
    """The key GolBatch.objects gives an object with these cells: the state
    hash of the pattern with the corner of its bounding box at cell (0, 0)
    (what GolBatch.hashes / GolEngine.hash() return for a board holding only
    it there, whatever the board's size).  `pattern` is any form as_cells
    takes; dead outer rows and columns do not count."""
    return _hash_cells(_trimmed(pattern))


def _axis_span(occupied: np.ndarray, torus: bool, reach: int) -> tuple[int, int]:
    """(start, extent) of an object on one axis from its occupied positions
    (bool [n], some true).  Clipped: minimum and maximum.  Torus: the box
    starts at the one occupied position whose `reach` cyclic predecessors are
    all empty and ends at the last occupied one before that gap; without such
    a position the object goes round the axis: (0, n)."""
    n = occupied.size
    if not torus:
        at = np.flatnonzero(occupied)
        return int(at[0]), int(at[-1] - at[0] + 1)
    start = occupied.copy()
    for k in range(1, reach + 1):
        start &= ~np.roll(occupied, k)
    at = np.flatnonzero(start)
    if at.size == 0:
        return 0, n
    s = int(at[0])
    return s, int(np.flatnonzero(np.roll(occupied, -s))[-1]) + 1


def label_objects(cells, torus: bool = True, reach: int = 1) -> np.ndarray:
    """The objects of one uint8 [H][W] board (H, W <= 64) on the host: the
    records GolBatch.objects gives for it (OBJECT_DTYPE [n], every object, in
    its order).  Two live cells are linked iff their Chebyshev distance, cyclic
    on a torus, is at most `reach` (1 or 2); an object is a connected
    component.  Labels spread as minima: every live cell starts with its
    row-major index and takes the smallest label within `reach` until nothing
    changes, so an object's label is its first cell and sorting the labels
    gives the order."""
    c = np.asarray(cells) != 0
    if c.ndim != 2 or not 1 <= c.shape[0] <= 64 or not 1 <= c.shape[1] <= 64:
        raise ValueError(f"label_objects takes one [H][W] board of at most 64 x 64 cells, not {c.shape}")
    if reach not in (1, 2):
        raise ValueError(f"reach must be 1 or 2, not {reach!r}")
    H, W = c.shape
    none = H * W

    def shifted(a, s, axis):  # a moved by s along axis; clipped: `none` comes in
        if torus:
            return np.roll(a, s, axis)
        out = np.full_like(a, none)
        src = [slice(None)] * 2
        dst = [slice(None)] * 2
        src[axis] = slice(0, a.shape[axis] - s) if s > 0 else slice(-s, None)
        dst[axis] = slice(s, None) if s > 0 else slice(0, a.shape[axis] + s)
        out[tuple(dst)] = a[tuple(src)]
        return out

    lab = np.where(c, np.arange(none, dtype=np.int32).reshape(H, W), none).astype(np.int32)
    while True:
        m = lab
        for axis in (0, 1):  # the square window, an axis at a time
            acc = m
            for d in range(1, min(reach, m.shape[axis] - 1) + 1):
                acc = np.minimum(acc, np.minimum(shifted(m, d, axis), shifted(m, -d, axis)))
            m = acc
        m = np.where(c, m, none)
        if np.array_equal(m, lab):
            break
        lab = m
    labels = np.unique(lab[c])
    out = np.zeros(labels.size, dtype=OBJECT_DTYPE)
    for rec, label in zip(out, labels):
        own = lab == label
        x, w = _axis_span(own.any(axis=0), torus, reach)
        y, h = _axis_span(own.any(axis=1), torus, reach)
        moved = np.roll(own, (-y, -x), (0, 1))  # plain on a clipped board: nothing of the object is before its corner
        rec["hash"] = _hash_cells(moved)
        rec["x"], rec["y"], rec["w"], rec["h"] = x, y, w, h
        rec["population"] = int(own.sum())
    return out


def object_table(named) -> dict:
    """{name: [pattern, ...]} -> {(hash, w, h, population): name}: the keys of
    GolBatch.objects' records for every distinct orientation (orientations) of
    every listed image, for batch.tally.  The caller lists an oscillator's
    phases.  ValueError if two names claim one key."""
    table: dict = {}
    for name, images in named.items():
        for image in images:
            for cells, _ in orientations(_trimmed(image)):
                key = (object_hash(cells), cells.shape[1], cells.shape[0], int(cells.sum()))
                if table.setdefault(key, name) != name:
                    raise ValueError(f"{name!r} and {table[key]!r} share an image")
    return table
