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
