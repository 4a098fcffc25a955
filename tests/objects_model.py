"""Cell-level model of the objects of a batch's boards (gol_objects_batch;
DESIGN.md section 5i) -- test infrastructure, independent of the package's
own labeller: objects by a breadth-first search over the links, boxes by
listing the cyclic runs of empty columns, the hash batch_model.board_hash (the
C oracle's) of the translated cells, order and truncation as the contract
states them."""
from collections import deque

import numpy as np

import batch_model as M
from gameoflife.patterns import OBJECT_DTYPE


def components(cells, torus, reach):
    """The objects of one uint8 [H][W] board as lists of (x, y), each in the
    order its cells were reached, the objects by their first cell in row-major
    order."""
    c = np.asarray(cells) != 0
    H, W = c.shape
    seen = np.zeros_like(c)
    out = []
    for y0 in range(H):
        for x0 in range(W):
            if not c[y0, x0] or seen[y0, x0]:
                continue
            seen[y0, x0] = True
            todo, obj = deque([(x0, y0)]), []
            while todo:
                x, y = todo.popleft()
                obj.append((x, y))
                for dy in range(-reach, reach + 1):
                    for dx in range(-reach, reach + 1):
                        nx, ny = x + dx, y + dy
                        if torus:
                            nx, ny = nx % W, ny % H
                        elif not (0 <= nx < W and 0 <= ny < H):
                            continue
                        if c[ny, nx] and not seen[ny, nx]:
                            seen[ny, nx] = True
                            todo.append((nx, ny))
            out.append(obj)
    return out


def empty_runs(occupied, n):
    """The maximal cyclic runs of positions of 0 .. n - 1 not in `occupied` as (first, length)."""
    occ = set(occupied)
    if not occ:
        return [(0, n)]
    runs = []
    for p in range(n):
        if p not in occ and (p - 1) % n in occ:
            length = 1
            while (p + length) % n not in occ:
                length += 1
            runs.append((p, length))
    return runs


def span(occupied, n, torus, reach):
    """(start, extent) on one axis by the contract's rule; at most one run of at least `reach` may exist."""
    if not torus:
        return min(occupied), max(occupied) - min(occupied) + 1
    gaps = [(p, k) for p, k in empty_runs(occupied, n) if k >= reach]
    assert len(gaps) <= 1, ("an object with two gaps", sorted(set(occupied)), n, reach)
    if not gaps:
        return 0, n
    p, k = gaps[0]
    return (p + k) % n, n - k


def board_objects(cells, torus=True, reach=1):
    """OBJECT_DTYPE [n]: every object of one uint8 [H][W] board."""
    c = np.asarray(cells, dtype=np.uint8)
    H, W = c.shape
    objs = components(c, torus, reach)
    out = np.zeros(len(objs), dtype=OBJECT_DTYPE)
    for rec, obj in zip(out, objs):
        x, w = span([p[0] for p in obj], W, torus, reach)
        y, h = span([p[1] for p in obj], H, torus, reach)
        moved = np.zeros((H, W), dtype=np.uint8)
        for px, py in obj:
            moved[(py - y) % H, (px - x) % W] = 1
        rec["hash"] = M.board_hash(moved)
        rec["x"], rec["y"], rec["w"], rec["h"] = x, y, w, h
        rec["population"] = len(obj)
    return out


def batch_objects(rows, W, torus=True, reach=1, max_objects=64):
    """(counts uint32 [n], objects OBJECT_DTYPE [n][max_objects]) of uint64 [n][H] rows: what
    GolBatch.objects(reach, max_objects) returns for these boards."""
    boards = M.unpack(rows, W)
    counts = np.zeros(len(boards), dtype=np.uint32)
    objects = np.zeros((len(boards), max_objects), dtype=OBJECT_DTYPE)
    for b, cells in enumerate(boards):
        recs = board_objects(cells, torus, reach)
        counts[b] = len(recs)
        keep = min(len(recs), max_objects)
        objects[b, :keep] = recs[:keep]
    return counts, objects
