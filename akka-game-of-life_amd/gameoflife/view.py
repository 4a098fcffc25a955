"""Pictures of a density map (GolEngine.density / ShardGroup.density): the
LoggerActor's board print (LoggerActor.scala:30-46) at a scale where one
character or pixel stands for a tile x tile block of cells.  Pure numpy."""
from __future__ import annotations

import numpy as np

RAMP = " .:-=+*#%@"


def _levels(counts, tile: int, top: int) -> np.ndarray:
    """count / tile^2 mapped onto 0 .. top: 0 only for a count of 0, at least
    1 for any other, `top` for a full tile."""
    c = np.asarray(counts, dtype=np.uint64)
    if c.ndim != 2:
        raise ValueError(f"a density map is a [th][tw] array, not one of shape {c.shape}")
    if tile < 1:
        raise ValueError(f"tile must be positive, not {tile!r}")
    lv = np.minimum(c * np.uint64(top) // np.uint64(int(tile) ** 2), np.uint64(top)).astype(np.int64)
    return np.where(c > 0, np.maximum(lv, 1), 0)


def density_ascii(counts, tile: int, ramp: str = RAMP) -> list[str]:
    """One string per map row, one character per tile: the first character of
    `ramp` for an empty tile, the last one for a full tile, and at least the
    second for any tile with a live cell."""
    if len(ramp) < 2:
        raise ValueError("the ramp needs at least two characters")
    chars = np.array(list(ramp))
    return ["".join(row) for row in chars[_levels(counts, tile, len(ramp) - 1)]]


def density_pgm(counts, tile: int) -> bytes:
    """The map as a binary 8-bit PGM (P5, maxval 255): 0 for an empty tile,
    255 for a full one, at least 1 for any tile with a live cell."""
    lv = _levels(counts, tile, 255).astype(np.uint8)
    th, tw = lv.shape
    return b"P5\n%d %d\n255\n" % (tw, th) + lv.tobytes()
