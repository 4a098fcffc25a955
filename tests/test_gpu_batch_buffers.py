"""GPU: the device buffers of one batch handle grown, reused and released in an
order no feature test walks (gol_batch.cpp's buffer owners; DESIGN.md sections
5f to 5k).  One batch of 10 boards of 8 x 7 -- 9 boards per wave, so a full
wave and a wave of one board -- goes through every entry point that allocates
on demand, each twice or three times with another size, and every result is
the CPU models'.  A second batch stops half way, so a handle is destroyed with
every buffer allocated and one with only some."""
import functools
import types

import numpy as np
import pytest

import batch_find_model as FM
import batch_model as M
import batch_rules_model as RM
import census_model as CM
import cycle_model as CY
import objects_model as OM
from gameoflife import _native as N
from gameoflife import patterns as P
from gameoflife.batch import GolBatch
from gameoflife.rules import rule_word

pytestmark = pytest.mark.gpu

BOARDS, W, H, SEED = 10, 8, 7, 0x5EED
FIRST, PART = 6, 4            # the boards that take rules of their own: 6 .. 9, some of either wave
NO_MATCH = [["OOOOO"] * 5]    # a 5 x 5 square of live cells: no soup holds one after 16 generations
MATCHING = [["O"], ["."], ["O.", ".O"]]
CYCLE_GENS = 40
ZEROS = {"calls": 0, "seen": 0, "tallied": 0, "truncated": 0, "overflowed": 0, "distinct": 0}


def _find_model(rows, patterns):
    """(counts uint32 [boards][P], planes uint64 [P][boards][H]): what find(patterns, matches=True) returns."""
    planes = np.stack([FM.match_rows(rows, W, *P.as_search(pat), True) for pat in patterns])
    return np.stack([FM.counts(p) for p in planes], axis=1), planes


def _cycles_model(rows, words):
    """Board i advanced CYCLE_GENS generations under words[i]: (final rows, period, seen)."""
    out = [CY.run_board(c, CYCLE_GENS, "torus", RM.masks(w)) for c, w in zip(M.unpack(rows, W), words)]
    return (M.pack(np.stack([o[0] for o in out])), np.array([o[1] for o in out], dtype=np.uint32),
            np.array([o[2] for o in out], dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def _reference():
    """Everything the walk compares with, computed once."""
    r = types.SimpleNamespace()
    r.seeded = M.seed_rows(BOARDS, W, H, SEED)
    r.after6, r.pops6, _ = M.run(r.seeded, W, 6)
    r.rows, r.pops10, _ = M.run(r.after6, W, 10)  # the boards of steps 2 to 5
    r.hashes = M.hashes(r.rows, W)
    r.populations = M.unpack(r.rows, W).sum(axis=(1, 2)).astype(np.uint32)
    r.none, r.some = _find_model(r.rows, NO_MATCH), _find_model(r.rows, MATCHING)
    assert not r.none[0].any() and r.some[0].any(axis=0).all()  # the patterns are what their names say
    r.objects1, r.objects8 = (OM.batch_objects(r.rows, W, True, 1, m) for m in (1, 8))
    assert (r.objects8[0] > 1).any()  # max_objects 1 truncates
    r.life = np.full(BOARDS, rule_word("life"), dtype=np.uint32)
    r.words = r.life.copy()
    r.words[FIRST:FIRST + PART] = RM.rule_words(BOARDS)[FIRST:FIRST + PART]
    r.cycles = [_cycles_model(r.rows, r.words)]
    r.cycles.append(_cycles_model(r.cycles[0][0], r.life))
    r.cycles.append(_cycles_model(r.cycles[1][0], r.words))
    return r


def _census(max_keys, objects):
    census = CM.Census(max_keys)
    census.add(*objects)
    return census


def _hashes(b, first, count):
    hashes, pops = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint32)
    b._chk(N.lib.gol_batch_hashes(b._h, first, count, hashes.ctypes.data_as(N._u64p), pops.ctypes.data_as(N._u32p)))
    return hashes, pops


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


def _walk(b, r, to_the_end):
    """Steps 1 to 6 on a fresh batch; to_the_end=False: stops after the first set_rules."""
    assert b.geometry() == {"boards_per_wave": 9, "waves": 2, "device_bytes": 2 * BOARDS * H * 8 + BOARDS * 4}
    b.seed(SEED)
    assert np.array_equal(b.snapshot(), r.seeded)
    # 1. the series buffer: [boards][2], then regrown to [boards][5]
    b.set_chunk(2)
    assert np.array_equal(b.step(6, populations=True), r.pops6) and np.array_equal(b.snapshot(), r.after6)
    b.set_chunk(5)
    assert np.array_equal(b.step(10, populations=True), r.pops10) and np.array_equal(b.snapshot(), r.rows)
    # 2. hashes of one board (the second wave's), then of all
    assert _same(_hashes(b, BOARDS - 1, 1), (r.hashes[-1:], r.populations[-1:]))
    assert _same(_hashes(b, 0, BOARDS), (r.hashes, r.populations))
    # 3. find: one pattern, three, one again in the buffers the three left
    assert _same(b.find(NO_MATCH, matches=True), r.none)
    assert _same(b.find(MATCHING, matches=True), r.some)
    assert _same(b.find(NO_MATCH, matches=True), r.none)
    # 4. objects: one record per board, then eight
    for max_objects, want in ((1, r.objects1), (8, r.objects8)):
        counts, objs = b.objects(reach=1, max_objects=max_objects)
        assert np.array_equal(counts, want[0]) and objs.tobytes() == want[1].tobytes()
    # 5. the census: a table of two slots, one of 128, two again
    for max_keys in (1, 64):
        b.census_begin(max_keys)
        assert b.census_add(reach=1, max_objects=8) == 0
        _census(max_keys, r.objects8).check(b.census_read(), b.census_stats())
    b.census_begin(1)
    assert b.census_stats() == ZEROS and len(b.census_read()) == 0
    # 6. rules for a part of the batch, for none of it, for the part again, a cycle step after each
    b.set_rules(r.words[FIRST:FIRST + PART], first=FIRST)
    assert np.array_equal(b.rules(), r.words) and np.array_equal(b.snapshot(), r.rows)
    if not to_the_end:
        return
    assert _same(b.step_cycles(CYCLE_GENS) + (b.snapshot(),), r.cycles[0][1:] + r.cycles[0][:1])
    b.set_rules(None)
    assert np.array_equal(b.rules(), r.life)
    assert _same(b.step_cycles(CYCLE_GENS) + (b.snapshot(),), r.cycles[1][1:] + r.cycles[1][:1])
    b.set_rules(r.words[FIRST:FIRST + PART], first=FIRST)
    assert np.array_equal(b.rules(), r.words)
    assert _same(b.step_cycles(CYCLE_GENS) + (b.snapshot(),), r.cycles[2][1:] + r.cycles[2][:1])
    assert b.epoch == 16 + 3 * CYCLE_GENS


def test_buffers_grow_are_reused_and_go_with_the_handle(gpu):
    r = _reference()
    b = GolBatch(BOARDS, W, H)
    _walk(b, r, True)
    b.close()  # 7. every buffer allocated ...
    b = GolBatch(BOARDS, W, H)
    _walk(b, r, False)
    b.close()  # ... and all but the cycle words
    with GolBatch(BOARDS, W, H) as fresh:  # the device is as it was: a third batch does what the first did
        fresh.seed(SEED)
        assert np.array_equal(fresh.step(6, populations=True), r.pops6)
