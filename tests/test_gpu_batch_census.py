"""GPU: the census of a batch's objects kept on the device
(gol_census_batch_*, GolBatch.census_*).  Entries and
statistics against the dict model of tests/census_model.py over the objects of
tests/objects_model.py, on the seeded boards of tests/objects_cases.py (loaded
from the model's states, so nothing here depends on the step kernels but the
test that says so) and on hand-made records for the keys no board produces."""
import ctypes

import numpy as np
import pytest

import batch_model as M
import census_model as CM
import objects_cases as C
from gameoflife import _native as N
from gameoflife import patterns as P
from gameoflife.batch import CENSUS_DTYPE, OBJECT_DTYPE, GolBatch, census_names, tally
from test_gpu_batch_cycles import _model as cycle_model

pytestmark = pytest.mark.gpu

T64, C64, T8, C8 = (C.SHAPES[i][0] for i in range(4))
MAX_KEYS = 4096
TABLE = P.object_table({"block": [["OO", "OO"]], "beehive": [[".OO.", "O..O", ".OO."]], "blinker": [["OOO"]],
                        "dot": [["O"]], "domino": [["OO"]]})
ZEROS = {"calls": 0, "seen": 0, "tallied": 0, "truncated": 0, "overflowed": 0, "distinct": 0}


def _batch(boards, shape):
    W, H, topo, vis = shape
    return GolBatch(boards, W, H, topology=topo, vis=vis)


def _recs(rows):
    """OBJECT_DTYPE records from (hash, x, y, w, h, population) rows."""
    out = np.zeros(len(rows), dtype=OBJECT_DTYPE)
    for f, col in zip(("hash", "x", "y", "w", "h", "population"), zip(*rows)):
        out[f] = np.array(col, dtype=np.uint64).astype(out.dtype[f])
    return out


def _key_counts(entries):
    return {tuple(int(e[f]) for f in CM.KEY): int(e["count"]) for e in entries}


@pytest.mark.parametrize("reach", C.REACHES)
@pytest.mark.parametrize("case", C.SHAPES, ids=C.shape_id)
def test_seeded_shapes_match_model(gpu, case, reach):
    shape, boards = case
    with _batch(boards, shape) as b:
        for g in C.generations(shape):
            b.load(C.states(shape, boards)[g])
            b.census_begin(MAX_KEYS)
            assert b.census_add(reach=reach, max_objects=C.MAX_OBJECTS) == 0
            census = CM.Census(MAX_KEYS)
            census.add(*C.model(shape, boards, g, reach))
            got = b.census_read()
            census.check(got, b.census_stats())
            assert got.tobytes() == census.entries().tobytes()
            counts, objs = b.objects(reach=reach, max_objects=C.MAX_OBJECTS)
            assert int(got["count"].sum()) == int(counts.sum()) == b.census_stats()["seen"]
            assert census_names(got, TABLE) == tally(counts, objs, TABLE)


def test_three_calls_accumulate_and_a_second_begin_empties(gpu):
    gens = C.generations(T64)
    assert len(gens) == 3
    with _batch(5, T64) as b:
        assert b.census_stats() == ZEROS
        b.census_begin(MAX_KEYS)
        assert b.census_stats() == ZEROS and len(b.census_read()) == 0
        census = CM.Census(MAX_KEYS)
        for call, g in enumerate(gens):
            b.load(C.states(T64, 5)[g])
            assert b.census_add(reach=1, max_objects=C.MAX_OBJECTS) == call == census.add(*C.model(T64, 5, g, 1))
        got = b.census_read()
        census.check(got, b.census_stats())
        assert b.census_stats()["calls"] == 3 and set(got["first_call"].tolist()) == {0, 1, 2}
        # counts are the sums of the three calls on their own
        alone = {}
        for g in gens:
            one = CM.Census()
            one.add(*C.model(T64, 5, g, 1))
            for key, n in _key_counts(one.entries()).items():
                alone[key] = alone.get(key, 0) + n
        assert _key_counts(got) == alone
        assert b.census_read().tobytes() == got.tobytes()  # reading clears nothing
        # the records of an objects call, merged board by board, are what add tallies
        b.census_begin(MAX_KEYS)
        merged = CM.Census(MAX_KEYS)
        counts, objs = C.model(T64, 5, gens[1], 1)
        for board in (3, 0, 4, 1, 2):
            assert b.census_add_records(objs[board], board) == merged.add_records(objs[board], board)
        got = b.census_read()
        merged.check(got, b.census_stats())
        one = CM.Census()
        one.add(counts, objs)
        assert _key_counts(got) == _key_counts(one.entries())
        b.census_begin(16)  # another capacity
        assert b.census_stats() == ZEROS and len(b.census_read()) == 0


def test_one_key_under_high_contention(gpu):
    """256 boards tiled with blocks at pitch 3: 441 per board, every record of every wave the same key."""
    cells = np.zeros((1, 64, 64), dtype=np.uint8)
    for y in range(0, 63, 3):
        for x in range(0, 63, 3):
            cells[0, y:y + 2, x:x + 2] = 1
    with GolBatch(256, 64, 64) as b:
        b.load(np.repeat(M.pack(cells), 256, axis=0))
        b.census_begin(MAX_KEYS)
        b.census_add(reach=1, max_objects=512)
        got = b.census_read()
        assert len(got) == 1 and int(got[0]["count"]) == 256 * 441 == 112896
        e = got[0]
        assert (int(e["hash"]), int(e["w"]), int(e["h"]), int(e["population"])) == (P.object_hash(["OO", "OO"]), 2, 2, 4)
        assert (int(e["first_call"]), int(e["first_board"]), int(e["first_y"]), int(e["first_x"])) == (0, 0, 0, 0)
        assert b.census_stats() == {"calls": 1, "seen": 112896, "tallied": 112896, "truncated": 0, "overflowed": 0,
                                    "distinct": 1}


def test_all_keys_of_a_wave_different(gpu):
    rng = np.random.default_rng(C.SEED)
    hashes = rng.integers(0, 1 << 64, size=4096, dtype=np.uint64)
    assert len(set(hashes.tolist())) == 4096
    recs = np.zeros(4096, dtype=OBJECT_DTYPE)
    recs["hash"], recs["w"], recs["h"], recs["population"] = hashes, 3, 3, 5
    recs["x"], recs["y"] = np.arange(4096) % 64, np.arange(4096) // 64
    with _batch(3, T8) as b:
        b.census_begin(MAX_KEYS)
        census = CM.Census(MAX_KEYS)
        assert b.census_add_records(recs, 9) == 0 == census.add_records(recs, 9)
        assert b.census_add_records(recs, 2) == 1 == census.add_records(recs, 2)
        got = b.census_read()
        census.check(got, b.census_stats())
        assert len(got) == 4096 and (got["count"] == 2).all() and (got["first_call"] == 0).all()
        assert (got["first_board"] == 9).all() and got["hash"].tolist() == sorted(hashes.tolist())


def test_keys_that_differ_in_one_word_only(gpu):
    rows = [  # hash, x, y, w, h, population
        (0xABCDEF, 0, 0, 2, 2, 4), (0xABCDEF, 1, 0, 3, 2, 4), (0xABCDEF, 2, 0, 2, 3, 4), (0xABCDEF, 3, 0, 2, 2, 5),
        # hashes that differ above bit 47 only: the first word of the key is the same
        (0x0000123456789ABC, 4, 0, 1, 1, 1), (0x0001123456789ABC, 5, 0, 1, 1, 1), (0x8000123456789ABC, 6, 0, 1, 1, 1),
        (0xFFFF123456789ABC, 7, 0, 1, 1, 1),
        (0, 8, 0, 1, 1, 1), (0, 9, 0, 64, 64, 4096), ((1 << 64) - 1, 10, 0, 1, 1, 1), ((1 << 64) - 1, 11, 0, 64, 64, 4096),
        (1 << 47, 12, 0, 1, 1, 1), (1 << 48, 13, 0, 1, 1, 1), (1, 14, 0, 1, 1, 1), (1 << 63, 15, 0, 255, 255, 65535),
    ]
    recs = _recs(rows)
    assert len({(r[0],) + r[3:] for r in rows}) == len(rows) == 16
    # key i occurs i + 1 times, spread over the array, and a record without a population is skipped
    many = np.concatenate([recs[i:] for i in range(len(rows))][::-1] + [_recs([(0xABCDEF, 0, 0, 2, 2, 0)])])
    with _batch(3, T8) as b:
        b.census_begin(64)
        census = CM.Census(64)
        assert b.census_add_records(many, 1) == census.add_records(many, 1)
        got = b.census_read()
        census.check(got, b.census_stats())
        assert len(got) == 16 and sorted(got["count"].tolist()) == list(range(1, 17))
        assert b.census_stats()["seen"] == len(many) - 1 == 136
        assert not got["reserved"].any()


def test_truncation_is_counted(gpu):
    counts, objs = C.model(T64, 5, 64, 1, 8)
    assert (counts > 8).all()
    with _batch(5, T64) as b:
        b.load(C.states(T64, 5)[64])
        b.census_begin(MAX_KEYS)
        b.census_add(reach=1, max_objects=8)
        census = CM.Census(MAX_KEYS)
        census.add(counts, objs)
        census.check(b.census_read(), b.census_stats())
        s = b.census_stats()
        assert s["truncated"] == int((counts - 8).sum()) > 0 and s["tallied"] == 40 and s["overflowed"] == 0


def test_overflow_is_counted_and_kept_entries_are_exact(gpu):
    shape, boards = C.SHAPES[2]
    assert shape == T8
    with _batch(boards, T8) as b:
        for g in C.generations(T8):
            b.load(C.states(T8, boards)[g])
            b.census_begin(1)  # two slots
            b.census_add(reach=1, max_objects=C.MAX_OBJECTS)
            census = CM.Census(1)
            census.add(*C.model(T8, boards, g, 1))
            assert census.stats()["distinct"] > 2
            got, s = b.census_read(), b.census_stats()
            census.check(got, s)  # the invariants, and every kept entry the model's
            assert s["overflowed"] > 0 and 1 <= len(got) <= 2
            assert s["overflowed"] == census.stats()["tallied"] - int(got["count"].sum())


def test_read_with_a_short_capacity(gpu):
    with _batch(5, T64) as b:
        b.load(C.states(T64, 5)[64])
        b.census_begin(MAX_KEYS)
        b.census_add()
        want = b.census_read()
        assert len(want) > 3
        out = np.full(len(want) * 32, 0x5A, dtype=np.uint8).view(CENSUS_DTYPE)
        sentinel = out.tobytes()
        n = ctypes.c_size_t(12345)
        op = out.ctypes.data_as(ctypes.POINTER(N.GolCensusEntry))
        for capacity in (0, len(want) - 1):
            assert N.lib.gol_census_batch_read(b._h, op, capacity, ctypes.byref(n)) == N.GOL_EINVAL
            assert n.value == len(want) and out.tobytes() == sentinel
            assert b"distinct keys" in N.lib.gol_batch_last_error(b._h)
        assert N.lib.gol_census_batch_read(b._h, op, len(want), None) == N.GOL_EINVAL and out.tobytes() == sentinel
        assert N.lib.gol_census_batch_read(b._h, op, len(want), ctypes.byref(n)) == N.GOL_OK
        assert out.tobytes() == want.tobytes()


def test_a_call_changes_nothing(gpu):
    boards, N_ = 33, 512
    W, H, topo, vis = T8
    rows = M.seed_rows(boards, W, H, C.SEED)
    with _batch(boards, T8) as b:
        b.seed(C.SEED)
        b.step(3)
        before = (b.snapshot(), b.hashes(), b.epoch)
        objects_before = b.objects(reach=2, max_objects=16)
        stats_before = b.objects_stats()
        b.census_begin(MAX_KEYS)
        for reach in C.REACHES:
            b.census_add(reach=reach, max_objects=7)
        b.census_read()
        assert np.array_equal(b.snapshot(), before[0]) and np.array_equal(b.hashes(), before[1])
        assert b.epoch == before[2] == 3 and b.objects_stats() == stats_before
        after = b.objects(reach=2, max_objects=16)
        assert np.array_equal(after[0], objects_before[0]) and after[1].tobytes() == objects_before[1].tobytes()
        # a settle step that follows gives the model's answer
        b.seed(C.SEED)
        b.census_add()
        pops, settled = b.step(64, populations=True, settled=True)
        want = M.run(rows, W, 64, topo)
        assert np.array_equal(b.snapshot(), want[0]) and np.array_equal(pops, want[1])
        assert np.array_equal(settled, want[2])
        # ... and so does a cycle step continued across a call
        final, period, seen = cycle_model(T8, boards, N_)
        with _batch(boards, T8) as other:
            other.seed(C.SEED)
            other.step_cycles(100)
            plain = other.step_cycles(N_ - 100)
            b.seed(C.SEED)
            b.step_cycles(100)
            b.census_add(reach=2, max_objects=7)
            mine = b.step_cycles(N_ - 100)
            assert np.array_equal(mine[0], plain[0]) and np.array_equal(mine[1], plain[1])
            assert np.array_equal(b.snapshot(), other.snapshot()) and b.epoch == other.epoch == N_
            assert np.array_equal(b.snapshot(), final)
        assert b.geometry()["device_bytes"] == 2 * boards * H * 8 + boards * 4


def test_refusals_before_begin_and_of_bad_arguments(gpu):
    with _batch(3, T8) as b:
        b.seed(C.SEED)
        call, n = ctypes.c_uint32(77), ctypes.c_size_t(78)
        out = np.full(4 * 32, 0x5A, dtype=np.uint8).view(CENSUS_DTYPE)
        sentinel = out.tobytes()
        op = out.ctypes.data_as(ctypes.POINTER(N.GolCensusEntry))
        recs = _recs([(5, 0, 0, 1, 1, 1)])
        rp = recs.ctypes.data_as(ctypes.POINTER(N.GolBatchObject))
        for rc in (N.lib.gol_census_batch_add(b._h, 1, 128, ctypes.byref(call)),
                   N.lib.gol_census_batch_add_records(b._h, rp, 1, 0, ctypes.byref(call)),
                   N.lib.gol_census_batch_read(b._h, op, 4, ctypes.byref(n))):
            assert rc == N.GOL_EINVAL
            assert b"no census has begun" in N.lib.gol_batch_last_error(b._h)
        assert call.value == 77 and n.value == 78 and out.tobytes() == sentinel
        for max_keys in (0, -1, (1 << 20) + 1):
            assert N.lib.gol_census_batch_begin(b._h, max_keys) == N.GOL_EINVAL
            assert b"max_keys must be 1 .. 2^20" in N.lib.gol_batch_last_error(b._h)
        assert b.census_stats() == ZEROS
        b.census_begin(8)
        refusals = {
            "reach 0": (N.lib.gol_census_batch_add, (0, 128, ctypes.byref(call)), b"reach must be 1 or 2"),
            "reach 3": (N.lib.gol_census_batch_add, (3, 128, ctypes.byref(call)), b"reach must be 1 or 2"),
            "max_objects 0": (N.lib.gol_census_batch_add, (1, 0, ctypes.byref(call)), b"max_objects must be 1 .. 1024"),
            "max_objects 1025": (N.lib.gol_census_batch_add, (1, 1025, ctypes.byref(call)),
                                 b"max_objects must be 1 .. 1024"),
            "n 2^22 + 1": (N.lib.gol_census_batch_add_records, (rp, (1 << 22) + 1, 0, ctypes.byref(call)),
                           b"n must be at most 2^22"),
            "null records": (N.lib.gol_census_batch_add_records, (None, 1, 0, ctypes.byref(call)), b"records is null"),
            "board 2^22": (N.lib.gol_census_batch_add_records, (rp, 1, 1 << 22, ctypes.byref(call)),
                           b"board must be below 2^22"),
        }
        for what, (fn, args, word) in refusals.items():
            assert fn(b._h, *args) == N.GOL_EINVAL, what
            assert word in N.lib.gol_batch_last_error(b._h), (what, N.lib.gol_batch_last_error(b._h))
        assert call.value == 77 and b.census_stats() == ZEROS  # a refused call takes no ordinal
        # n = 0 takes an ordinal and tallies nothing; the largest board and a NULL call_out are fine
        assert N.lib.gol_census_batch_add_records(b._h, None, 0, 0, ctypes.byref(call)) == N.GOL_OK and call.value == 0
        assert N.lib.gol_census_batch_add_records(b._h, rp, 1, (1 << 22) - 1, None) == N.GOL_OK
        got = b.census_read()
        assert len(got) == 1 and (int(got[0]["first_call"]), int(got[0]["first_board"])) == (1, (1 << 22) - 1)
        assert b.census_stats() == {"calls": 2, "seen": 1, "tallied": 1, "truncated": 0, "overflowed": 0, "distinct": 1}
