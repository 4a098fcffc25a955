"""CPU: the dict census of tests/census_model.py against what a caller had
before the device census -- batch.tally over the records patterns.label_objects
gives -- on the seeded boards of tests/objects_cases.py, its accounting and
exemplar rule by hand, and batch.census_names on a hand-made entry array."""
import numpy as np
import pytest

import batch_model as M
import census_model as CM
import objects_cases as C
from gameoflife import patterns as P
from gameoflife.batch import CENSUS_DTYPE, OBJECT_DTYPE, census_names, tally

TABLE = P.object_table({"block": [["OO", "OO"]], "beehive": [[".OO.", "O..O", ".OO."]], "blinker": [["OOO"]],
                        "dot": [["O"]], "domino": [["OO"]]})


def _labelled(shape, boards, generation, reach, max_objects):
    """(counts, objects) as GolBatch.objects gives them, from the package's own host labeller."""
    W, H, topo, vis = shape
    cells = M.unpack(C.states(shape, boards)[generation], W)
    counts = np.zeros(boards, dtype=np.uint32)
    objects = np.zeros((boards, max_objects), dtype=OBJECT_DTYPE)
    for b in range(boards):
        recs = P.label_objects(cells[b], torus=topo == "torus", reach=reach)
        counts[b] = len(recs)
        objects[b, :min(len(recs), max_objects)] = recs[:max_objects]
    return counts, objects


@pytest.mark.parametrize("case", C.SHAPES, ids=C.shape_id)
def test_model_names_equal_tally_of_the_labelled_records(case):
    shape, boards = case
    g = C.generations(shape)[-1]
    for reach, max_objects in ((1, C.MAX_OBJECTS), (2, 8)):
        counts, objects = _labelled(shape, boards, g, reach, max_objects)
        census = CM.Census()
        assert census.add(*C.model(shape, boards, g, reach, max_objects)) == 0
        assert census_names(census.entries(), TABLE) == tally(counts, objects, TABLE)
        stats = census.stats()
        assert stats["seen"] == int(counts.sum()) == stats["tallied"] + stats["truncated"]
        assert stats["tallied"] == int(np.minimum(counts, max_objects).sum()) == int(census.entries()["count"].sum())
        census.check(census.entries(), stats)


def _recs(*rows):
    out = np.zeros(len(rows), dtype=OBJECT_DTYPE)
    for rec, (h, x, y, w, hh, pop) in zip(out, rows):
        rec["hash"], rec["x"], rec["y"], rec["w"], rec["h"], rec["population"] = h, x, y, w, hh, pop
    return out


def test_model_accounting_exemplar_and_order_by_hand():
    census = CM.Census(max_keys=4)
    # board 0 has three objects and room for two, board 1 one
    counts = np.array([3, 1], dtype=np.uint32)
    objects = np.zeros((2, 2), dtype=OBJECT_DTYPE)
    objects[0] = _recs((7, 5, 5, 2, 2, 4), (9, 1, 6, 3, 1, 3))
    objects[1, 0] = _recs((7, 0, 9, 2, 2, 4))[0]
    assert census.add(counts, objects) == 0
    # the same key earlier on the board than call 0 had it, but in a later call; a population 0 is no record
    assert census.add_records(_recs((7, 0, 0, 2, 2, 4), (5, 0, 0, 0, 0, 0), (9, 0, 0, 3, 1, 3), (9, 2, 2, 1, 3, 3)), 7) == 1
    assert census.stats() == {"calls": 2, "seen": 7, "tallied": 6, "truncated": 1, "overflowed": 0, "distinct": 3}
    e = census.entries()
    assert [tuple(int(r[f]) for f in CM.KEY) + (int(r["count"]),) for r in e] == [(7, 2, 2, 4, 3), (9, 3, 1, 3, 2),
                                                                                   (9, 1, 3, 3, 1)]
    assert [(int(r["first_call"]), int(r["first_board"]), int(r["first_y"]), int(r["first_x"])) for r in e] == [
        (0, 0, 5, 5), (0, 0, 6, 1), (1, 7, 2, 2)]
    assert not e["reserved"].any()
    census.check(e, census.stats())
    with pytest.raises(AssertionError):  # a count off by one breaks the second invariant
        bad = e.copy()
        bad["count"][0] += 1
        census.check(bad, census.stats())


def test_model_beyond_its_room_asserts_the_invariants_only():
    census = CM.Census(max_keys=1)
    census.add_records(_recs((1, 0, 0, 1, 1, 1), (2, 0, 0, 1, 1, 1), (2, 3, 0, 1, 1, 1)))
    full = census.entries()
    kept = full[:1]  # the device kept the key with two objects and lost the other
    census.check(kept, {"calls": 1, "seen": 3, "tallied": 2, "truncated": 0, "overflowed": 1, "distinct": 1})
    with pytest.raises(AssertionError):
        census.check(kept, {"calls": 1, "seen": 3, "tallied": 2, "truncated": 0, "overflowed": 0, "distinct": 1})
    with pytest.raises(AssertionError):  # a kept entry has the model's count
        wrong = kept.copy()
        wrong["count"][0] = 1
        census.check(wrong, {"calls": 1, "seen": 3, "tallied": 1, "truncated": 0, "overflowed": 2, "distinct": 1})


def test_census_names_on_a_hand_made_entry_array():
    entries = np.zeros(4, dtype=CENSUS_DTYPE)
    block = next(k for k, v in TABLE.items() if v == "block")
    blinkers = sorted(k for k, v in TABLE.items() if v == "blinker")
    assert len(blinkers) == 2
    for e, (key, count) in zip(entries, [(block, 10), (blinkers[0], 3), (blinkers[1], 4), ((123, 5, 5, 9), 2)]):
        e["hash"], e["w"], e["h"], e["population"] = key
        e["count"] = count
    assert census_names(entries, TABLE) == {"block": 10, "blinker": 7, None: 2}
    assert census_names(entries[:0], TABLE) == {}
    # a key that differs from the block's in its population alone is not a block
    entries[3]["hash"], entries[3]["w"], entries[3]["h"], entries[3]["population"] = block[0], block[1], block[2], 5
    assert census_names(entries, TABLE) == {"block": 10, "blinker": 7, None: 2}
