"""Dict model of the census of a batch's objects (gol_census_batch_*,
GolBatch.census_*) -- test infrastructure.  A plain
dictionary over (counts, records) as tests/objects_model.py and
tests/objects_cases.py give them: the contract's accounting, its exemplar rule
(the minimum of (call, board, y, x)) and its output order.  The model has room
for every key; what the device may do once it has not is in `check`."""
import numpy as np

from gameoflife.batch import CENSUS_DTYPE

KEY = ("hash", "w", "h", "population")


class Census:
    def __init__(self, max_keys=65536):
        self.max_keys = max_keys
        self.calls = self.seen = self.tallied = self.truncated = 0
        self.keys = {}  # (hash, w, h, population) -> [count, (call, board, y, x)]

    def _tally(self, rec, board):
        key = tuple(int(rec[f]) for f in KEY)
        place = (self.calls, board, int(rec["y"]), int(rec["x"]))
        slot = self.keys.setdefault(key, [0, place])
        slot[0] += 1
        slot[1] = min(slot[1], place)
        self.tallied += 1

    def add(self, counts, objects):
        """What census_add tallies of boards whose objects(reach, max_objects) is (counts, objects); the ordinal."""
        max_objects = objects.shape[1]
        for board, (n, recs) in enumerate(zip(counts.tolist(), objects)):
            self.seen += n
            self.truncated += max(n - max_objects, 0)
            for rec in recs[:min(n, max_objects)]:
                self._tally(rec, board)
        self.calls += 1
        return self.calls - 1

    def add_records(self, records, board=0):
        for rec in np.asarray(records).reshape(-1):
            if int(rec["population"]) != 0:
                self.seen += 1
                self._tally(rec, board)
        self.calls += 1
        return self.calls - 1

    def entries(self):
        """CENSUS_DTYPE [distinct]: what census_read returns while every key has room."""
        out = np.zeros(len(self.keys), dtype=CENSUS_DTYPE)
        order = sorted(self.keys.items(), key=lambda kv: (-kv[1][0],) + kv[0])
        for e, (key, (count, (call, board, y, x))) in zip(out, order):
            e["hash"], e["w"], e["h"], e["population"] = key
            e["count"] = count
            e["first_call"], e["first_board"], e["first_y"], e["first_x"] = call, board, y, x
        return out

    def stats(self):
        return {"calls": self.calls, "seen": self.seen, "tallied": self.tallied, "truncated": self.truncated,
                "overflowed": 0, "distinct": len(self.keys)}

    def check(self, entries, stats):
        """The device's (census_read(), census_stats()) against the model.  Always: the two invariants, the calls,
        seen and truncated, the order, and every entry present equal to the model's for its key.  With room for every
        key (distinct <= max_keys): nothing overflowed and nothing is missing."""
        assert entries.dtype == CENSUS_DTYPE
        want = self.stats()
        assert stats["seen"] == stats["tallied"] + stats["truncated"] + stats["overflowed"], stats
        assert int(entries["count"].sum()) == stats["tallied"] and stats["distinct"] == len(entries), stats
        assert {k: stats[k] for k in ("calls", "seen", "truncated")} == {k: want[k] for k in ("calls", "seen", "truncated")}
        order = [(-int(e["count"]),) + tuple(int(e[f]) for f in KEY) for e in entries]
        assert order == sorted(order) and len(set(o[1:] for o in order)) == len(order)
        if len(self.keys) <= self.max_keys:
            assert stats == want, (stats, want)
            model = self.entries()
            assert entries.tobytes() == model.tobytes(), (entries[:4].tolist(), model[:4].tolist())
            return
        by_key = {tuple(int(e[f]) for f in KEY): e for e in self.entries()}
        for e in entries:
            assert e.tobytes() == by_key[tuple(int(e[f]) for f in KEY)].tobytes(), e
