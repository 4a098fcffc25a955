"""GPU: per-board rules on a batch (gol_rules_batch_*, GolBatch.set_rules;
DESIGN.md section 5k).  Board i under rule i must do, bit for bit, what board
i of a uniform batch created with rule i does: the model of
tests/batch_rules_model.py steps every board alone under its own rule, and the
cycle words are held against uniform batches, which
tests/test_gpu_batch_cycles.py holds to their model.

Each shape reaches another loop or seam of the RULES instances:

    64 x 64 torus        k = 1, rotates, scalar masks
    20 x 64 torus        k = 1, rotates, narrow
    63 x 64 ref-clipped  k = 1, clipped wide
    32 x 33 ref-clipped  k = 1, 31 idle lanes, narrow
    33 x 21 torus        k = 3, permutes, wide, one idle lane, per-lane masks
    5 x 7 torus          k = 9, narrow, one idle lane
    8 x 8 ref-clipped    k = 8, the reference's board

Board counts {1, k, k + 1, 4k + 1} with k = 64 // H: a last wave that is not
full, and a second workgroup at 4 waves per workgroup.  The model is computed
once per shape for 4k + 1 boards and 37 generations and shared read-only: a
board's seed and rule depend on its index alone, so the first n boards of it
are the batch of n boards."""
import functools

import numpy as np
import pytest

import batch_model as M
import batch_rules_model as RM
from gameoflife import _native as N
from gameoflife.batch import GolBatch
from gameoflife.rules import rule_from_word, rule_word

pytestmark = pytest.mark.gpu

SEED = 0xBA7C4
GENS = (1, 2, 37)
SHAPES = [(64, 64, "torus"), (20, 64, "torus"), (63, 64, "ref-clipped"), (32, 33, "ref-clipped"),
          (33, 21, "torus"), (5, 7, "torus"), (8, 8, "ref-clipped")]


def _k(shape):
    return 64 // shape[1]


def _counts(shape):
    k = _k(shape)
    return sorted({1, k, k + 1, 4 * k + 1})


def _id(shape):
    return f"{shape[0]}x{shape[1]}-{shape[2]}"


CASES = [(s, n) for s in SHAPES for n in _counts(s)]


@functools.lru_cache(maxsize=None)
def _model(shape):
    """(rows, words, states [38][n][H], populations [n][37], settled [n]) of 4k + 1 seeded boards; read-only."""
    W, H, topo = shape
    n = 4 * _k(shape) + 1
    rows = M.seed_rows(n, W, H, SEED)
    words = RM.rule_words(n)
    out = (rows, words) + RM.run_history(rows, W, max(GENS), words, topo)
    for a in out:
        a.setflags(write=False)
    return out


def _settled(settled, gens):
    """What a call of `gens` generations reports, from the settle generation of a longer one."""
    return np.where((settled > 0) & (settled <= gens), settled, 0).astype(np.uint32)


def _batch(shape, boards, rule="life"):
    W, H, topo = shape
    return GolBatch(boards, W, H, topology=topo, rule=rule)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{_id(c[0])}-{c[1]}b")
def test_model_parity(gpu, case):
    shape, n = case
    rows, words, states, pops, settled = _model(shape)
    with _batch(shape, n) as b:
        b.set_rules(words[:n])
        for gens in GENS:
            b.seed(SEED)
            assert np.array_equal(b.snapshot(), rows[:n])
            got_pops, got_settled = b.step(gens, populations=True, settled=True)
            assert np.array_equal(b.snapshot(), states[gens][:n]), gens
            assert np.array_equal(got_pops, pops[:n, :gens]), gens
            assert np.array_equal(got_settled, _settled(settled[:n], gens)), gens
            assert np.array_equal(b.hashes(), M.hashes(states[gens][:n], shape[0])), gens
            assert b.epoch == gens
            # ... and the instances without the series and the settle words
            b.seed(SEED)
            assert b.step(gens) is None
            assert np.array_equal(b.snapshot(), states[gens][:n]), gens
            b.seed(SEED)
            assert np.array_equal(b.step(gens, populations=True), pops[:n, :gens]), gens
            b.seed(SEED)
            assert np.array_equal(b.step(gens, settled=True), _settled(settled[:n], gens)), gens
            assert np.array_equal(b.snapshot(), states[gens][:n]), gens


def test_the_model_tells_the_rules_apart():
    """No device: under one rule for every board the model's answer would be another, so parity shows the rule
    reached each board."""
    for shape in SHAPES:
        rows, words, states, pops, settled = _model(shape)
        n = rows.shape[0]
        life = RM.run_history(rows, shape[0], 2, np.full(n, rule_word("life"), dtype=np.uint32), shape[2])[0]
        differ = [i for i in range(n) if not np.array_equal(life[2][i], states[2][i])]
        assert len(differ) >= n - 2, (shape, differ)  # every board but life's own (and a chance equal)
        assert (settled > 0).any() and len(set(pops[:, -1].tolist())) > 2


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_chunk_independence(gpu, shape):
    rows, words, states, pops, settled = _model(shape)
    n = rows.shape[0]
    got = []
    with _batch(shape, n) as b:
        b.set_rules(words)
        for chunk in (5, 0):
            b.set_chunk(chunk)
            b.seed(SEED)
            p, s = b.step(37, populations=True, settled=True)
            got.append((b.snapshot(), p, s))
    for a, c in zip(got[0], got[1]):
        assert np.array_equal(a, c)
    assert np.array_equal(got[0][0], states[37]) and np.array_equal(got[0][1], pops)
    assert np.array_equal(got[0][2], _settled(settled, 37))


@pytest.mark.parametrize("shape", [(8, 8, "ref-clipped"), (5, 7, "torus"), (64, 64, "torus")], ids=_id)
def test_cycles_equal_the_uniform_batches(gpu, shape):
    W, H, topo = shape
    n = 4 * _k(shape) + 1
    rows = M.seed_rows(n, W, H, SEED)
    words = RM.named_words(n)
    got = {}
    with _batch(shape, n) as b:
        b.set_rules(words)
        for chunk in (0, 100):
            b.set_chunk(chunk)
            b.load(rows)
            period, seen = b.step_cycles(4096)
            got[chunk] = (period, seen, b.snapshot())
            assert b.epoch == 4096
    for name in RM.NAMED[:n]:  # the rules some board carries (the 64 x 64 batch has five boards)
        mine = np.flatnonzero(words == rule_word(name))
        assert mine.size >= 1
        with _batch(shape, n, rule=name) as u:
            for chunk in (0, 100):
                u.set_chunk(chunk)
                u.load(rows)
                period, seen = u.step_cycles(4096)
                final = u.snapshot()
                assert np.array_equal(got[chunk][0][mine], period[mine]), (name, chunk)
                assert np.array_equal(got[chunk][1][mine], seen[mine]), (name, chunk)
                assert np.array_equal(got[chunk][2][mine], final[mine]), (name, chunk)
    # the sweep saw something: every rule of the list ends these boards in a cycle, seen at different generations
    assert (got[0][0] > 0).all() and len(set(got[0][1].tolist())) > 2


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_same_rule_everywhere_equals_the_plain_batch(gpu, shape):
    n = 4 * _k(shape) + 1
    with _batch(shape, n) as a, _batch(shape, n) as b:
        b.set_rules(["life"] * n)
        a.seed(SEED)
        b.seed(SEED)
        pa, sa = a.step(37, populations=True, settled=True)
        pb, sb = b.step(37, populations=True, settled=True)
        assert np.array_equal(a.snapshot(), b.snapshot())
        assert np.array_equal(pa, pb) and np.array_equal(sa, sb)
        assert a.epoch == b.epoch == 37


def test_bookkeeping(gpu):
    shape = (33, 21, "torus")
    k = _k(shape)
    rows, words, states, pops, settled = _model(shape)
    n = rows.shape[0]
    W = shape[0]
    with _batch(shape, n, rule="B36/S23") as b:
        config = rule_word("B36/S23")
        assert b.rules().tolist() == [config] * n
        b.seed(SEED)
        b.step(3)
        before = b.snapshot()
        # set_rules touches neither the boards nor the epoch, and rules() returns what was set
        b.set_rules(words)
        assert np.array_equal(b.snapshot(), before) and b.epoch == 3
        assert np.array_equal(b.rules(), words)
        assert np.array_equal(b.rules(2, 5), words[2:7])
        assert rule_from_word(b.rules(0, 1)[0]).name == "life"
        # the forms set_rules takes
        b.set_rules([rule_from_word(w) for w in words[:3]] + ["B/S", (0x1FF, 0x1FF)], first=1)
        assert b.rules(1, 5).tolist() == words[:3].tolist() + [rule_word("B/S"), 0x01FF01FF]
        # a bad word raises and leaves rules() as it was
        held = b.rules()
        bad = words.copy()
        bad[4] |= np.uint32(1 << 9)
        with pytest.raises(N.GolError, match=r"rules\[4\]"):
            b.set_rules(bad)
        with pytest.raises(N.GolError, match="outside the batch"):
            b.set_rules(words, first=1)
        assert np.array_equal(b.rules(), held)
        # None: the configuration's rule again, equal to a fresh uniform batch from the same rows
        b.set_rules(None)
        assert b.rules().tolist() == [config] * n
        b.load(rows)
        got = b.step(37, populations=True, settled=True)
        with _batch(shape, n, rule="B36/S23") as u:
            u.load(rows)
            want = u.step(37, populations=True, settled=True)
            assert np.array_equal(b.snapshot(), u.snapshot())
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # a partial set: boards below k keep the configuration's rule; against the model
        b.set_rules(words[k:], first=k)
        mixed = np.concatenate([np.full(k, config, dtype=np.uint32), words[k:]])
        assert np.array_equal(b.rules(), mixed)
        final, mpops, msettled = RM.run(rows, W, 37, mixed, shape[2])
        b.load(rows)
        got = b.step(37, populations=True, settled=True)
        assert np.array_equal(b.snapshot(), final)
        assert np.array_equal(got[0], mpops) and np.array_equal(got[1], msettled)
        assert not np.array_equal(final[:k], states[37][:k])  # ... which the rules of the list would not give


def test_downstream_untouched(gpu):
    shape = (33, 21, "torus")
    rows, words, states, pops, settled = _model(shape)
    n = rows.shape[0]
    block = ["OO", "OO"]
    with _batch(shape, n) as b, _batch(shape, n) as u:
        b.set_rules(words)
        b.seed(SEED)
        b.step(37)
        final = b.snapshot()
        assert np.array_equal(final, states[37])
        u.load(final)
        assert np.array_equal(b.find(block), u.find(block))
        counts, objs = b.objects()
        want_counts, want_objs = u.objects()
        assert np.array_equal(counts, want_counts) and np.array_equal(objs, want_objs)
        assert counts.sum() > 0 and b.find(block).sum() > 0
