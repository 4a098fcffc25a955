"""CPU: the cases of the geometry sweeps (tests/sweep_cases.py), checked
without a device -- the batch enumeration against gol_batch_geometry_get, the
closed-form counts the GPU tests assert against, the three CPU steps against
each other on every visible-extent variant, the conditions the longer runs put
on their input, and the sweeps' sensitivity: the comparison the GPU tests use
reports a mismatch, at every height, for a model that ignores the visible
extents and for one that takes the torus wrap bit from `width` instead of
`width - 1`."""
import ctypes

import numpy as np
import pytest

import sweep_cases as S
from gameoflife import _native as N
from oracle import oracle as O

TOPOLOGY = {"torus": N.GOL_TORUS, "ref-clipped": N.GOL_REF_CLIPPED}


def _accepts(W, H, topology, vis):
    c = N.GolBatchConfig()
    c.boards, c.width, c.height, c.topology = 1, W, H, TOPOLOGY[topology]
    c.birth_mask, c.survive_mask = O.LIFE
    c.device = 0
    c.vis_width, c.vis_height = vis
    g = N.GolBatchGeometry()
    rc = N.lib.gol_batch_geometry_get(ctypes.byref(c), ctypes.byref(g))
    assert rc in (N.GOL_OK, N.GOL_EINVAL)
    return rc == N.GOL_OK


def _board(W, H, topology, vis):
    """The board a configuration stands for: 0 is the default W - 1 / H - 1,
    W + 1 / H + 1 the same board as W / H; a torus has no visible extents."""
    if topology == "torus":
        return W, H
    vw, vh = (vis[0] if vis[0] > 0 else W - 1), (vis[1] if vis[1] > 0 else H - 1)
    return W, H, min(vw, W), min(vh, H)


@pytest.mark.parametrize("topology", ["torus", "ref-clipped"])
def test_enumeration_is_what_the_validator_accepts(topology):
    accepted = set()
    for W in range(0, 66):
        for H in range(0, 66):
            for vw in (0, W - 1, W, W + 1):
                for vh in (0, H - 1, H, H + 1):
                    if _accepts(W, H, topology, (vw, vh)):
                        accepted.add(_board(W, H, topology, (vw, vh)))
    geoms = S.batch_geometries(topology)
    assert len(set(geoms)) == len(geoms)
    assert {_board(W, H, topology, vis) for W, H, vis in geoms} == accepted
    # every geometry as the sweep passes it, the (0, 0) of the default included
    assert all(_accepts(W, H, topology, vis) for W, H, vis in geoms)


def test_batch_counts():
    assert len(S.batch_geometries("torus")) == S.batch_geometry_count("torus") == 3844
    assert len(S.batch_geometries("ref-clipped")) == S.batch_geometry_count("ref-clipped") == 16125
    for topology in TOPOLOGY:
        per_height = [S.batch_geometries(topology, H) for H in range(1, 65)]
        assert [len(g) for g in per_height] == [S.batch_geometry_count(topology, H) for H in range(1, 65)]
        assert sorted(sum(per_height, [])) == sorted(S.batch_geometries(topology))
        for H in range(1 if topology == "ref-clipped" else 3, 65):
            long = S.long_run_geometries(topology, H)
            assert len(long) == S.long_run_count(topology, H) and set(long) <= set(per_height[H - 1])
            assert {g[0] for g in long} >= set(S.LONG_WIDTHS)
    # the default extents go in as (0, 0), and a quarter or so of the clipped geometries are defaults
    assert sum(1 for g in S.batch_geometries("ref-clipped") if g[2] == (0, 0)) == 63 * 63 - 1


def test_rule_words_include_births_on_0_neighbours():
    for W, H in ((3, 3), (47, 11), (64, 64), (1, 2)):
        words = S.batch_rule_words(W, H)
        assert words.dtype == np.uint32 and len(words) == S.batch_boards(H)
        assert not (words & ~np.uint32(0x01FF01FF)).any()
        assert (words & 1).any()
        assert np.array_equal(words, S.batch_rule_words(W, H))
    assert any((S.batch_rule_words(W, 7) & 1).sum() < S.batch_boards(7) for W in range(3, 10))
    assert S.UNIFORM_RULES[0][0] & 1 and not S.UNIFORM_RULES[1][0] & 1
    assert O.LIFE not in S.UNIFORM_RULES


SIZES = [(2, 2), (3, 2), (5, 7), (8, 8), (31, 4), (32, 5), (33, 6), (40, 9), (63, 3), (64, 64), (65, 5), (97, 4)]


@pytest.mark.parametrize("rule", [O.LIFE, O.REF_LITERAL, (0x049, 0x16E)])
def test_the_three_steps_agree_on_every_visible_extent(rule):
    ran = 0
    for W, H in SIZES:
        cells = (np.random.default_rng([W, H]).random((H, W)) < 0.5).astype(np.uint8)
        for vis in S.clipped_variants(W, H):
            v = S.visible(W, H, "ref-clipped", vis)
            a = O.step_cells(cells, O.REF_CLIPPED, rule, vis=v)
            b = O.np_step(cells, O.REF_CLIPPED, rule, vis=v)
            c = O.unpack(O.step_packed(O.pack(cells), W, O.REF_CLIPPED, rule, vis=v), W)
            assert np.array_equal(a, b) and np.array_equal(a, c), (W, H, vis)
            ran += 1
    assert ran == 4 * len(SIZES) - 1  # (2, 2) has no default extents


def test_visible_extents_change_the_result():
    cells = (np.random.default_rng(409).random((9, 40)) < 0.5).astype(np.uint8)
    default = O.step_cells(cells, O.REF_CLIPPED, O.LIFE)
    for vis in ((40, 9), (40, 8), (39, 9)):
        assert (O.step_cells(cells, O.REF_CLIPPED, O.LIFE, vis=vis) != default).any(), vis


def test_engine_variants_are_what_gol_create_accepts():
    from gameoflife.engine import GolEngine

    def accepts(W, H, vis):
        try:
            GolEngine(W, H, topology="ref-clipped", vis=vis).close()
            return True
        except N.GolError as e:
            assert e.code in (N.GOL_EINVAL, N.GOL_ENODEV)
            return e.code == N.GOL_ENODEV
    for W in (1, 2, 3, 7, 33, 130):
        for H in (1, 2, 3, 9, 26):
            want = {(W, H, *S.explicit_extents(W, H, vis)) for vis in S.engine_variants(W, H)}
            got = {(W, H, vw, vh) for vw in (W - 1, W) for vh in (H - 1, H)
                   if vw > 0 and vh > 0 and accepts(W, H, (vw, vh))}
            assert got == want, (W, H)
            assert accepts(W, H, (0, 0)) == ((0, 0) in S.engine_variants(W, H))
    assert not accepts(2, 2, (0, 0))  # refused, as today
    # one column: explicit extents only
    assert not accepts(1, 9, (0, 0)) and accepts(1, 9, (1, 9)) and accepts(1, 9, (1, 8))
    assert [c[:2] for c in S.one_column_cases()[::12]] == [(2, (1, 2)), (3, (1, 2)), (3, (1, 3)), (9, (1, 8)),
                                                           (9, (1, 9))]


def test_shard_counts():
    assert sorted(w for b in S.WORD_BLOCKS for w in b) == list(range(1, 261)) + list(range(264, 521, 4))
    total = 0
    for words in S.WORDS + S.WORDS_VEC4:
        cases = S.torus_cases(words)
        assert len(cases) == len(set(cases)) == S.torus_case_count(words), words
        # 16-byte lanes deeper than 7 off the B3/S23 torus are never generated
        assert not any(rule == "generic" and lanes == 4 and G > 7 for rule, G, lanes, _ in cases)
        assert all(lanes == 0 or words % lanes == 0 for _, _, lanes, _ in cases)
        total += len(cases)
    assert total == S.TORUS_CASES
    assert sorted(w for b in S.CLIPPED_BLOCKS for w in b) == sorted(S.CLIPPED_WIDTHS) and len(S.CLIPPED_WIDTHS) == 157
    assert {W % 32 for W in range(2, 131)} == set(range(32))
    for W in S.CLIPPED_WIDTHS:
        assert len(S.clipped_cases(W)) == S.clipped_case_count(W)
    assert len(S.one_column_cases()) == S.ONE_COLUMN_COUNT == 60
    assert len(S.clipped_height_cases(7)) == S.CLIPPED_HEIGHT_COUNT == 300
    # every block of the torus sweep meets an odd and an even word count, one the whole-row wave's 128 words
    for block in S.WORD_BLOCKS[:26]:
        want = S.expected_strips(block)
        assert all(want[(G, 0)] >= {62, 124} for G in range(2, 13))
        assert want[(1, 1)] == {64} and want[(1, 2)] == {128} and want[(1, 4)] == {256} and want[(7, 4)] == {248}
    assert sum(128 in S.expected_strips(b).get((10, 0), ()) for b in S.WORD_BLOCKS) == 1


def test_mismatch_names_the_first_wrong_word():
    a = {"final": np.arange(6, dtype=np.uint64).reshape(2, 3), "settled": np.zeros(2, dtype=np.uint32)}
    b = {k: v.copy() for k, v in a.items()}
    assert S.mismatch(a, b) is None
    b["final"][1, 2] ^= np.uint64(1 << 63)
    assert S.mismatch(b, a).startswith("final[1, 2]: 0x8000000000000005 for 0x5")
    b = {k: v.copy() for k, v in a.items()}
    b["settled"][1] = 2
    assert S.mismatch(b, a).startswith("settled[1]: 0x2 for 0x0")
    b["settled"] = b["settled"].astype(np.uint64)
    assert "uint64" in S.mismatch(b, a)


def test_longer_runs_split_their_input():
    """Conditions on the input of the longer runs, on the model alone: the
    boards include settled and unsettled ones, boards with a period and boards
    without.  Three heights show it, so it holds over the sweep."""
    settled, period = [], []
    for topology, H in (("torus", 3), ("ref-clipped", 8), ("torus", 64)):
        for g in S.long_run_geometries(topology, H):
            short, long = S.expected_long(g, topology)
            settled.append(short["settled"])
            period.append(long["period"])
            assert ((long["seen"] == 0) == (long["period"] == 0)).all()
    settled, period = np.concatenate(settled), np.concatenate(period)
    assert (settled == 0).any() and (settled != 0).any()
    assert (period == 0).any() and (period != 0).any()


@pytest.mark.parametrize("H", range(1, 65))
def test_sweep_notices_ignored_visible_extents(H):
    rule = S.UNIFORM_RULES[1]
    noticed = 0
    for g in ((47, H, (0, 0) if H > 1 else (46, 1)), (33, H, (33, H - 1) if H > 1 else (32, 1))):
        assert g in S.batch_geometries("ref-clipped", H)
        true = S.expected_uniform(g, "ref-clipped", rule)
        assert S.mismatch(S.expected_uniform(g, "ref-clipped", rule, step=S.stepper("ref-clipped", rule,
                          S.visible(*g[:2], "ref-clipped", g[2]))), true) is None
        wrong = S.expected_uniform(g, "ref-clipped", rule, step=S.step_all_visible(rule))
        noticed += S.mismatch(wrong, true) is not None
    assert noticed >= 1


@pytest.mark.parametrize("H", range(3, 65))
def test_sweep_notices_a_wrap_bit_taken_from_width(H):
    noticed = 0
    for W in (3, 47, 64):
        g = (W, H, (0, 0))
        true = S.expected_uniform(g, "torus", O.LIFE)
        wrong = S.expected_uniform(g, "torus", O.LIFE, step=S.step_wrap_bit_off_by_one(O.LIFE))
        noticed += S.mismatch(wrong, true) is not None
    assert noticed >= 1


def test_the_corrupted_wrap_is_the_true_step_away_from_column_0():
    cells = (np.random.default_rng(7).random((9, 20)) < 0.5).astype(np.uint8)
    cells[:, -1] = 0  # nothing in the last column: nothing to wrap to column 0
    assert np.array_equal(S.step_wrap_bit_off_by_one(O.LIFE)(cells), O.step_cells(cells, O.TORUS, O.LIFE))
