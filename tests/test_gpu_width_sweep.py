"""GPU: the shard engine on every row width up to two strips and every short
height ("The geometry sweeps"), bit-exact against the CPU
oracle: per-generation hashes and the final board of step(hashes=True), the
final board and gol_hash of the unhashed step.  The hand-picked lists of
tests/test_gpu_parity.py and tests/test_gpu_unhashed_passes.py keep the large
boards, the band schedules and the rings; here the boards are tiny and the
widths, heights, depths, lane widths and visible extents are all of them.

A case runs G + 1 generations at a fixed depth G: one pass of depth G and a
one-generation remainder.  One context per board shape is reused across
depths, lane widths and both families (set_tuning + load; load resets the
epoch), so every run after the first starts on stale spare planes.  The cases
and the counts the tests assert come from tests/sweep_cases.py."""
import numpy as np
import pytest

import sweep_cases as S
from gameoflife import _native as N
from gameoflife.engine import GolEngine, ShardGroup
from gameoflife.rules import Rule
from gameoflife.shard import shard_rows_py
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def run_case(e, board, ref, gens, G, lanes, family, what):
    """One case on a context that may have run others: tuning, load, step,
    compare with ref = (final board, per-generation hashes) of the oracle."""
    final_cpu, want = ref
    e.set_tuning(gens_per_pass=G, words_per_lane=lanes)
    e.load(board)
    if family == "hashed":
        got = e.step(gens, hashes=True)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{what}: first hash mismatch at generation {bad[0] + 1}"
    else:
        e.step(gens)
        assert e.hash() == int(want[-1]), f"{what}: gol_hash"
    assert e.epoch == gens, what
    final = e.snapshot()
    bad = np.argwhere(final != final_cpu)
    assert bad.size == 0, (f"{what}: first wrong word (row, col) {tuple(bad[0])}: {final[tuple(bad[0])]:#010x} for "
                           f"{final_cpu[tuple(bad[0])]:#010x}, {len(bad)} wrong")


def oracle_run(board, W, gens, topology, rule, vis=None):
    return O.run_packed(board, W, gens, topology, rule, vis=vis, nthreads=1)


@pytest.mark.parametrize("block", S.WORD_BLOCKS, ids=lambda b: f"words{b[0]}-{b[-1]}")
def test_torus_widths(gpu, block):
    ran, strips = 0, {}
    for words in block:
        W = 32 * words
        rules = {"life": O.LIFE, "generic": S.generic_rule(words)}
        cases = S.torus_cases(words)
        for rule_name, G in sorted({c[:2] for c in cases}):
            H, gens = S.torus_height(G), G + 1
            board = O.seed_packed(W, H, 131 * words + G)
            ref = oracle_run(board, W, gens, O.TORUS, rules[rule_name])
            with GolEngine(W, H, rule=Rule(*rules[rule_name])) as e:
                for _, _, lanes, family in (c for c in cases if c[:2] == (rule_name, G)):
                    run_case(e, board, ref, gens, G, lanes, family, f"{words} words, {rule_name}, G = {G}, "
                             f"lanes {lanes}, {family}")
                    assert e.pass_plan(gens, family == "hashed") == [G, 1]
                    strips.setdefault((G, lanes), set()).add(e.occupancy(G)[1])
                    ran += 1
    assert ran == sum(S.torus_case_count(w) for w in block)
    for key, want in S.expected_strips(block).items():
        assert strips.get(key, set()) >= want, (key, strips.get(key), want)


@pytest.mark.parametrize("words", S.HEIGHT_WORDS)
def test_torus_heights(gpu, words):
    """Every height 1 .. 26 at every depth: tori shorter than the halo (rows <
    G, wrapping more than once), the 4-, 6- and 8-row band paths of the
    single-generation kernel, and everything between."""
    W = 32 * words
    ran = 0
    for H in S.HEIGHTS:
        board = O.seed_packed(W, H, 977 * words + H)
        with GolEngine(W, H) as e:
            for G in S.DEPTHS:
                ref = oracle_run(board, W, G + 1, O.TORUS, O.LIFE)
                for family in S.FAMILIES:
                    run_case(e, board, ref, G + 1, G, 0, family, f"{words} words x {H} rows, G = {G}, {family}")
                    ran += 1
    assert ran == len(S.HEIGHTS) * len(S.DEPTHS) * len(S.FAMILIES) == 624


def clipped_board(W, H):
    cells = (np.random.default_rng([W, H]).random((H, W)) < 0.5).astype(np.uint8)
    return O.pack(cells)


def run_clipped(W, rule, cases):
    """Cases [(H, vis, G, family)] of one stored width, one context per (H, vis); returns how many ran."""
    ran = 0
    for H, vis in sorted({c[:2] for c in cases}):
        # the rule gol_create accepts visible extents by, restated: vw in {W - 1, W}, vh in {H - 1, H} (0: the default
        # W - 1 / H - 1), a visible cell in each direction and more than one in all
        vw, vh = (vis[0] or W - 1), (vis[1] or H - 1)
        assert W - 1 <= vw <= W and H - 1 <= vh <= H and vw >= 1 and vh >= 1 and (vw, vh) != (1, 1)
        board = clipped_board(W, H)
        refs = {}
        with GolEngine(W, H, topology="ref-clipped", rule=Rule(*rule), vis=vis) as e:
            for _, _, G, family in (c for c in cases if c[:2] == (H, vis)):
                if G not in refs:
                    refs[G] = oracle_run(board, W, G + 1, O.REF_CLIPPED, rule, vis=(vw, vh))
                run_case(e, board, refs[G], G + 1, G, 0, family, f"{W} x {H} clipped, visible {vw} x {vh}, G = {G}, "
                         f"{family}")
                ran += 1
    return ran


@pytest.mark.parametrize("block", S.CLIPPED_BLOCKS, ids=lambda b: f"W{b[0]}-{b[-1]}")
def test_clipped_widths(gpu, block):
    """All 31 partial-word remainders over one to five words, and either side
    of the strip boundaries, at every visible-extent variant."""
    for W in block:
        variants = [(vw, vh) for vw in (W - 1, W) for vh in (S.CLIPPED_H - 1, S.CLIPPED_H)
                    if vw >= 1 and vh >= 1 and (vw, vh) != (1, 1)]
        assert len(variants) == 4  # a board two columns wide keeps all four
        assert run_clipped(W, S.clipped_rule(W), S.clipped_cases(W)) == S.clipped_case_count(W) == len(variants) * 12


def test_one_column_boards(gpu):
    """W = 1 with an explicit vis_width of 1: refused at the default extents
    (vis_width 0), accepted and stepped at these."""
    with pytest.raises(N.GolError) as ei:
        GolEngine(1, 9, topology="ref-clipped")
    assert ei.value.code == N.GOL_EINVAL
    assert run_clipped(1, O.LIFE, S.one_column_cases()) == S.ONE_COLUMN_COUNT
    assert run_clipped(1, O.REF_LITERAL, S.one_column_cases()) == S.ONE_COLUMN_COUNT


@pytest.mark.parametrize("W", S.CLIPPED_HEIGHT_WIDTHS)
def test_clipped_heights(gpu, W):
    assert run_clipped(W, S.clipped_rule(W), S.clipped_height_cases(W)) == S.CLIPPED_HEIGHT_COUNT


def test_two_by_two_default_extents_refused(gpu):
    with pytest.raises(N.GolError) as ei:
        GolEngine(2, 2, topology="ref-clipped")
    assert ei.value.code == N.GOL_EINVAL


@pytest.mark.parametrize("gpp", [1, 3, 6])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("vis", [(65, 23), (65, 22)], ids=lambda v: f"vis{v[0]}x{v[1]}")
def test_group_explicit_extents(gpu, vis, n, gpp):
    """Explicit visible extents on uneven row shards: row_visible compares
    grow0 + r with an explicit vis_rows on shards whose grow0 > 0."""
    W, H, gens = 65, 23, 2 * gpp + 1
    full = clipped_board(W, H)
    shards = []
    for k in range(n):
        r0, rows = shard_rows_py(H, k, n)
        e = GolEngine(W, H, topology="ref-clipped", row0=r0, rows=rows, vis=vis)
        e.set_tuning(gens_per_pass=gpp)
        e.load(full[r0:r0 + rows])
        shards.append(e)
    assert len({s.rows for s in shards}) == 2 and shards[-1].row0 > 0
    g = ShardGroup(shards)
    got = g.step(gens, hashes=True)
    board = g.snapshot()
    h = g.hash()
    g.close()
    for s in shards:
        s.close()
    ref, want = oracle_run(full, W, gens, O.REF_CLIPPED, O.LIFE, vis=vis)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(board, ref)
    assert h == int(want[-1])
