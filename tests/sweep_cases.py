"""The cases of the two geometry sweeps (tests/test_gpu_batch_sweep.py,
tests/test_gpu_width_sweep.py) -- test infrastructure,
no device.  Everything the GPU tests enumerate, count and compare with lives
here, so that tests/test_sweep_cases.py can check it without a GPU: the
enumerations against the validators, the counts in closed form, and the
comparison functions against models corrupted on purpose.

Batch engine: every geometry gol_batch_geometry_get accepts.  Shard engine:
every row width up to two strips of the widest lanes, every short height."""
import numpy as np

import batch_model as M
import batch_rules_model as R
import cycle_model as C
from oracle import oracle as O

# ---------------------------------------------------------------- batch engine

MAX_SIDE = 64
SWEEP_GENS = 6
SETTLE_GENS = 40
CYCLE_GENS = 96  # crosses the snapshots at generations 1, 3, 7, 15, 31 and 63
LONG_WIDTHS = (31, 32, 33, 47, 64)  # and the smallest width the validator accepts
# the uniform generic instance: one rule with a birth on 0 neighbours, one without
UNIFORM_RULES = ((0x049, 0x16E), (0x048, 0x00C))  # B036/S123568, B36/S23


def clipped_variants(W, H):
    """The visible extents a ref-clipped board of W x H stored cells runs
    with: vw in {W - 1, W}, vh in {H - 1, H}, some cell visible in each
    direction and more than one visible cell.  The default extents are given
    as (0, 0) -- the same board as (W - 1, H - 1) -- so that the defaulting
    runs too."""
    out = []
    for vw in (W - 1, W):
        for vh in (H - 1, H):
            if vw >= 1 and vh >= 1 and (vw, vh) != (1, 1):
                out.append((0, 0) if (vw, vh) == (W - 1, H - 1) else (vw, vh))
    return out


def batch_geometries(topology, height=None):
    """[(W, H, vis)]: every geometry of the batch engine, or those of one height."""
    heights = range(1, MAX_SIDE + 1) if height is None else (height,)
    out = []
    for H in heights:
        for W in range(1, MAX_SIDE + 1):
            if topology == "torus":
                if W >= 3 and H >= 3:
                    out.append((W, H, (0, 0)))
            else:
                out.extend((W, H, vis) for vis in clipped_variants(W, H))
    return out


def batch_geometry_count(topology, height=None):
    """len(batch_geometries(...)) in closed form.  Torus: 62 widths for each of
    62 heights.  Clipped: over the 64 widths there are 127 visible widths (W = 1
    has one), over the heights likewise; the visible width 1 occurs twice (W =
    1 and 2) and meets a visible height 1 once at H = 1 and once at H = 2."""
    if height is not None:
        if topology == "torus":
            return 62 if 3 <= height <= MAX_SIDE else 0
        return 127 * (2 if height >= 2 else 1) - (2 if height <= 2 else 0)
    return 62 * 62 if topology == "torus" else 127 * 127 - 4


def visible(W, H, topology, vis):
    """The extents a model steps with: None on a torus and for the default."""
    return None if topology == "torus" or tuple(vis) == (0, 0) else tuple(vis)


def explicit_extents(W, H, vis):
    """(vw, vh) of a ref-clipped board's visible extents, the default spelled out."""
    return (W - 1, H - 1) if tuple(vis) == (0, 0) else tuple(vis)


def batch_boards(H):
    """One full wave (k = 64 // H boards) and a last wave of one board."""
    return MAX_SIDE // H + 1


def batch_seed(W, H):
    return 0x5EED0000 + 977 * W + H


def batch_rule_words(W, H):
    """uint32 [batch_boards(H)]: one rule word per board from an rng seeded by
    (W, H); board W % n has a birth on 0 neighbours whatever was drawn."""
    n = batch_boards(H)
    rng = np.random.default_rng([W, H])
    words = (rng.integers(0, 1 << 32, n, dtype=np.uint64) & np.uint64(R.WORD_BITS)).astype(np.uint32)
    words[W % n] |= np.uint32(1)
    return words


def uniform_rule(W, H):
    return UNIFORM_RULES[(W + H) % 2]


def long_run_geometries(topology, H):
    """[(W, H, vis)] of the longer runs of one height: the smallest width the
    validator accepts and LONG_WIDTHS; tori as they are, clipped boards at the
    default extents and at (W, H)."""
    geoms = batch_geometries(topology, H)
    if topology == "torus":
        kinds = [geoms]
    else:
        kinds = [[g for g in geoms if g[2] == (0, 0)], [g for g in geoms if g[2] == (g[0], g[1])]]
    out = []
    for mine in kinds:
        if mine:  # a clipped board one row high has no default extents
            widths = {min(g[0] for g in mine), *LONG_WIDTHS}
            out.extend(g for g in mine if g[0] in widths)
    return out


def long_run_count(topology, H):
    """len(long_run_geometries(...)) in closed form: six widths, twice on a
    clipped board of two rows or more (its default extents and (W, H))."""
    return (1 + len(LONG_WIDTHS)) * (1 if topology == "torus" or H == 1 else 2)


def mismatch(got, want):
    """None if every array of `got` equals its namesake in `want` bit for bit,
    else a line naming the first that does not and its first wrong element.
    The one comparison of the batch sweep."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{name}: {g.dtype}{g.shape} for {w.dtype}{w.shape}"
        bad = np.argwhere(g != w)
        if bad.size:
            at = tuple(int(i) for i in bad[0])
            return f"{name}{list(at)}: {int(g[at]):#x} for {int(w[at]):#x} ({len(bad)} wrong)"
    return None


def stepper(topology, rule, vis):
    """The true model's step of one uint8 [H][W] board."""
    return lambda cells: M.step_board(cells, topology, rule, vis)


def history_with(step, rows, W, gens):
    """batch_model.run_history with the step handed in (the corrupted models
    of tests/test_sweep_cases.py): (states, populations, settled)."""
    cells = M.unpack(rows, W)
    n, H = cells.shape[0], cells.shape[1]
    states = np.zeros((gens + 1, n, H), dtype=np.uint64)
    pops = np.zeros((n, gens), dtype=np.uint32)
    settled = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        hist = [cells[i]]
        for _ in range(gens):
            hist.append(step(hist[-1]))
        states[:, i] = M.pack(np.stack(hist))
        pops[i] = [int(h.sum()) for h in hist[1:]]
        settled[i] = M.settled_at(hist)
    return states, pops, settled


def sweep_result(states, pops, settled, W):
    """What the sweep compares of a run: the arrays `mismatch` takes."""
    return {"final": states[-1], "populations": pops, "settled": settled, "hashes": M.hashes(states[-1], W),
            "population": pops[:, -1].copy()}


def expected_uniform(geometry, topology, rule, step=None):
    """The model's sweep_result of the seeded boards of one geometry under one
    rule; `step`: a step of one board in place of the true one."""
    W, H, vis = geometry
    rows = M.seed_rows(batch_boards(H), W, H, batch_seed(W, H))
    if step is None:
        out = M.run_history(rows, W, SWEEP_GENS, topology, rule, visible(W, H, topology, vis))
    else:
        out = history_with(step, rows, W, SWEEP_GENS)
    return sweep_result(*out, W)


def expected_rules(geometry, topology):
    """The model's {final, populations} of the seeded boards under batch_rule_words."""
    W, H, vis = geometry
    rows = M.seed_rows(batch_boards(H), W, H, batch_seed(W, H))
    states, pops, _ = R.run_history(rows, W, SWEEP_GENS, batch_rule_words(W, H), topology,
                                    visible(W, H, topology, vis))
    return {"final": states[-1], "populations": pops}


def expected_long(geometry, topology):
    """The model's longer runs of one geometry, B3/S23: ({final, settled} after
    SETTLE_GENS, {final, period, seen} after CYCLE_GENS)."""
    W, H, vis = geometry
    v = visible(W, H, topology, vis)
    rows = M.seed_rows(batch_boards(H), W, H, batch_seed(W, H))
    final, _, settled = M.run(rows, W, SETTLE_GENS, topology, O.LIFE, v)
    cfinal, period, seen = C.run(rows, W, CYCLE_GENS, topology, O.LIFE, v)
    return {"final": final, "settled": settled}, {"final": cfinal, "period": period, "seen": seen}


def step_all_visible(rule):
    """A corrupted clipped model: the visible extents ignored, every stored cell visible."""
    return lambda cells: O.step_cells(cells, O.REF_CLIPPED, rule, vis=(cells.shape[1], cells.shape[0]))


def step_wrap_bit_off_by_one(rule):
    """A corrupted torus model: the cell west of column 0 read from bit `width`
    of the row (always dead) instead of bit width - 1."""
    birth = np.array([(rule[0] >> k) & 1 for k in range(9)], dtype=np.uint8)
    survive = np.array([(rule[1] >> k) & 1 for k in range(9)], dtype=np.uint8)

    def step(cells):
        c = np.asarray(cells, dtype=np.int32)
        # west of column 0: dead; east of column W - 1: column 0
        wide = np.concatenate([np.zeros_like(c[:, :1]), c, c[:, :1]], axis=1)
        tall = np.concatenate([wide[-1:], wide, wide[:1]], axis=0)
        H, W = c.shape
        n = sum(tall[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if (dx, dy) != (0, 0))
        return np.where(c == 1, survive[n], birth[n]).astype(np.uint8)
    return step


# ---------------------------------------------------------------- shard engine

DEPTHS = tuple(range(1, 13))
WORDS = tuple(range(1, 261))                 # every word count up to 260
WORDS_VEC4 = tuple(range(264, 521, 4))       # and on to 520 under forced 16-byte lanes
FORCED_DEPTHS_LIFE = (1, 2, 7, 12)
FORCED_DEPTHS_GENERIC = (1, 2, 7)            # gol_set_tuning refuses 16-byte lanes deeper than 7 off the B3/S23 torus
GENERIC_DEPTHS = (1, 3, 8, 12)
FAMILIES = ("hashed", "unhashed")            # step(hashes=True) / the unhashed step
WORD_BLOCKS = tuple(WORDS[i:i + 10] for i in range(0, len(WORDS), 10)) + (WORDS_VEC4[:33], WORDS_VEC4[33:])
HEIGHT_WORDS = (1, 2, 3, 124, 125)
HEIGHTS = tuple(range(1, 27))
CLIPPED_DEPTHS = (1, 2, 3, 5, 8, 12)
CLIPPED_WIDTHS = tuple(range(2, 131)) + tuple(32 * w + r for w in (61, 62, 63, 64, 123, 124, 125)
                                              for r in (0, 1, 17, 31))
CLIPPED_BLOCKS = tuple(CLIPPED_WIDTHS[i:i + 16] for i in range(0, len(CLIPPED_WIDTHS), 16))
CLIPPED_H = 9
ONE_COLUMN_HEIGHTS = (2, 3, 9)
CLIPPED_HEIGHTS = tuple(range(2, 27))
CLIPPED_HEIGHT_WIDTHS = (7, 33)
CLIPPED_HEIGHT_DEPTHS = (1, 5, 12)


def torus_height(G):
    return 2 * G + 3


def forced_lanes(words):
    """The forced words per lane a row of `words` words is swept with."""
    if words > WORDS[-1]:
        return (4,) if words in WORDS_VEC4 else ()
    return tuple(v for v in (1, 2, 4) if words % v == 0)


def generic_rule(words):
    """(birth, survive) masks from an rng seeded by the word count."""
    rng = np.random.default_rng(words)
    return int(rng.integers(0, 512)), int(rng.integers(0, 512))


def torus_cases(words):
    """[(rule, G, lanes, family)] of one row width of the torus sweep; rule is
    "life" or "generic", lanes 0 (automatic), 1, 2 or 4.  Every case runs G + 1
    generations on a 32 * words x torus_height(G) torus."""
    out = []
    if words <= WORDS[-1]:
        out += [("life", G, 0, f) for G in DEPTHS for f in FAMILIES]
        out += [("generic", G, 0, FAMILIES[words % 2]) for G in GENERIC_DEPTHS]
    for v in forced_lanes(words):
        out += [("life", G, v, f) for G in FORCED_DEPTHS_LIFE for f in FAMILIES]
        out += [("generic", G, v, f) for G in FORCED_DEPTHS_GENERIC for f in FAMILIES]
    return out


def torus_case_count(words):
    """len(torus_cases(words)) in closed form: 12 depths twice and 4 generic
    depths once under automatic lanes, 4 + 3 depths twice per forced lane width."""
    lanes = (words % 1 == 0) + (words % 2 == 0) + (words % 4 == 0) if words <= 260 else int(words % 4 == 0)
    return (12 * 2 + 4 if words <= 260 else 0) + lanes * (4 + 3) * 2


# over WORDS and WORDS_VEC4: 260 rows of 28, forced lanes on 260 + 130 + 65 + 65 rows of 14
TORUS_CASES = 260 * 28 + (260 + 130 + 65 + 65) * 14


def engine_variants(W, H):
    """The visible extents gol_create accepts of {W - 1, W} x {H - 1, H} on a
    ref-clipped board (restated from it: every stored cell needs a visible
    neighbour), the default as (0, 0)."""
    return clipped_variants(W, H)


def clipped_rule(W):
    return O.LIFE if W % 2 == 0 else O.REF_LITERAL


def clipped_cases(W):
    """[(H, vis, G, family)] of one stored width of the clipped sweep, G + 1 generations each."""
    return [(CLIPPED_H, vis, G, f) for vis in engine_variants(W, CLIPPED_H) for G in CLIPPED_DEPTHS for f in FAMILIES]


def clipped_case_count(W):
    """Four visible-extent variants (a board two columns wide keeps them all), six depths, two families."""
    assert W >= 2
    return 4 * 6 * 2


def one_column_cases():
    """[(H, vis, G, family)] of the one-column boards: W = 1 with an explicit vis_width of 1."""
    return [(H, (1, vh), G, f) for H in ONE_COLUMN_HEIGHTS for vh in (H - 1, H) if vh != 1
            for G in CLIPPED_DEPTHS for f in FAMILIES]


ONE_COLUMN_COUNT = (1 + 2 + 2) * 6 * 2


def clipped_height_cases(W):
    """[(H, vis, G, family)]: heights 2 .. 26 at the default and the (W, H) extents."""
    return [(H, vis, G, f) for H in CLIPPED_HEIGHTS for vis in ((0, 0), (W, H)) for G in CLIPPED_HEIGHT_DEPTHS
            for f in FAMILIES]


CLIPPED_HEIGHT_COUNT = 25 * 2 * 3 * 2


def expected_strips(words_block):
    """{(G, lanes): strip widths} that a block of the torus sweep must meet
    through gol_occupancy: 62-word strips on an odd and 124 on an even word
    count at every G >= 2, the whole-row wave's 128 at G = 10 on the 128-word
    row, 248 under forced 16-byte lanes, and at G = 1 the 64, 128 and 256 of
    the three forced lane widths."""
    want = {}
    odd = any(w % 2 for w in words_block if w <= 260)
    even = any(w % 2 == 0 for w in words_block if w <= 260)
    for G in DEPTHS[1:]:
        want[(G, 0)] = ({62} if odd else set()) | ({124} if even else set())
    if 128 in words_block:
        want[(10, 0)] = want[(10, 0)] | {128}
    if any(4 in forced_lanes(w) for w in words_block):
        for G in FORCED_DEPTHS_LIFE[1:]:
            want[(G, 4)] = {248}
        want[(1, 4)] = {256}
    if odd:
        want[(1, 1)] = {64}
    if even:
        want[(1, 2)] = {128}
    return want
