"""CPU: active-row stepping's run arithmetic (csrc/gol_active.h: dilate,
subtract, from_bitmap, scan_due, dense) through tests/active_probe.cpp, built
with plain g++ -- no HIP, no GPU -- against a model written here from the
rules of DESIGN.md section 5c as sets of rows, and the three C-ABI entry
points' null-argument behaviour through ctypes."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")

ROWS = (8, 63, 64, 65, 512, 4096)
DEPTHS = (1, 2, 7, 12)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("active") / "active_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "active_probe.cpp"), "-o", exe], check=True)

    def run(lines):
        p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = [[int(x) for x in l.split()] for l in p.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture(scope="module")
def consts(probe):
    (block, max_runs, first_backoff, max_backoff), = probe(["consts"])
    return block, max_runs, (first_backoff, max_backoff)


def pairs(flat):
    assert len(flat) % 2 == 0
    return list(zip(flat[::2], flat[1::2]))


def fmt(runs):
    return f"{len(runs)} " + " ".join(f"{lo} {hi}" for lo, hi in runs)


def rowset(runs):
    return set(itertools.chain.from_iterable(range(lo, hi) for lo, hi in runs))


def check_shape(runs, rows, block, max_runs):
    """Sorted, disjoint (not even touching), inside [0, rows), block-aligned
    (the last run may end at `rows`), at most max_runs."""
    assert len(runs) <= max_runs
    prev = -1
    for lo, hi in runs:
        assert 0 <= lo < hi <= rows and lo > prev, (runs, rows)
        assert lo % block == 0 and (hi % block == 0 or hi == rows), (runs, rows)
        prev = hi


def input_runs(rows, block):
    """Run lists inside [0, rows): touching row 0, touching `rows`, both (the
    seam), adjacent, unaligned, empty, and more than kMaxRuns of them."""
    cases = [[], [(0, 1)], [(rows - 1, rows)], [(0, 1), (rows - 1, rows)], [(0, rows)],
             [(rows // 2, rows // 2 + 1)], [(rows // 3, rows // 3 + 2), (rows // 3 + 2, rows // 3 + 3)]]
    if rows > 2 * block:
        cases += [[(block, 2 * block)], [(block - 1, block + 1)], [(0, block), (block, 2 * block)],
                  [(rows - block - 3, rows - 2)], [(5, 9), (rows - 9, rows - 5)]]
    if rows >= 4096:
        # 10 single rows 2, 3, 4 ... blocks apart: the cap must close the smallest gaps
        many, at = [], 10
        for k in range(10):
            many.append((at, at + 1))
            assert at < rows
            at += (k + 2) * block
        cases += [many, [(k * 5 * block + 7, k * 5 * block + 70) for k in range(12)]]
    return [c for c in cases if all(0 <= lo < hi <= rows for lo, hi in c)]


def test_dilate_covers_every_row_within_reach(probe, consts):
    block, max_runs, _ = consts
    keys = [(rows, G, wrap, runs) for rows in ROWS for G in DEPTHS for wrap in (0, 1)
            for runs in input_runs(rows, block)]
    got = probe([f"dilate {rows} {G} {wrap} {fmt(runs)}" for rows, G, wrap, runs in keys])
    assert len(keys) > 400
    for (rows, G, wrap, runs), flat in zip(keys, got):
        out = pairs(flat)
        check_shape(out, rows, block, max_runs)
        want = set()
        for r in rowset(runs):
            for d in range(-G, G + 1):
                if wrap:
                    want.add((r + d) % rows)
                elif 0 <= r + d < rows:
                    want.add(r + d)
        assert want <= rowset(out), (rows, G, wrap, runs, out)
        if not runs:
            assert out == []


def test_dilate_stays_tight_when_runs_are_few(probe, consts):
    """With at most kMaxRuns / 2 input runs nothing is merged for the cap: the
    result is exactly the blocks that hold a row within reach."""
    block, max_runs, _ = consts
    keys = [(rows, G, wrap, runs) for rows in ROWS for G in DEPTHS for wrap in (0, 1)
            for runs in input_runs(rows, block) if 2 * len(runs) <= max_runs]
    got = probe([f"dilate {rows} {G} {wrap} {fmt(runs)}" for rows, G, wrap, runs in keys])
    for (rows, G, wrap, runs), flat in zip(keys, got):
        blocks = set()
        for lo, hi in runs:
            for r in (range(lo - G, hi + G)):
                if wrap or 0 <= r < rows:
                    blocks.add((r % rows) // block)
        want = set()
        for b in blocks:
            want |= set(range(b * block, min((b + 1) * block, rows)))
        assert rowset(pairs(flat)) == want, (rows, G, wrap, runs, pairs(flat))


def test_dilate_at_the_seam(probe, consts):
    """A run at row 0 of a torus yields [rows - G, rows) and [0, hi + G),
    block-aligned; a clipped board clamps instead."""
    block, *_ = consts
    (torus, clipped) = probe([f"dilate 4096 7 1 1 0 {block}", f"dilate 4096 7 0 1 0 {block}"])
    assert pairs(torus) == [(0, 2 * block), (4096 - block, 4096)]
    assert pairs(clipped) == [(0, 2 * block)]


def test_the_cap_closes_the_smallest_gaps(probe, consts):
    block, max_runs, _ = consts
    rows = 8 * max_runs * block
    # max_runs + 1 single-block runs three blocks apart, but for one gap of a single block
    at = [4 * k for k in range(max_runs)] + [4 * (max_runs - 1) + 2]
    runs = [(b * block + 3, b * block + 4) for b in at]
    (flat,) = probe([f"normalize {rows} {fmt(runs)}"])
    out = pairs(flat)
    check_shape(out, rows, block, max_runs)
    assert out == [(b * block, (b + 1) * block) for b in at[:max_runs - 1]] + [(at[-2] * block, (at[-1] + 1) * block)]


def test_subtract_splits_a(probe, consts):
    block, *_ = consts
    keys = []
    for rows in ROWS:
        ins = input_runs(rows, block)
        norm = [pairs(f) for f in probe([f"normalize {rows} {fmt(r)}" for r in ins])]
        dil = [pairs(f) for f in probe([f"dilate {rows} 7 1 {fmt(r)}" for r in ins])]
        raw = [sorted(r) for r in ins if len(r) <= 2]  # sorted and disjoint, not aligned
        lists = norm + dil + raw
        keys += [(a, b) for a in lists for b in lists]
    got = probe([f"subtract {fmt(a)} {fmt(b)}" for a, b in keys])
    assert len(keys) > 2000
    for (a, b), flat in zip(keys, got):
        out = pairs(flat)
        sa, sb, so = rowset(a), rowset(b), rowset(out)
        assert so == sa - sb, (a, b, out)
        assert so | (sa & sb) == sa and not (so & sb)
        assert all(lo < hi for lo, hi in out) and all(x[1] <= y[0] for x, y in zip(out, out[1:])), (a, b, out)


def test_from_bitmap_round_trips(probe, consts):
    block, max_runs, _ = consts
    keys = []
    for rows in ROWS:
        nblocks = -(-rows // block)
        patterns = {0, 1, (1 << nblocks) - 1, 1 << (nblocks - 1), 0b1011 & ((1 << nblocks) - 1),
                    int("10" * 32, 2) & ((1 << nblocks) - 1), int("1100111" * 10, 2) & ((1 << nblocks) - 1)}
        keys += [(rows, nblocks, m) for m in sorted(patterns)]
    lines = []
    for rows, nblocks, m in keys:
        words = [(m >> (32 * k)) & 0xFFFFFFFF for k in range(-(-nblocks // 32))]
        lines.append(f"bitmap {rows} 0 {nblocks} {len(words)} " + " ".join(map(str, words)))
    for (rows, nblocks, m), flat in zip(keys, probe(lines)):
        out = pairs(flat)
        check_shape(out, rows, block, max_runs)
        want = set()
        for b in range(nblocks):
            if (m >> b) & 1:
                want |= set(range(b * block, min((b + 1) * block, rows)))
        assert want <= rowset(out), (rows, bin(m), out)
        if bin(m).count("1") <= max_runs:  # nothing merged for the cap: exact, and back to the same bitmap
            assert rowset(out) == want, (rows, bin(m), out)
            back = 0
            for lo, hi in out:
                for b in range(lo // block, -(-hi // block)):
                    back |= 1 << b
            assert back == m
    # an offset bitmap: bit k is block lo_block + k
    (flat,) = probe([f"bitmap 4096 5 3 1 {0b101}"])
    assert pairs(flat) == [(5 * block, 6 * block), (7 * block, 8 * block)]


def test_scan_and_dense_thresholds(probe, consts):
    block, _, (first_backoff, max_backoff) = consts
    cases = [(now, last) for last in (0, 1, block, 3 * block, 1000) for now in
             (0, last, 2 * last + 4 * block - 1, 2 * last + 4 * block, 2 * last + 4 * block + 1, 10 ** 9)]
    got = probe([f"due {now} {last}" for now, last in cases])
    assert [g[0] for g in got] == [int(now >= 2 * last + 4 * block) for now, last in cases]
    cases = [(launched, rows) for rows in (1, 2, 7, 8, 512, 4097) for launched in
             (0, rows // 2, rows // 2 + 1, rows)]
    got = probe([f"dense {launched} {rows}" for launched, rows in cases])
    assert [g[0] for g in got] == [int(launched > rows // 2) for launched, rows in cases]
    # each wait longer than the last until the cap: a dense board is scanned ever less often
    waits, b = [], 0
    for _ in range(10):
        (b,), = probe([f"backoff {b}"])
        waits.append(b)
    assert waits[0] == first_backoff >= 1 and waits[-1] == waits[-2] == max_backoff >= 64
    assert all(y > x or x == max_backoff for x, y in zip(waits, waits[1:]))


# ---- the C ABI, without a device ------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from gameoflife import _native as N
    return N


def test_the_entry_points_exist(lib):
    for name in ("gol_set_active_rows", "gol_active_stats_read", "gol_active_rows"):
        assert hasattr(lib.lib, name), name
        assert name in lib.header_symbols()


def test_null_arguments_are_refused_without_a_device(lib):
    st = lib.GolActiveStats()
    n = ctypes.c_int32(7)
    buf = (ctypes.c_int64 * 2)()
    assert lib.lib.gol_set_active_rows(None, 1) == lib.GOL_EINVAL
    assert lib.lib.gol_active_stats_read(None, ctypes.byref(st), 0) == lib.GOL_EINVAL
    assert lib.lib.gol_active_rows(None, buf, 1, ctypes.byref(n)) == lib.GOL_EINVAL
    assert n.value == 7


def test_the_abi_version_stays(lib):
    assert lib.lib.gol_abi_version() == 2 == lib.GOL_ABI_VERSION
