"""CPU: the pass schedule's pure functions (csrc/gol_plan.h: band plan of a
launch, XCD chunk, depth planner) through tests/schedule_probe.cpp, built with
plain g++ -- no HIP, no GPU.

* tests/golden/schedule.json: schedules recorded from the schedule code as it
  stood before the rules moved into gol_plan.h (its launches captured on the
  CPU), never from the code under test.  "band": per entry the resident waves
  `res`, the fixed band `br`, the GOL_TAIL override `tail` = [present, set,
  frac, div] and, per depth of `g`, the strips, the input ranges lo / hi and
  the result [row_lo0, row_hi0, band0, nbands0, row_lo1, row_hi1, band1,
  nbands1, waves, grid, small] (null: no launch).  "xcd": [gens, strips,
  override, chunk].  "plan": [n, cap, fixed depth, hashed row, wide,
  run-length depths].
* the schedules DESIGN.md section 4 states, as literals;
* invariants of every band plan and depth plan over a wider generated grid."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
WAVES_PER_WG = 4


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schedule") / "schedule_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "schedule_probe.cpp"), "-o", exe], check=True)

    def run(lines):
        p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = [[int(x) for x in l.split()] for l in p.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "schedule.json")) as f:
        return json.load(f)


def band_case(lo, hi, strips, gens, resident, band_rows=0, tail=(0, 0, 0, 0)):
    n = 2 if hi[1] != 0 else 1
    return (f"band {n} {lo[0]} {hi[0]} {lo[1]} {hi[1]} {strips} {gens} {resident} {band_rows} "
            f"{tail[0]} {tail[1]} {tail[2]!r} {tail[3]}")


def test_band_plans_match_the_recorded_schedules(probe, golden):
    assert golden["waves_per_wg"] == WAVES_PER_WG
    cases, want = [], []
    for e in golden["band"]:
        for i, G in enumerate(e["g"]):
            if e["out"][i] is None:  # a shard without interior rows: nothing launched
                assert e["hi"][i][0] <= e["lo"][i][0]
                continue
            cases.append(band_case(e["lo"][i], e["hi"][i], e["strips"][i], G, e["res"], e["br"], e["tail"]))
            want.append(e["out"][i])
    assert len(cases) >= 390  # the table was read whole
    got = probe(cases)
    wrong = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, wrong[:5]


def test_xcd_chunks_match_the_recorded_schedules(probe, golden):
    got = probe([f"xcd {g} {s} {env}" for g, s, env, _ in golden["xcd"]])
    assert [g[0] for g in got] == [chunk for _, _, _, chunk in golden["xcd"]]


def test_plans_match_the_recorded_schedules(probe, golden):
    got = probe([f"plan {n} {cap} {fixed} {hashed} {wide}" for n, cap, fixed, hashed, wide, _ in golden["plan"]])
    want = [[d for d, count in runs for _ in range(count)] for *_, runs in golden["plan"]]
    assert got == want


def test_known_schedules(probe):
    """DESIGN.md section 4 and the bench's boards, 3 resident blocks per CU on
    256 CUs (3072 waves), B3/S23 tori."""
    R = 3072
    got = probe([
        band_case([0, 0], [262144, 0], 67, 10, R),
        band_case([0, 0], [65536, 0], 17, 10, R),
        band_case([0, 0], [65536, 0], 17, 6, R),
        band_case([0, 0], [4096, 0], 1, 10, R),   # whole-row waves: one strip
        band_case([0, 0], [262144, 0], 32, 1, R),  # 16-byte lanes
        "xcd 10 67 0", "xcd 10 17 0", "xcd 1 32 0", "xcd 1 8 0",
        "plan 20 12 0 0 1", "plan 20 12 0 0 0", "plan 20 12 0 1 1", "plan 20 12 0 1 0",
        "plan 1024 12 0 0 0",
    ])
    # 1024-row bulk bands, the last resident round in quarter-height bands
    assert got[0] == [0, 250624, 1024, 245, 250624, 262144, 256, 45, (245 + 45) * 67, 4858, 0]
    assert got[1] == [0, 57976, 256, 227, 57976, 65536, 42, 180, (227 + 180) * 17, 1730, 0]
    assert got[2][:4] == [0, 65536, 137, 479] and got[2][7] == 0 and got[2][10] == 0
    assert got[3] == [0, 4096, 4, 1024, 0, 0, 4, 0, 1024, 256, 1]
    assert got[4][:4] == [0, 262144, 6, 43691] and got[4][7] == 0
    assert [g[0] for g in got[5:9]] == [8, 8, 32, 8]
    assert got[9] == got[10] == got[11] == [10, 10]
    assert sum(got[12]) == 20
    assert got[13] == [10] * 101 + [7] * 2


STRIPS = (1, 2, 17, 31, 32, 33, 67)
ROWS = (1, 2, 3, 7, 8, 63, 64, 65, 127, 256, 257, 997, 1024, 4096, 4099, 8191, 30001, 32768, 65521, 65536, 65537,
        131071, 131072, 262139, 262144)
RESIDENT = (0, 2048, 3072, 4096, 5120, 8192)


def ceil_div(a, b):
    return -(-a // b)


def test_band_plan_invariants(probe):
    keys = [(s, rows, G, res, br, tail)
            for s in STRIPS for rows in ROWS for G in range(1, 13) for res in RESIDENT
            for br, tail in ((0, (0, 0, 0, 0)), (0, (1, 1, 1.0, 3)), (37, (0, 0, 0, 0)))]
    plans = probe([band_case([0, 0], [rows, 0], s, G, res, br, tail) for s, rows, G, res, br, tail in keys])
    # the band the small-board cut replaces: the plain pick for the same inputs
    picks = probe([f"pick {br} {rows} {s} {G} {res if G > 1 else 0}" for s, rows, G, res, br, _ in keys])
    for (s, rows, G, res, br, tail), p, (picked,) in zip(keys, plans, picks):
        lo0, hi0, b0, n0, lo1, hi1, b1, n1, waves, grid, small = p
        ctx = (s, rows, G, res, br, tail, p)
        assert b0 >= 1 and b1 >= 1, ctx
        assert lo0 == 0 and n0 == ceil_div(hi0 - lo0, b0), ctx
        if n1:  # a tail: the ranges tile [0, rows) in order
            assert 0 < hi0 == lo1 < hi1 == rows and n1 == ceil_div(hi1 - lo1, b1), ctx
            t = hi1 - lo1
            assert 2 * t <= rows and t % b1 == 0 and b1 >= 8, ctx
            assert G > 1 and not small, ctx
        else:
            assert hi0 == rows, ctx
        if small:
            # a multiple of 4, >= 4, never taller than the band it replaces
            # (which itself is as short as the range on boards of 1-3 rows)
            assert b0 <= picked and ((b0 % 4 == 0 and b0 >= 4) or b0 == picked < 4), ctx
            assert n1 == 0 and br == 0, ctx
        else:
            assert b0 == picked, ctx
        assert waves == (n0 + n1) * s and grid == ceil_div(waves, WAVES_PER_WG), ctx


def test_two_range_plans_keep_their_ranges(probe):
    """The boundary blocks of a sharded pass: both ranges as given, one band
    height, no occupancy rule, no tail."""
    keys = [(s, rows, G, res) for s in STRIPS for rows in (25, 997, 32768, 262144) for G in range(1, 13)
            for res in (0, 3072)]
    plans = probe([band_case([0, rows - G], [G, rows], s, G, res) for s, rows, G, res in keys])
    for (s, rows, G, res), p in zip(keys, plans):
        lo0, hi0, b0, n0, lo1, hi1, b1, n1, waves, grid, small = p
        assert (lo0, hi0, lo1, hi1) == (0, G, rows - G, rows) and b0 == b1 >= 1 and not small, (s, rows, G, res, p)
        assert n0 == n1 == ceil_div(G, b0) and waves == 2 * n0 * s and grid == ceil_div(waves, WAVES_PER_WG)


def test_depth_plan_invariants(probe):
    keys = [(n, cap, fixed, hashed, wide)
            for n in (1, 2, 7, 11, 20, 102, 1000, 1024) for cap in range(1, 13) for fixed in (0, cap)
            for hashed in (0, 1) for wide in (0, 1)]
    plans = probe([f"plan {n} {cap} {fixed} {hashed} {wide}" for n, cap, fixed, hashed, wide in keys])
    for (n, cap, fixed, hashed, wide), plan in zip(keys, plans):
        assert sum(plan) == n and plan == sorted(plan, reverse=True), (n, cap, fixed, plan)
        assert all(1 <= d <= cap for d in plan), (n, cap, fixed, plan)
        if fixed:
            assert plan[:-1] == [cap] * (len(plan) - 1)
