"""CPU: the accounting of pass timing (csrc/gol_profile.h: slot_clock_ghz,
add, clock_ghz) through tests/profile_probe.cpp, built with plain g++ -- no
HIP, no GPU.  Every expected figure is a literal worked out by hand from the
rules in include/gol.h's gol_profile_stats comment; the inputs are binary
fractions, so the sums are exact."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")

FIELDS = ("kernel_ms", "launches", "generations", "exchange_ms", "exchanges", "boundary_ms", "boundary_launches",
          "exchange_exposed_ms", "pass_tail_ms", "clock_ghz")
NONE = "0 0 0 0"  # a part that was not timed


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("profile") / "profile_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "profile_probe.cpp"), "-o", exe], check=True)

    def run(lines):
        p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        return [[float(x) for x in l.split()] for l in p.stdout.splitlines()]
    return run


def totals(probe, passes):
    """The totals after `passes` (main ms ghz gens | exchange | boundary, each part timed ms tied after)."""
    (out,) = probe([f"pass {p}" for p in passes] + ["totals"])
    return dict(zip(FIELDS, out))


def test_a_part_that_ended_before_the_main_launch_adds_nothing(probe):
    t = totals(probe, ["1 1.0 2.0 4  1 0.5 1 -0.25  1 0.125 1 -1.0"])
    assert t == dict(kernel_ms=1.0, launches=1, generations=4, exchange_ms=0.5, exchanges=1, boundary_ms=0.125,
                     boundary_launches=1, exchange_exposed_ms=0.0, pass_tail_ms=0.0, clock_ghz=2.0)


def test_the_exposed_exchange_is_capped_at_the_exchange(probe):
    # the exchange ended 0.75 ms after the interior but lasted 0.5 ms; the tail has no cap
    t = totals(probe, ["1 1.0 2.0 1  1 0.5 1 0.75  1 0.25 1 0.75"])
    assert t["exchange_exposed_ms"] == 0.5 and t["pass_tail_ms"] == 0.75
    assert t["exchange_ms"] == 0.5 and t["boundary_ms"] == 0.25


def test_the_exposed_parts_sum_over_passes(probe):
    t = totals(probe, ["1 1.0 2.0 1  1 0.5 1 0.25  1 0.25 1 0.375",    # inside the exchange: 0.25; tail 0.375
                       "1 1.0 2.0 1  1 0.5 1 -0.5  1 0.25 1 0.125",    # hidden: 0; tail 0.125
                       "1 1.0 2.0 1  1 0.5 1 2.0  1 0.25 1 -0.125"])   # capped: 0.5; tail 0
    assert t["exchange_exposed_ms"] == 0.75 and t["pass_tail_ms"] == 0.5
    assert t["exchanges"] == 3 and t["boundary_launches"] == 3 and t["launches"] == 3 and t["generations"] == 3
    assert t["exchange_ms"] == 1.5 and t["boundary_ms"] == 0.75 and t["kernel_ms"] == 3.0


def test_untied_parts_add_their_time_and_count_only(probe):
    # `after` of an untied part means nothing, whatever it holds
    t = totals(probe, ["1 1.0 2.0 2  1 0.5 0 9.0  1 0.25 0 9.0",
                       f"0 0 0 0  1 0.5 0 0  {NONE}",     # an exchange alone (its pass's launch failed)
                       f"0 0 0 0  {NONE}  1 0.25 0 0"])   # a boundary launch alone (a group shard's)
    assert t["exchange_exposed_ms"] == 0.0 and t["pass_tail_ms"] == 0.0
    assert t["exchange_ms"] == 1.0 and t["exchanges"] == 2 and t["boundary_ms"] == 0.5 and t["boundary_launches"] == 2
    assert t["launches"] == 1 and t["generations"] == 2 and t["kernel_ms"] == 1.0


def test_a_launch_without_a_clock_counts_in_the_time_only(probe):
    t = totals(probe, [f"1 1.0 2.0 3  {NONE}  {NONE}", f"1 4.0 0.0 5  {NONE}  {NONE}"])
    assert t["kernel_ms"] == 5.0 and t["launches"] == 2 and t["generations"] == 8
    assert t["clock_ghz"] == 2.0  # not (2.0 * 1 + 0 * 4) / 5
    assert t["exchanges"] == 0 and t["boundary_launches"] == 0


def test_the_clock_is_weighted_by_launch_time(probe):
    # (2.0 GHz * 1 ms + 2.5 GHz * 3 ms) / 4 ms
    t = totals(probe, [f"1 1.0 2.0 1  {NONE}  {NONE}", f"1 3.0 2.5 1  {NONE}  {NONE}"])
    assert t["clock_ghz"] == 2.375


def test_no_clocked_launch_reports_zero(probe):
    assert totals(probe, [])["clock_ghz"] == 0.0
    assert totals(probe, [f"1 1.0 0.0 1  {NONE}  {NONE}"])["clock_ghz"] == 0.0
    # a main launch that was not timed leaves no clock either, whatever its slot held
    t = totals(probe, [f"0 1.0 2.0 7  {NONE}  {NONE}"])
    assert t["clock_ghz"] == 0.0 and t["launches"] == 0 and t["generations"] == 0 and t["kernel_ms"] == 0.0


def test_totals_start_again_from_nothing(probe):
    first, second = probe(["pass 1 1.0 2.0 4  1 0.5 1 0.25  1 0.25 1 0.5", "totals", "totals"])
    assert first[0] == 1.0 and second == [0.0] * len(FIELDS)


def test_slot_clock(probe):
    # 64 sub-slots of 8 words: word 0 core-clock ticks, word 1 100 MHz reference ticks (gol_kernels.h)
    (consts,) = probe(["consts"])
    assert consts == [64, 8, 512]

    def slot(words):
        (ghz,), = probe([f"slot {len(words)} " + " ".join(f"{w} {v}" for w, v in words.items())])
        return ghz
    assert slot({}) == 0.0                       # nothing reported
    assert slot({0: 12345, 8: 99}) == 0.0        # no reference tick counted: no clock, not a division by zero
    assert slot({0: 2400, 1: 100}) == pytest.approx(2.4, rel=1e-12)  # 24 core ticks per 10 ns
    # every sub-slot is summed: 63 report 20 ticks per reference tick, the last one 84 -> 1344 / 64 = 21
    words = {}
    for k in range(64):
        words[8 * k], words[8 * k + 1] = (84 if k == 63 else 20), 1
        words[8 * k + 2] = words[8 * k + 7] = 10 ** 15  # the rest of a sub-slot's line is not read
    assert slot(words) == pytest.approx(2.1, rel=1e-12)
