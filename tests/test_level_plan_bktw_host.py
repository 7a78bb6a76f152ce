"""CPU: the planner's wide-form fields (quick-adc_amd/host/level_plan.hpp, driver tests/cpp/level_plan_bktw_host.cpp).

The driver plans every case twice, with and without copies, and checks launch by launch: LevelLaunch::bktw is set exactly when every
run of a split launch covers whole octaves that are all stored wide and has bktw_min_run codes; LevelLaunch::bkt exactly when
every run covers whole narrow blocks and meets no wide octave; a launch that mixes them, or touches a wide octave without
covering whole ones, equals today's plan field for field.  Here: known cases (the headline among them) and a sweep of sizes, W,
fallback masks, level options and probe orders."""
import os
import subprocess

import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "level_plan_bktw_host")
TILE = 16384


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "level_plan_bktw_host.cpp"), EXE, link=False)
    return EXE


def plan(exe, sizes, W, orders, block=TILE, fallback=0, level_base=16384, growth=4, head_level=0, min_run=1, t5=0, t4=0, t3=0,
         small_run=1, share_variant=0):
    args = [",".join(str(s) for s in sizes), block, W, fallback, level_base, growth, head_level, min_run, t5, t4, t3, len(orders),
            ";".join(" ".join(str(p) for p in o) for o in orders), small_run, share_variant]
    out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    words = out.stdout.decode().split()
    assert out.returncode == 0 and words and words[0] == "ok", (args, out.stdout, out.stderr)
    return tuple(int(w) for w in words[1:5]) + (words[5],)    # launches, wide launches, wide runs, narrow launches, paid planes


def test_known_cases(driver):
    n = 12 * TILE + 37
    # W = one tile: level 0 narrow, levels [1, 4) and [4, 12 + 37) cover two octaves each
    assert plan(driver, [n], TILE, [[0]]) == (3, 2, 2, 1, "66")
    # W = two tiles: level 1 starts one tile before the first octave: neither form (it meets a wide octave); level 2 is wide
    assert plan(driver, [n], 2 * TILE, [[0]]) == (3, 1, 1, 1, "6")
    # W = 0 or beyond the partition: narrow everywhere
    assert plan(driver, [n], 0, [[0]]) == (3, 0, 0, 3, "-")
    assert plan(driver, [n], 16 * TILE, [[0]]) == (3, 0, 0, 3, "-")
    # the last octave fell back: level 2 covers a wide and a narrow octave: neither form
    assert plan(driver, [n], TILE, [[0]], fallback=0b1000) == (3, 1, 1, 1, "6")
    # octaves 2 and 3 fell back: level 2 lies on narrow blocks only
    assert plan(driver, [n], TILE, [[0]], fallback=0b1100) == (3, 1, 1, 2, "6")
    # every octave fell back: no wide copy
    assert plan(driver, [n], TILE, [[0]], fallback=0b1111) == (3, 0, 0, 3, "-")
    # thresholds: the runs have 3 and 8 tiles (+ 37)
    assert plan(driver, [n], TILE, [[0]], t5=3 * TILE, t4=3 * TILE + 1)[4] == "54"
    assert plan(driver, [n], TILE, [[0]], t3=8 * TILE)[4] == "63"
    assert plan(driver, [n], TILE, [[0]], min_run=3 * TILE + 1, t4=1) == (3, 1, 1, 1, "4")
    assert plan(driver, [n], TILE, [[0]], min_run=0) == (3, 0, 0, 1, "-")
    # two queries that probe two partitions in opposite orders: level 1 is one wide launch of two runs; level 2 mixes whole
    # partitions (they start at 0) with a narrow tail: today's plan
    assert plan(driver, [4 * TILE, 4 * TILE + 37], TILE, [[0, 1], [1, 0]], fallback=0b100) == (3, 1, 2, 1, "6")
    # a shared launch never takes the form
    assert plan(driver, [n], TILE, [[0], [0]], share_variant=0x41)[1] == 0
    # the headline: 10^9 codes, blocks of 2^25, W = 2^27, level base 512 x 4^k behind a head of 5 levels: the level from 2^25 plans
    # narrow (three blocks below W), the levels from 2^27 (two octaves) and 2^29 (the clipped octave) wide, 4 paid planes
    assert plan(driver, [10 ** 9], 1 << 27, [[0]] * 2, block=1 << 25, level_base=512, head_level=5, min_run=1 << 27, t5=1 << 27,
                t4=1 << 27, small_run=1 << 17) == (7, 2, 4, 1, "44")
    # ... and with the octave from 2^28 fallen back the level from 2^27 has no bucket form at all, the level from 2^29 stays wide
    assert plan(driver, [10 ** 9], 1 << 27, [[0]] * 2, block=1 << 25, fallback=0b010, level_base=512, head_level=5, min_run=1 << 27,
                t4=1 << 27, small_run=1 << 17) == (7, 1, 2, 1, "4")


@pytest.mark.parametrize("W", [TILE, 2 * TILE, 8 * TILE])
@pytest.mark.parametrize("growth", [2, 4])
def test_sweep(driver, W, growth):
    wide = 0
    for sizes in ([W + 1], [3 * W], [4 * W + 37], [12 * TILE + 37], [W, 5 * W + 5], [9 * W, 2 * W + 3, 4 * W]):
        for fallback in (0, 1, 2, 0b101):
            for base in (TILE, W, 2 * W, 48):
                for orders in ([[0]], [list(range(len(sizes)))] * 2, [list(range(len(sizes))), list(reversed(range(len(sizes))))]):
                    for min_run, t4 in ((1, 0), (W + 1, 1), (1, 2 * W)):
                        for block in (TILE, W):
                            wide += plan(driver, sizes, W, orders, block=block, fallback=fallback, level_base=base, growth=growth,
                                         min_run=min_run, t4=t4, small_run=1)[1]
    assert wide > 100
