"""CPU: the planner's bucket-form fields (quick-adc_amd/host/level_plan.hpp, driver tests/cpp/level_plan_bkt_host.cpp).

The driver plans every case twice, with and without bucket copies, and checks launch by launch: LevelLaunch::bkt is set exactly
when every run of a split launch starts on a block of its partition's copy, ends on one or at the partition's end and has
bkt_min_run codes; such runs carry the slots between their blocks' offsets and the tiles of the copy and of its side array, the
workgroups derive from the slots, the code counts stay the originals; every other launch and run equals today's field for field.
Here: the sweep of partition sizes, block sizes and level options, and what the counts of a few known cases must be."""
import os
import subprocess

import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "level_plan_bkt_host")
TILE = 16384


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "level_plan_bkt_host.cpp"), EXE, link=False)
    return EXE


def plan(exe, sizes, block, orders, level_base=16384, growth=4, head_level=0, bkt_min_run=1, t6=0, t5=0, t4=0, small_run=1,
         share_variant=0):
    args = [",".join(str(s) for s in sizes), block, level_base, growth, head_level, bkt_min_run, t6, t5, t4, len(orders),
            ";".join(" ".join(str(p) for p in o) for o in orders), small_run, share_variant]
    out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    words = out.stdout.decode().split()
    assert out.returncode == 0 and words and words[0] == "ok", (args, out.stdout, out.stderr)
    return tuple(int(w) for w in words[1:])                   # launches, bucket launches, bucket runs


def test_known_cases(driver):
    n = 3 * TILE + 37
    # levels [0, 16 Ki), [16 Ki, 64 Ki): both on blocks of one tile; with blocks of two tiles neither is
    assert plan(driver, [n], TILE, [[0]]) == (2, 2, 2)
    assert plan(driver, [n], 2 * TILE, [[0]]) == (2, 0, 0)
    # ... [64 Ki, n) starts on a block of two tiles and ends the partition
    assert plan(driver, [65536 + 6 * TILE + 37], 2 * TILE, [[0], [0]]) == (3, 1, 2)
    # bkt_min_run: the first level's runs are too short, the launch keeps today's plan
    assert plan(driver, [n], TILE, [[0]], bkt_min_run=TILE + 1) == (2, 1, 1)
    assert plan(driver, [n], TILE, [[0]], bkt_min_run=0) == (2, 0, 0)
    # two partitions, the second probed behind 32 Ki codes of the first: its cut at 64 Ki falls on its block 2
    assert plan(driver, [2 * TILE, 2 * TILE + 37], TILE, [[0, 1]])[1:] == (3, 4)
    # one run of a launch without a copy (partition 2 has none) keeps the whole launch on today's plan
    assert plan(driver, [4 * TILE, 4 * TILE, 4 * TILE], TILE, [[0], [2]])[1] == 0
    # a shared launch (every query over the same codes, sibling-major) never takes the form
    assert plan(driver, [n], TILE, [[0], [0]], share_variant=0x41)[1] == 0
    # the headline: 10^9 codes, blocks of 2^25, level base 512 x 4^k behind a head of 5 levels: the levels from 2^25, 2^27 and 2^29
    assert plan(driver, [10 ** 9], 1 << 25, [[0]] * 2, level_base=512, head_level=5, bkt_min_run=1 << 25, t6=1 << 25, t5=1 << 27,
                small_run=1 << 17) == (7, 3, 6)


@pytest.mark.parametrize("block", [TILE, 2 * TILE, 1 << 17])
@pytest.mark.parametrize("growth", [2, 4])
def test_sweep(driver, block, growth):
    total = 0
    for sizes in ([3 * TILE + 37], [1 << 18], [(1 << 18) + 5], [(1 << 20) - TILE], [2 * TILE, 2 * TILE + 37, 1 << 17],
                  [1 << 17, 3 * (1 << 17) + 1, 1 << 16, 5 * TILE]):
        orders = [list(range(len(sizes))), list(reversed(range(len(sizes))))]
        for level_base in (TILE, 4 * TILE, 512):
            for head_level in (0, 3):
                for bkt_min_run, t6, t5, t4 in ((1, 0, 0, 0), (1, 1, 1 << 16, 1 << 18), (1 << 16, 1 << 17, 0, 1 << 19)):
                    total += plan(driver, sizes, block, orders, level_base, growth, head_level, bkt_min_run, t6, t5, t4,
                                  small_run=1 if level_base >= TILE else 1 << 14)[1]
    assert total > 0
