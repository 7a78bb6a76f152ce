"""CPU: the planner's 5-plane flag (quick-adc_amd/host/level_plan.hpp, driver tests/cpp/level_plan_split5_host.cpp).

LevelLaunch::split5 = split and split5_min_run != 0 and every run of the launch has at least split5_min_run codes.  split6 keeps its
meaning beside it (the launcher prefers 5 planes over 6 over 7), and LevelOptions without its last member leaves the form off."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "level_plan_split5_host")
LAUNCH = ("first", "nitems", "small", "shared", "split", "split6", "split5", "minn", "maxn")
UNSET = -1


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "level_plan_split5_host.cpp"), EXE, link=False)
    return EXE


def plan(exe, tmp_path, sizes, assign, split5_min_run, split6_min_run=100000, split_min_run=40000, small_run=1 << 14, share_variant=0):
    assign = np.ascontiguousarray(assign, np.int32)
    nq, ma = assign.shape
    fin, fout = str(tmp_path / "plan5.in"), str(tmp_path / "plan5.out")
    with open(fin, "wb") as f:
        np.array([small_run, share_variant, split_min_run, split6_min_run, split5_min_run, nq, ma, len(sizes)], np.int64).tofile(f)
        np.array(sizes, np.int64).tofile(f)
        assign.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", (out.stdout, out.stderr)
    w = [int(x) for x in np.fromfile(fout, np.uint64)]
    assert len(w) == 1 + w[0] * len(LAUNCH)
    return [dict(zip(LAUNCH, w[1 + i * len(LAUNCH):1 + (i + 1) * len(LAUNCH)])) for i in range(w[0])]


def check(launches, split5_min_run, split6_min_run):
    t5 = 0 if split5_min_run == UNSET else split5_min_run
    for ll in launches:
        assert ll["split5"] == (ll["split"] and t5 != 0 and ll["minn"] >= t5), ll
        assert ll["split6"] == (ll["split"] and split6_min_run != 0 and ll["minn"] >= split6_min_run), ll
        assert not ll["split5"] or ll["split"]


# one partition of 600000 codes at scan position 0: runs of 16384 (level 3, row-major), 98304, 393216 and 75712 codes on tiles
SIZES = [600000, 1000, 196608]


@pytest.mark.parametrize("t5", [UNSET, 0, 1, 75712, 75713, 98304, 98305, 393216, 393217, 1 << 40])
def test_split5_follows_its_threshold(driver, tmp_path, t5):
    ls = plan(driver, tmp_path, SIZES, [[0]], t5)
    check(ls, t5, 100000)
    split = [ll for ll in ls if ll["split"]]
    assert sorted(ll["maxn"] for ll in split) == [75712, 98304, 393216]
    want = 0 if t5 in (UNSET, 0) else sum(1 for n in (75712, 98304, 393216) if n >= t5)
    assert sum(ll["split5"] for ll in split) == want
    assert [ll["split6"] for ll in split if ll["maxn"] == 393216] == [1]                 # unchanged beside it
    assert not any(ll["split6"] for ll in split if ll["maxn"] != 393216)


@pytest.mark.parametrize("t6", [0, 1, 100000, 1 << 40])
def test_split6_is_independent_of_split5(driver, tmp_path, t6):
    a = plan(driver, tmp_path, SIZES, [[0]], 1, split6_min_run=t6)
    b = plan(driver, tmp_path, SIZES, [[0]], 0, split6_min_run=t6)
    c = plan(driver, tmp_path, SIZES, [[0]], UNSET, split6_min_run=t6)
    check(a, 1, t6)
    check(b, 0, t6)
    strip = lambda ls: [{k: v for k, v in ll.items() if k != "split5"} for ll in ls]
    assert strip(a) == strip(b) == strip(c)
    assert all(ll["split5"] == ll["split"] for ll in a) and not any(ll["split5"] for ll in b + c)


def test_the_shortest_run_of_a_launch_decides(driver, tmp_path):
    """two queries whose runs of one level differ in length (393216 and 65536 codes, partition 2 behind partition 0's level edge)"""
    ls = plan(driver, tmp_path, SIZES, [[0, 1], [2, 1]], 100000)
    check(ls, 100000, 100000)
    mixed = [ll for ll in ls if ll["split"] and ll["nitems"] == 2 and ll["minn"] != ll["maxn"]]
    assert mixed and all(ll["split5"] == (ll["minn"] >= 100000) for ll in mixed)
    ls = plan(driver, tmp_path, SIZES, [[0, 1], [0, 1]], 1, share_variant=0x41)          # shared launches are never split
    check(ls, 1, 100000)
    assert not any(ll["split"] or ll["split5"] for ll in ls if ll["shared"]) and any(ll["shared"] for ll in ls)
