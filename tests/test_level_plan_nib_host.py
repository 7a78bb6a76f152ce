"""CPU: the planner's nibble-form field (quick-adc_amd/host/level_plan.hpp, driver tests/cpp/level_plan_nib_host.cpp).

LevelLaunch::nib = 8 where the launch is split, every run has a pointer into its partition's nibble-plane copy and at least
nib8_min_run codes; else nib_ns (9 or 10) where every run has at least nib_min_run codes; else 0.  A threshold of 0 means never,
LevelOptions without the three members leaves the form off, split5 keeps its meaning beside it (the launcher prefers the nibble
form), a run's pointer is the tile of its first code, and a shared launch never takes the form."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "level_plan_nib_host")
LAUNCH = ("first", "nitems", "small", "shared", "split", "split5", "nib", "minn", "maxn", "with_nib", "on_tile")
UNSET = -1


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "level_plan_nib_host.cpp"), EXE, link=False)
    return EXE


def plan(exe, tmp_path, sizes, assign, nib, nib8, ns=9, has_nib=None, split5_min_run=100000, split_min_run=40000, small_run=1 << 14,
         share_variant=0):
    assign = np.ascontiguousarray(assign, np.int32)
    nq, ma = assign.shape
    fin, fout = str(tmp_path / "plann.in"), str(tmp_path / "plann.out")
    with open(fin, "wb") as f:
        np.array([small_run, share_variant, split_min_run, split5_min_run, nib, nib8, ns, nq, ma, len(sizes)], np.int64).tofile(f)
        np.array(sizes, np.int64).tofile(f)
        np.array([1] * len(sizes) if has_nib is None else has_nib, np.int64).tofile(f)
        assign.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", (out.stdout, out.stderr)
    w = [int(x) for x in np.fromfile(fout, np.uint64)]
    assert len(w) == 1 + w[0] * len(LAUNCH)
    return [dict(zip(LAUNCH, w[1 + i * len(LAUNCH):1 + (i + 1) * len(LAUNCH)])) for i in range(w[0])]


def expected(ll, nib, nib8, ns):
    if not ll["split"] or ll["with_nib"] != ll["nitems"]:
        return 0
    if nib8 and ll["minn"] >= nib8:
        return 8
    return ns if nib and ll["minn"] >= nib else 0


def check(launches, nib, nib8, ns, t5=100000):
    for ll in launches:
        assert ll["nib"] == expected(ll, nib, nib8, ns), ll
        assert ll["on_tile"] == ll["with_nib"], ll                       # every pointer is the run's first tile in the copy its launch reads
        assert ll["split5"] == (ll["split"] and t5 != 0 and ll["minn"] >= t5), ll    # unchanged beside it
        assert not ll["nib"] or (ll["split"] and not ll["shared"] and not ll["small"]), ll


# one partition of 600000 codes at scan position 0: runs of 16384 (level 3, row-major), 98304, 393216 and 75712 codes on tiles
SIZES = [600000, 1000, 196608]
RUNS = (75712, 98304, 393216)


@pytest.mark.parametrize("ns", [9, 10])
@pytest.mark.parametrize("t", [0, 1, 75712, 75713, 98304, 98305, 393216, 393217, 1 << 40])
def test_nib_follows_its_threshold(driver, tmp_path, t, ns):
    ls = plan(driver, tmp_path, SIZES, [[0]], t, 0, ns)
    check(ls, t, 0, ns)
    split = [ll for ll in ls if ll["split"]]
    assert sorted(ll["maxn"] for ll in split) == list(RUNS)
    assert sorted(ll["maxn"] for ll in split if ll["nib"] == ns) == [n for n in RUNS if t and n >= t]
    assert all(ll["nib"] in (0, ns) for ll in ls)


@pytest.mark.parametrize("t8", [0, 1, 98304, 98305, 393216, 393217])
@pytest.mark.parametrize("t", [0, 1, 98304, 1 << 40])
def test_eight_planes_above_their_own_threshold(driver, tmp_path, t, t8):
    ls = plan(driver, tmp_path, SIZES, [[0]], t, t8, 10)
    check(ls, t, t8, 10)
    split = [ll for ll in ls if ll["split"]]
    assert sorted(ll["maxn"] for ll in split if ll["nib"] == 8) == [n for n in RUNS if t8 and n >= t8]
    assert sorted(ll["maxn"] for ll in split if ll["nib"] == 10) == [n for n in RUNS if t and n >= t and not (t8 and n >= t8)]


def test_zero_and_unset_mean_never(driver, tmp_path):
    a = plan(driver, tmp_path, SIZES, [[0]], 0, 0)
    b = plan(driver, tmp_path, SIZES, [[0]], UNSET, UNSET, UNSET)
    assert a == b and not any(ll["nib"] for ll in a) and any(ll["split5"] for ll in a)
    assert all(ll["with_nib"] == ll["nitems"] for ll in a if ll["split"])           # the copies are there; the thresholds say no


def test_nib_beside_split5(driver, tmp_path):
    """Both qualify on the 393216-code run: both fields are set (the launcher takes the nibble form), and split5 does not change."""
    on = plan(driver, tmp_path, SIZES, [[0]], 1, 0)
    off = plan(driver, tmp_path, SIZES, [[0]], 0, 0)
    check(on, 1, 0, 9)
    both = [ll for ll in on if ll["nib"] and ll["split5"]]
    assert [ll["maxn"] for ll in both] == [393216]
    strip = lambda ls: [{k: v for k, v in ll.items() if k != "nib"} for ll in ls]
    assert strip(on) == strip(off)


def test_a_partition_without_the_copy_keeps_the_other_forms(driver, tmp_path):
    ls = plan(driver, tmp_path, SIZES, [[0]], 1, 0, has_nib=[0, 1, 1])
    check(ls, 1, 0, 9)
    assert not any(ll["nib"] or ll["with_nib"] for ll in ls) and any(ll["split5"] for ll in ls)
    # two queries in one launch, one run with the copy and one without: the launch does not take the form
    ls = plan(driver, tmp_path, SIZES, [[0, 1], [2, 1]], 1, 0, has_nib=[1, 1, 0])
    check(ls, 1, 0, 9)
    mixed = [ll for ll in ls if ll["split"] and 0 < ll["with_nib"] < ll["nitems"]]
    assert mixed and not any(ll["nib"] for ll in mixed)


def test_the_shortest_run_decides_and_shared_launches_never(driver, tmp_path):
    ls = plan(driver, tmp_path, SIZES, [[0, 1], [2, 1]], 100000, 0)
    check(ls, 100000, 0, 9)
    mixed = [ll for ll in ls if ll["split"] and ll["nitems"] == 2 and ll["minn"] != ll["maxn"]]
    assert mixed and all(bool(ll["nib"]) == (ll["minn"] >= 100000) for ll in mixed)
    ls = plan(driver, tmp_path, SIZES, [[0, 1], [0, 1]], 1, 1, share_variant=0x41)
    check(ls, 1, 1, 9)
    assert any(ll["shared"] for ll in ls) and not any(ll["nib"] or ll["split"] for ll in ls if ll["shared"])


def test_runs_off_the_tiles_have_no_pointer(driver, tmp_path):
    """A second partition behind 1000 codes: its runs start where the level edges fall, not on tiles of its copy."""
    ls = plan(driver, tmp_path, [1000, 600000], [[0, 1]], 1, 1)
    check(ls, 1, 1, 9)
    assert all(ll["with_nib"] == 0 and ll["nib"] == 0 for ll in ls if not ll["split"])
    assert all(ll["with_nib"] == ll["nitems"] for ll in ls if ll["split"])
