"""CPU: the level planner of the float-ADC engine (quick-adc_amd/host/adc_plan.hpp, driver tests/cpp/adc_plan_host.cpp).

The exactness argument of DESIGN.md section 11 rests on the plan alone: every code of a query's scan order is scanned exactly
once, in the level its scan index falls in, by a run that stays inside one probed partition.  Each case below is planned by
the header as the library compiles it and the whole plan is checked here, query by query."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_plan_host")
REFUSAL = "query %d probes %d codes: at most 2^32 - 1 per query"


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "adc_plan_host.cpp"), EXE, link=False)
    return EXE


def plan(exe, tmp_path, sizes, assign, R):
    """the plan of one batch as a dict, or the refusal's message"""
    assign = np.ascontiguousarray(assign, np.int32)
    nq, ma = assign.shape
    fin, fout = str(tmp_path / "plan.in"), str(tmp_path / "plan.out")
    with open(fin, "wb") as f:
        np.array([R, nq, ma, len(sizes)], np.int32).tofile(f)
        np.asarray(sizes, np.uint32).tofile(f)
        assign.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    text = out.stdout.decode().strip()
    assert out.returncode == 0, out.stderr.decode()
    if text.startswith("refused: "):
        return text[len("refused: "):]
    assert text == "ok"
    with open(fout, "rb") as f:
        level0, growth, wg_target, run_min, run_max, levels, n_items = (int(x) for x in np.fromfile(f, np.uint32, 7))
        p = dict(level0=level0, growth=growth, wg_target=wg_target, run_min=run_min, run_max=run_max, levels=levels,
                 total=np.fromfile(f, np.uint64, nq), edge=np.fromfile(f, np.uint64, levels + 1),
                 level_first=np.fromfile(f, np.uint32, levels + 1), cap=np.fromfile(f, np.uint32, nq),
                 items=np.fromfile(f, np.uint32, 8 * n_items).reshape(n_items, 8).astype(np.int64))
        assert f.read() == b""
    return p


def check(p, sizes, assign, R):
    """the invariants the exactness argument uses, for every query; returns the longest run of every level"""
    sizes, assign = np.asarray(sizes, np.int64), np.asarray(assign, np.int64)
    nq, ma = assign.shape
    assert (p["level0"], p["growth"], p["run_min"], p["run_max"]) == (512, 16, 2048, 65536)
    total = sizes[assign].sum(axis=1)
    assert np.array_equal(p["total"].astype(np.int64), total)
    edge = [0, max(R, 512)]
    while edge[-1] < total.max():
        edge.append(edge[-1] * 16)
    assert p["edge"].astype(np.int64).tolist() == edge and p["levels"] == len(edge) - 1
    items, first = p["items"], p["level_first"].astype(np.int64)
    assert first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] == len(items)
    level = np.searchsorted(first, np.arange(len(items)), side="right") - 1     # (a level without items repeats its first)
    query, slot, start, count, sbase = (items[:, i] for i in range(5))
    assert (items[:, 5:] == 0).all()
    assert ((query >= 0) & (query < nq) & (slot >= 0) & (slot < ma)).all()
    assert ((count >= 1) & (count <= p["run_max"])).all()
    lo, hi = np.asarray(edge)[level], np.minimum(total[query], np.asarray(edge)[level + 1])
    assert (lo <= sbase).all() and (sbase + count <= hi).all()
    slot_base = np.concatenate([np.zeros((nq, 1), np.int64), np.cumsum(sizes[assign], axis=1)[:, :-1]], axis=1)
    assert (start + count <= sizes[assign[query, slot]]).all()
    assert (sbase - start == slot_base[query, slot]).all()
    for q in range(nq):                                                          # array order = level by level, then scan order
        mine = np.flatnonzero(query == q)
        ends = sbase[mine] + count[mine]
        assert np.array_equal(sbase[mine], np.concatenate([[0], ends[:-1]])[:len(mine)])
        assert (ends[-1] if len(mine) else 0) == total[q]
    want_cap = np.maximum(1, np.minimum(total, max(R, 512) + 32 * R * (p["levels"] - 1) + 4096))
    assert np.array_equal(p["cap"].astype(np.int64), want_cap)
    return [int(count[level == l].max()) if (level == l).any() else 0 for l in range(p["levels"])]


# (name, partition sizes, assign [nq][ma], R)
CASES = [(("total_%d" % n), [n], [[0]], 1) for n in (0, 1, 511, 512, 513, 8192, 8193)] + [
    ("R_600_level0_is_R", [599, 1, 2, 9000], [[0, 1, 2, 3]], 600),
    ("R_600_total_600", [600], [[0]], 600),
    ("partition_ends_on_edges", [512, 7680, 100], [[0, 1, 2]], 1),              # 512 and 8192 are level edges
    ("partition_straddles_edges", [500, 30, 7700, 9], [[0, 1, 2, 3]], 1),
    ("empty_partitions_first_inside_last", [0, 700, 0, 0, 9000, 0], [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]], 1),
    ("only_empty_partitions", [0, 0], [[0, 1, 0, 1]], 1),
    ("same_partition_twice", [5000, 3], [[0, 0, 1, 0]], 1),
    ("nq3_unequal_ma4", [10, 513, 8193, 0, 140000], [[0, 1, 2, 3], [4, 0, 0, 1], [3, 3, 3, 0]], 7),
    ("nq3_ma1", [1, 8192, 600], [[0], [1], [2]], 100),
    ("run_above_kRunMin", [7000000, 11], [[1, 0]], 100),                        # last level spans 4.9 M codes: runs of 3072
    ("run_at_kRunMax", [1 << 31, 12345, 1 << 30], [[1, 0, 2], [2, 1, 1]], 100),
    ("total_2_32_minus_1", [0xffffffff, 0], [[1, 0]], 1),
]


@pytest.mark.parametrize("name,sizes,assign,R", CASES, ids=[c[0] for c in CASES])
def test_plan_tiles_every_scan_order_exactly_once(driver, tmp_path, name, sizes, assign, R):
    p = plan(driver, tmp_path, sizes, assign, R)
    assert isinstance(p, dict), p
    longest = check(p, sizes, assign, R)
    if name == "run_above_kRunMin":
        assert p["run_min"] < longest[-1] < p["run_max"]
    if name == "run_at_kRunMax":
        assert longest[-1] == p["run_max"]
    if name.startswith("total_") and sizes[0] <= 8193:                           # the edges 512 and 8192 from both sides
        assert p["levels"] == (1 if sizes[0] <= 512 else 2 if sizes[0] <= 8192 else 3)


@pytest.mark.parametrize("sizes,assign,q,total", [
    ([0xffffffff, 1], [[0, 1]], 0, 1 << 32),
    ([5, 1 << 31], [[0, 0], [1, 1], [1, 1]], 1, 1 << 32),                        # the first query over the limit is named
    ([0xffffffff], [[0, 0, 0, 0]], 0, 4 * 0xffffffff),
])
def test_plan_refuses_a_query_over_2_32_minus_1_codes(driver, tmp_path, sizes, assign, q, total):
    assert plan(driver, tmp_path, sizes, assign, 10) == REFUSAL % (q, total)
