"""CPU: the range planner (host/adc_plan.hpp: plan_range, plan_range_rerun, range_entries; driver tests/cpp/adc_range_plan_host.cpp;
DESIGN.md section 11.13).

The runs cover every query's scan order exactly once, partition by partition in assign[] order; the first regions hold
min(total[q], kRangeFirstCap) entries and never more than total[q]; after an attempt the regions that overflowed hold exactly the
counted rows, so a pass scans at most twice; a query probing more than 2^32 - 1 codes is refused, and so are regions that add up to more
than the entry limit — with made-up counts, since no GPU test reaches QADC_ADC_MAX_ENTRIES."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_range_plan_host")
FIRST_CAP, RUN_MIN, RUN_MAX, WG_TARGET = 4096, 2048, 65536, 2048   # kRangeFirstCap, kRunMin, kRunMax, kWgTarget
MAX_ENTRIES = 1 << 34                                               # QADC_ADC_MAX_ENTRIES


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def test_the_constants_are_the_headers():
    plan = open(os.path.join(ROOT, "quick-adc_amd", "host", "adc_plan.hpp")).read()
    assert "kRangeFirstCap = %d;" % FIRST_CAP in plan and "kRunMin = %d, kRunMax = %d;" % (RUN_MIN, RUN_MAX) in plan
    assert "#define QADC_ADC_MAX_ENTRIES (1ull << 34)" in open(os.path.join(ROOT, "include", "qadc.h")).read()


def plan(exe, tmp_path, sizes, assign, counts=None, max_entries=MAX_ENTRIES):
    assign = np.asarray(assign, np.int32)
    nq, ma = assign.shape
    fin = str(tmp_path / "plan.in")
    with open(fin, "wb") as f:
        np.array([len(sizes), nq, ma, counts is not None], np.int32).tofile(f)
        np.asarray(sizes, np.uint32).tofile(f)
        assign.tofile(f)
        np.array([max_entries], np.uint64).tofile(f)
        if counts is not None:
            np.asarray(counts, np.uint32).tofile(f)
    out = subprocess.run([exe, fin], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()
    res = dict(items=[])
    for ln in out.stdout.decode().splitlines():
        name, _, rest = ln.partition(" ")
        if name == "item":
            res["items"].append(tuple(int(x) for x in rest.split()))
        elif name in ("total", "cap", "recap"):
            res[name] = [int(x) for x in rest.split()]
        elif name in ("first", "second"):
            n, _, why = rest.partition(" ")
            res[name] = (int(n), "" if why == "-" else why)
        else:
            res[name] = rest
    return res


def check_cover(sizes, assign, res):
    """every query's scan order [0, total) is covered once, in runs that stay inside one probed partition"""
    sizes = np.asarray(sizes, np.int64)
    nq, ma = assign.shape
    total = sizes[assign].sum(axis=1)
    assert res["total"] == list(total)
    span = int(total.sum())
    per_wg = -(-span // WG_TARGET)
    run = min(RUN_MAX, max(RUN_MIN, -(-per_wg // 1024) * 1024))            # the cut of a level (plan_levels)
    at = {q: 0 for q in range(nq)}
    last = (-1, -1)
    for q, slot, start, count, sbase in res["items"]:
        assert (q, slot) >= last, "the items come query by query in scan order"
        last = (q, slot)
        pbase = int(sizes[assign[q, :slot]].sum())
        assert sbase == at[q] == pbase + start, "query %d: run at scan index %d, expected %d" % (q, sbase, at[q])
        assert 1 <= count <= run and start + count <= sizes[assign[q, slot]]
        assert count == run or start + count == sizes[assign[q, slot]], "only the last run of a partition is short"
        at[q] += count
    assert [at[q] for q in range(nq)] == list(total), "a scan order is not covered to its end"


def test_runs_cover_every_scan_order_once_and_regions_fit(driver, tmp_path):
    rng = np.random.default_rng(1)
    sizes = np.array([0, 1, 1023, 1025, 2049, 70000, 4096, 4097, 131072 + 5, 3], np.uint32)
    for nq, ma in ((1, 1), (3, 4), (7, 10), (40, 6)):
        assign = rng.integers(0, len(sizes), (nq, ma)).astype(np.int32)
        assign[0, 0] = 0                                         # a probed empty partition
        res = plan(driver, tmp_path, sizes, assign)
        check_cover(sizes, assign, res)
        total = np.asarray(sizes, np.int64)[assign].sum(axis=1)
        assert res["cap"] == [min(int(t), FIRST_CAP) for t in total]
        assert all(c <= t for c, t in zip(res["cap"], total))
        assert res["first"] == (sum(res["cap"]), "")
    res = plan(driver, tmp_path, [0, 5], np.array([[0, 0], [0, 1]], np.int32))
    assert res["total"] == [0, 5] and res["cap"] == [0, 5] and res["items"] == [(1, 1, 0, 5, 0)]


def test_long_batches_get_longer_runs_up_to_the_maximum(driver, tmp_path):
    sizes = np.array([3_000_000, 2 ** 31], np.uint32)
    res = plan(driver, tmp_path, sizes, np.array([[0, 0], [0, 0]], np.int32))      # span 12e6 -> runs of 6144
    check_cover(sizes, np.array([[0, 0], [0, 0]]), res)
    assert max(i[3] for i in res["items"]) == 6144
    res = plan(driver, tmp_path, sizes, np.array([[1]], np.int32))                 # span 2^31 -> capped at kRunMax
    check_cover(sizes, np.array([[1]]), res)
    assert max(i[3] for i in res["items"]) == RUN_MAX and len(res["items"]) == 2 ** 31 // RUN_MAX


def test_the_rerun_regions_equal_the_counts(driver, tmp_path):
    sizes = [10000, 200, 0, 5000]
    assign = np.array([[0, 1], [1, 2], [3, 3], [2, 2]], np.int32)               # totals 10200, 200, 10000, 0
    counts = [10200, 200, 4097, 0]                                               # q0 keeps all, q1 fits, q2 one past its region, q3 nothing
    res = plan(driver, tmp_path, sizes, assign, counts)
    assert res["cap"] == [4096, 200, 4096, 0]
    assert res["rerun"] == "1" and res["recap"] == [10200, 200, 4097, 0] and res["second"] == (10200 + 200 + 4097, "")
    again = plan(driver, tmp_path, sizes, assign, [4096, 0, 17, 0])              # nothing overflowed: no re-run, the regions stay
    assert again["rerun"] == "0" and again["recap"] == again["cap"]
    assert all(c <= t for c, t in zip(res["recap"], res["total"]))


def test_more_than_2_to_32_minus_1_codes_per_query_is_refused(driver, tmp_path):
    sizes = np.array([2 ** 32 - 1, 1], np.uint32)
    ok = plan(driver, tmp_path, sizes, np.array([[0]], np.int32), [0])
    assert "refused" not in ok and ok["total"] == [2 ** 32 - 1]
    res = plan(driver, tmp_path, sizes, np.array([[1, 1], [0, 1]], np.int32))
    assert res["refused"].startswith("query 1 probes 4294967296 codes") and "2^32 - 1" in res["refused"] and not res["items"]


def test_regions_beyond_the_entry_limit_are_refused(driver, tmp_path):
    """made-up counts: five queries of 2^32 - 1 probed codes each that keep everything need 5 (2^32 - 1) > 2^34 entries"""
    sizes = np.array([2 ** 32 - 1], np.uint32)
    assign = np.zeros((5, 1), np.int32)
    counts = [2 ** 32 - 1] * 5
    res = plan(driver, tmp_path, sizes, assign[:1], counts[:1])
    assert res["first"] == (FIRST_CAP, "") and res["second"] == (2 ** 32 - 1, "")
    res = plan(driver, tmp_path, np.array([2 ** 31], np.uint32), assign, [2 ** 31] * 5)
    assert res["first"] == (5 * FIRST_CAP, "") and res["rerun"] == "1"
    n, why = res["second"]
    assert n == 5 * 2 ** 31 and why == ""                                       # 2.5 * 2^32 <= 2^34: still fits
    res = plan(driver, tmp_path, np.array([2 ** 32 - 1], np.uint32), assign, counts, MAX_ENTRIES)
    n, why = res["second"]
    assert n == 5 * (2 ** 32 - 1) and "at most %d" % MAX_ENTRIES in why and str(n) in why
    small = plan(driver, tmp_path, [100], np.zeros((3, 1), np.int32), [100, 100, 100], max_entries=250)   # and the first attempt is checked too
    assert small["first"][0] == 300 and "at most 250" in small["first"][1]
