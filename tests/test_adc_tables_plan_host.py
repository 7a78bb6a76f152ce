"""CPU: the launch geometry of the float-ADC feeders (quick-adc_amd/host/adc_tables_plan.hpp, driver
tests/cpp/adc_tables_plan_host.cpp).  launch_adc_tables and launch_adc_encode launch what the header plans, and the kernels index
LDS and their output by it, so the header as the library compiles it is held here to
  * a restatement of the launcher's arithmetic, for every input of a sweep over the shapes the entry points admit;
  * the invariants the kernels rely on: the workgroups' (probe range, sub-quantizer range, centroid range) tile
    [0, ma) x [0, nsq) x [0, centroids) exactly once, the dynamic LDS is at most 48 KiB, probes >= 1, grid.y and grid.z are at
    most 65535 and mper * msplit == nsq; the encoder's chunks tile [0, n) exactly once;
  * the geometry every case of tests/adc_tables_cases.py is named for (what tests/test_gpu_adc_tables_geometry.py runs)."""
import os
import subprocess

import numpy as np
import pytest

import adc_tables_cases as cases
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_tables_plan_host")
LDS_LIMIT = 48 * 1024
MAX_DIM = 4096

NQ = (1, 2, 3, 5, 31, 32, 33, 127, 128, 129, 256, 257, 511, 512, 513, 2047, 2048, 4096)
MA = (1, 2, 15, 16, 17, 24, 32, 33, 64, 256, 300)
SHAPES = [(nsq, 256) for nsq in (4, 8, 16)] + [(nsq, 65536) for nsq in (2, 4, 8)]
DS = (1, 2, 5, 8, 12, 16, 30, 32, 64, 120, 256)


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "adc_tables_plan_host.cpp"), EXE, link=False)
    return EXE


def run(exe, tmp_path, rows):
    """rows of (kind, a0 .. a5) -> int64 [n][12]"""
    fin, fout = str(tmp_path / "plans.in"), str(tmp_path / "plans.out")
    np.asarray(rows, np.int64).reshape(-1, 7).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0, out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % len(rows)
    return np.fromfile(fout, np.int64).reshape(len(rows), 12)


def tables_plans(exe, tmp_path, shapes):
    """shapes of (nq, ma, nsq, centroids, dim, rotated) -> list of plans (None: refused)"""
    got = run(exe, tmp_path, [(0,) + tuple(int(v) for v in s) for s in shapes])
    names = ("probes", "pgroups", "msplit", "mper", "cper", "cslices", "DS")
    return [None if not g[0] else dict(zip(names, (int(v) for v in g[1:8])), grid=tuple(int(v) for v in g[8:11]), lds_bytes=int(g[11])) for g in got]


def ceil_div(a, b):
    return -(-a // b)


def restated(nq, ma, nsq, centroids, dim, rotated):
    """launch_adc_tables as it stood before the header, and the probes it had before the halving loop"""
    ds = dim // nsq
    groups = ceil_div(ma, 16)
    msplit = 1
    if nq * groups < 512:
        msplit = nsq
    if nq * groups * msplit < 512:
        groups = min(ma, max(groups, ceil_div(512, nq * msplit)))
    probes = ceil_div(ma, groups)
    mper = nsq // msplit

    def lds_floats(p):
        return p * mper * ds + p * mper + (p * dim if rotated else 0)

    unhalved = probes
    while probes > 1 and 4 * lds_floats(probes) > LDS_LIMIT:
        probes = (probes + 1) // 2
    pgroups = ceil_div(ma, probes)
    cper = centroids // 256
    while cper > 1 and nq * pgroups * msplit * (centroids // (256 * cper)) < 2048:
        cper //= 2
    cslices = centroids // (256 * cper)
    plan = dict(probes=probes, pgroups=pgroups, msplit=msplit, mper=mper, cper=cper, cslices=cslices, DS=ds if ds in (8, 16, 32) else 0,
                grid=(nq, pgroups, msplit * cslices), lds_bytes=4 * lds_floats(probes))
    return plan, unhalved


def probe_cover(ma, probes, pgroups):
    """how often the workgroups of grid.y cover every probe, by the kernel's a0 = blockIdx.y * probes, na = min(probes, ma - a0)"""
    count = np.zeros(ma, np.int64)
    for y in range(pgroups):
        a0 = y * probes
        na = min(probes, ma - a0)
        assert na >= 1, "probe group %d of %d is empty (ma %d, probes %d)" % (y, pgroups, ma, probes)
        count[a0:a0 + na] += 1
    return count


def centroid_cover(nsq, centroids, mper, cper, grid_z):
    """how often the workgroups of grid.z cover every (sub-quantizer, centroid), by the kernel's cslices = centroids / (256 * cper),
    m0 = (blockIdx.z / cslices) * mper, c0 = (blockIdx.z % cslices) * cper * 256 and c = c0 + cb * 256 + tid"""
    count = np.zeros((nsq, centroids), np.int64)
    cslices = centroids // (256 * cper)
    for z in range(grid_z):
        m0, c0 = (z // cslices) * mper, (z % cslices) * cper * 256
        assert m0 + mper <= nsq and c0 + cper * 256 <= centroids, "workgroup z %d reaches past the tables" % z
        count[m0:m0 + mper, c0:c0 + cper * 256] += 1
    return count


def test_plan_equals_the_restatement_and_tiles_the_tables(driver, tmp_path):
    shapes = []
    for nsq, centroids in SHAPES:
        for ds in sorted(set(DS + (MAX_DIM // nsq,))):               # (the largest is 256, already listed, for 16 x 8)
            if ds * nsq <= MAX_DIM:
                shapes += [(nq, ma, nsq, centroids, ds * nsq, rot) for nq in NQ for ma in MA for rot in (0, 1)]
    assert len(set(shapes)) == len(shapes) == 18 * 11 * (6 * 12 - 1) * 2
    plans = tables_plans(driver, tmp_path, shapes)
    probe_seen, centroid_seen = set(), set()
    for shape, p in zip(shapes, plans):
        nq, ma, nsq, centroids, dim, rot = shape
        assert p is not None, "an admitted shape is refused: %s" % (shape,)
        want, _ = restated(*shape)
        assert p == want, "%s: planned %s, restated %s" % (shape, p, want)
        assert p["probes"] >= 1 and p["lds_bytes"] <= LDS_LIMIT, (shape, p)
        assert p["mper"] * p["msplit"] == nsq and p["cper"] * p["cslices"] * 256 == centroids, (shape, p)
        assert p["grid"][0] == nq and 1 <= p["grid"][1] <= 65535 and 1 <= p["grid"][2] <= 65535, (shape, p)
        assert p["grid"][1] == p["pgroups"] and p["grid"][2] == p["msplit"] * p["cslices"], (shape, p)
        key = (ma, p["probes"], p["pgroups"])                      # the cover depends on these alone: each is walked once
        if key not in probe_seen:
            probe_seen.add(key)
            assert (probe_cover(*key) == 1).all(), (shape, p)
        key = (nsq, centroids, p["mper"], p["cper"], p["grid"][2])
        if key not in centroid_seen:
            centroid_seen.add(key)
            assert (centroid_cover(*key) == 1).all(), (shape, p)
    # the sweep reaches what it is there for
    assert any(p["probes"] < restated(*s)[1] for s, p in zip(shapes, plans)), "the halving loop is never entered"
    assert any(p["msplit"] == 1 and p["mper"] > 1 and p["probes"] > 1 for p in plans)
    assert any(p["cper"] > 1 and p["mper"] > 1 for p in plans)
    assert {p["DS"] for p in plans} == {0, 8, 16, 32}


def test_plan_refuses_what_the_kernel_does_not_take(driver, tmp_path):
    bad = [(0, 1, 4, 256, 128, 0), (1, 0, 4, 256, 128, 0), (1, 1, 0, 256, 128, 0), (1, 1, 4, 256, 0, 0), (1, 1, 4, 256, 130, 0),
           (1, 1, 4, 256, 4100, 0), (1, 1, 4, 16, 128, 0), (1, 1, 4, 512, 128, 0), (1, 1, 2, 65536, MAX_DIM + 2, 1)]
    assert tables_plans(driver, tmp_path, bad) == [None] * len(bad)
    got = run(driver, tmp_path, [(1, 0, 4, 8, 0, 0, 0), (1, 5, 0, 8, 0, 0, 0), (1, 5, 4, 0, 0, 0, 0), (1, 5, 4, 10, 0, 0, 0), (1, 5, 4, 4100, 0, 0, 0)])
    assert not got[:, 0].any()


@pytest.mark.parametrize("case", cases.TABLES, ids=[c["name"] for c in cases.TABLES])
def test_every_gpu_case_reaches_the_geometry_it_is_named_for(driver, tmp_path, case):
    shape = (case["nq"], case["ma"], case["nsq"], case["centroids"], case["dim"], int(case["opq"]))
    (p,) = tables_plans(driver, tmp_path, [shape])
    want, unhalved = restated(*shape)
    assert p == want == case["plan"]
    assert unhalved == case["unhalved"]
    assert case["ma"] - (p["pgroups"] - 1) * p["probes"] == case["last"]
    assert cases.table_bytes(case) == case["nq"] * case["ma"] * case["nsq"] * case["centroids"] * 4


def test_the_gpu_cases_cover_the_geometries_of_the_issue():
    """each property below is held by at least one case the GPU test runs"""
    t8, t16 = cases.TABLES8, cases.TABLES16
    halved = [c for c in cases.TABLES if c["plan"]["probes"] < c["unhalved"]]
    assert any(c["plan"]["msplit"] == 1 and c["opq"] for c in halved) and any(c["plan"]["msplit"] == 1 and not c["opq"] for c in halved)
    assert any(c["plan"]["msplit"] > 1 for c in halved)
    assert any(c["unhalved"] // c["plan"]["probes"] == 8 for c in halved)                          # three halvings
    assert any(c["plan"]["msplit"] == 1 and c["plan"]["probes"] > 1 and c["last"] < c["plan"]["probes"] for c in t8)
    assert sum(c["dim"] == MAX_DIM for c in t8) == 2
    assert any(c["plan"]["mper"] > 1 and c["plan"]["cper"] > 1 and c["plan"]["probes"] == 1 for c in t16)
    assert any(c["plan"]["mper"] > 1 and c["plan"]["cper"] > 1 and c["plan"]["probes"] == 2 for c in t16)
    assert {(c["nsq"], c["plan"]["DS"]) for c in t16} >= {(2, 8), (4, 32), (2, 0), (8, 16)}
    assert all(cases.table_bytes(c) <= 1 << 30 for c in cases.TABLES)                              # one pass of the default table budget


# ---- the 8-bit encoder ------------------------------------------------------------------------------------------------------

def encode_restated(n, nsq, dim):
    vper = max(1, min(32, 8192 // dim))
    ds = dim // nsq
    return dict(vper=vper, DS=ds if ds in (8, 16, 32) else 0, grid=min(ceil_div(n, vper), 8192), lds_bytes=vper * (4 * 8 + 4 * 4 + dim * 4 + nsq * 4 + nsq))


def encode_plans(exe, tmp_path, shapes):
    got = run(exe, tmp_path, [(1, n, nsq, dim, 0, 0, 0) for n, nsq, dim in shapes])
    return [None if not g[0] else dict(vper=int(g[1]), DS=int(g[2]), grid=int(g[3]), lds_bytes=int(g[4])) for g in got]


def chunks_of(n, vper, grid, wg):
    """the (v0, nv) chunks of one workgroup: the kernel's loop for (v0 = blockIdx.x * vper; v0 < n; v0 += gridDim.x * vper)"""
    return [(v0, min(vper, n - v0)) for v0 in range(wg * vper, n, grid * vper)]


def test_encode_plan_equals_the_restatement_and_tiles_the_vectors(driver, tmp_path):
    sizes = (1, 2, 31, 32, 33, 8192, 8193, 262143, 262144, 262145, 8192 * 32 + 33, 8192 * 4 + 5, 1000003, (1 << 32) + 7)
    shapes = [(n, nsq, ds * nsq) for nsq in (4, 8, 16) for ds in sorted(set(DS + (MAX_DIM // nsq,))) if ds * nsq <= MAX_DIM for n in sizes]
    for shape, p in zip(shapes, encode_plans(driver, tmp_path, shapes)):
        n, nsq, dim = shape
        assert p == encode_restated(*shape), shape
        assert p["vper"] >= 1 and 1 <= p["grid"] <= 8192 and p["lds_bytes"] <= LDS_LIMIT, (shape, p)
        # chunk j belongs to workgroup j % grid: every chunk is taken once, a workgroup's chunks are grid * vper apart
        nchunks = ceil_div(n, p["vper"])
        assert p["grid"] == min(nchunks, 8192)
        if n <= 1000003:
            trips = ceil_div(nchunks, p["grid"])
            v0 = (np.arange(p["grid"], dtype=np.int64)[:, None] + np.arange(trips, dtype=np.int64)[None, :] * p["grid"]) * p["vper"]
            taken = np.sort(v0[v0 < n])                            # what the workgroups' loops visit
            assert np.array_equal(taken, np.arange(0, n, p["vper"])), shape
            assert trips == len(chunks_of(n, p["vper"], p["grid"], 0))


@pytest.mark.parametrize("case", cases.ENCODE, ids=[c["name"] for c in cases.ENCODE])
def test_every_encoder_case_takes_a_second_trip(driver, tmp_path, case):
    (p,) = encode_plans(driver, tmp_path, [(case["n"], case["nsq"], case["dim"])])
    assert p == encode_restated(case["n"], case["nsq"], case["dim"]) == case["plan"]
    first, second = (chunks_of(case["n"], p["vper"], p["grid"], wg) for wg in (0, 1))
    assert (len(first), len(second)) == case["trips"]
    assert first[1][1] == p["vper"] and second[1][1] == case["last"]               # a full second chunk and a one-vector one
    assert chunks_of(case["n"], p["vper"], p["grid"], 2)[1:] == []
    assert case["n"] > cases.ENCODE_ROWS and case["n"] % cases.ENCODE_ROWS != 0     # the tiling ends inside the distinct rows
