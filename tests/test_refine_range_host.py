"""CPU: the host twin of the exact range search (refine::range and refine::rerank_range of quick-adc_amd/host/refine.hpp, driver
tests/cpp/refine_range_host.cpp) — the written definition of qadc_refine_range and qadc_refine_rerank_range (DESIGN.md section
11.21), to which the GPU is held bit for bit.

The twin is compared, bit for bit, with an independent numpy restatement (tests/refine_range_cases.py: refine_cases.np_distance over
the held rows, the filter in numpy, a float compare with the radius, a sort of the words), and with itself three ways: range equals
rerank_range of every held key that passes the filter; under radius +inf on finite data range equals the twin's knn at R >= rows;
under radius +inf the first R rows of rerank_range equal rerank of the same keys."""
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_range_cases as rr

INF, F32 = rr.INF, np.float32
DIMS = (1, 63, 64, 65, 128, 256, 257, 4096)
RADII = [np.nan, np.inf, 0.0, -0.0, -1.0, rr.FLT_MAX, rr.SUBNORMAL]


@pytest.fixture(scope="module")
def driver():
    return rr.build_driver()


def check(exe, tmp_path, cases, names):
    for name, c, got in zip(names, cases, rr.run_twin(exe, tmp_path, cases)):
        rr.assert_same(got, rr.run_numpy(c), name)
        ops = [op for op in c["ops"] if op[0] in ("range", "rerank_range")]
        for i, (op, g) in enumerate(zip(ops, got)):
            nq = len(op[1])
            if op[0] == "range":
                diff = rr.same(g, g["xr"])
                assert diff is None and g["xr"]["missing"] == 0, "%s range %d: %s differs from rerank_range of every held key" % (name, i, diff)
                for q in range(nq):
                    lo, hi = int(g["lims"][q]), int(g["lims"][q + 1])
                    size = int(g["knn_sizes"][q])
                    if np.isposinf(op[2][q]) and np.isfinite(g["knn_dist"][q, :size]).all():
                        assert hi - lo == size and np.array_equal(g["keys"][lo:hi], g["knn_keys"][q, :size]), "%s range %d: knn" % (name, i)
                        assert np.array_equal(g["dist"][lo:hi].view(np.uint32), g["knn_dist"][q, :size].view(np.uint32))
            else:
                assert g["missing"] == g["rr_missing"]
                for q in range(nq):
                    lo, hi = int(g["lims"][q]), int(g["lims"][q + 1])
                    size = int(g["rr_sizes"][q])
                    if np.isposinf(op[4][q]) and np.isfinite(g["rr_dist"][q, :size]).all():
                        assert hi - lo == size and np.array_equal(g["keys"][lo:hi], g["rr_keys"][q, :size]), "%s rerank_range %d: rerank" % (name, i)
                        assert np.array_equal(g["dist"][lo:hi].view(np.uint32), g["rr_dist"][q, :size].view(np.uint32))


def some_radii(rng, vec, q):
    """per query a radius that keeps a part of the rows: a quantile of its float64 distances"""
    d = ((vec[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(-1)
    return np.array([np.quantile(d[i], rng.uniform(0.1, 0.9)) for i in range(len(q))], F32)


def filter_ops(rng, q, radius, lo, rows):
    keys = np.arange(lo, lo + rows, dtype=np.int64)
    inside = rng.choice(keys, rows // 3, replace=False)
    across = np.concatenate([np.arange(max(0, lo - 5), lo + 7), np.arange(lo + rows - 7, min(2 ** 32, lo + rows + 5))])
    outside = np.array([k for k in (lo - 40, lo - 1, lo + rows, lo + rows + 33) if 0 <= k < 2 ** 32], np.int64)
    ops = []
    for mode in ("exclude", "allow"):
        ops += [rr.range_(q, radius, (mode, s)) for s in (inside, across, outside, np.zeros(0, np.uint32), keys)]
    return ops


def exact_radius_ops(c, q, tmp_path, exe):
    """range calls whose radius equals one row's distance bit for bit, taken from the twin's radius +inf result"""
    base = rr.run_twin(exe, tmp_path, [dict(c, ops=c["ops"] + [rr.range_(q, INF)])])[0][-1]
    ops = []
    for count in (0, 1, 5):
        ops.append(rr.range_(q, np.array([rr.radius_keeping(base, i, count, strict=False) for i in range(len(q))], F32)))
    return ops


@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_the_twin_equals_the_numpy_restatement_on_a_dense_store(driver, tmp_path, dtype):
    rng = np.random.default_rng(61 + rr.DTYPES[dtype])
    cases, names = [], []
    for dim in DIMS:
        rows = 120 if dim < 4096 else 30
        lo = 1000
        vec = rng.normal(size=(rows, dim)).astype(F32)
        q = rng.normal(size=(3, dim)).astype(F32)
        part = some_radii(rng, vec, q)
        c = rr.dense_case(dim, dtype, lo, vec, [])
        ops = [rr.range_(q, part), rr.range_(q, INF)] + [rr.range_(q, r) for r in RADII] + exact_radius_ops(c, q, tmp_path, driver)
        ops += [rr.range_(q, np.array([np.nan, part[1], 0.0], F32))]
        if dim in (1, 65, 256):
            ops += filter_ops(rng, q, part * F32(2), lo, rows)
        segs = [rng.integers(lo - 3, lo + rows + 3, n) for n in (0, 1, 90)]
        segs[2][:10] = segs[2][10:20]                                          # keys listed twice
        ops += [rr.rerank_range(q, segs, INF), rr.rerank_range(q, segs, part * F32(2)), rr.rerank_range(q, segs, np.nan),
                rr.rerank_range(q, [[0xFFFFFFFF, lo], [], [lo + 1] * 7], INF)]
        cases.append(dict(c, ops=c["ops"] + ops))
        names.append("dim %d %s" % (dim, dtype))
    nf = rc.nonfinite_case(rng, 65, "f32")
    vec, q = nf["adds"][0][1], nf["queries"]
    cases.append(rr.dense_case(65, dtype, 0, vec, [rr.range_(q, INF), rr.range_(q, rr.FLT_MAX), rr.range_(q, 50.0),
                                                    rr.rerank_range(q, [np.arange(30)] * 4, INF)]))
    names.append("non-finite rows and queries")
    hi = rng.normal(size=(90, 8)).astype(F32)
    cases.append(rr.dense_case(8, dtype, 2 ** 32 - 90, hi, [rr.range_(hi[:2], 6.0), rr.range_(hi[:2], INF, ("allow", [2 ** 32 - 1, 2 ** 32 - 90])),
                                                            rr.rerank_range(hi[:2], [[2 ** 32 - 1, 2 ** 32 - 2, 5], [2 ** 32 - 91]], INF)]))
    names.append("keys up to 2^32 - 1")
    if dtype == "f16":
        h = rc.half_range_case(rng, 65)
        cases.append(rr.case(False, 65, "f16", [rr.add(0, h["adds"][0][1]), rr.range_(h["queries"], INF), rr.range_(h["queries"], 1e-9),
                                                rr.range_(h["queries"], 4.0e9)]))
        names.append("half range")
    if dtype != "sq8":
        cases.append(rr.case(False, 8, dtype, [rr.range_(np.zeros((3, 8), F32), INF), rr.rerank_range(np.zeros((2, 8), F32), [[1, 2], []], INF)]))
        names.append("an empty store")
    check(driver, tmp_path, cases, names)


@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_the_twin_equals_the_numpy_restatement_on_a_keyed_store(driver, tmp_path, dtype):
    rng = np.random.default_rng(71 + rr.DTYPES[dtype])
    cases, names = [], []
    for dim in (1, 65, 128):
        labels = rng.choice(2 ** 32 - 1, 150, replace=False).astype(np.uint32)
        labels[:3] = (0, 0xFFFFFFFE, 0xFFFFFFFD)
        vec = rng.normal(size=(150, dim)).astype(F32)
        q = rng.normal(size=(3, dim)).astype(F32)
        part = some_radii(rng, vec, q)
        segs = [labels[:40], labels[30:120][::-1], np.concatenate([labels[:5], labels[:5], [7, 0xFFFFFFFF]])]
        ops = [rr.range_(q, INF), rr.put(labels[:100], vec[:100]), rr.range_(q, INF), rr.range_(q, part), rr.rerank_range(q, segs, INF),
               rr.remove(labels[10:60:2]), rr.range_(q, INF), rr.rerank_range(q, segs, INF), rr.rerank_range(q, segs, part),
               rr.put(labels[50:], vec[:100] + F32(1)), rr.range_(q, part * F32(2)), rr.range_(q, INF, ("exclude", labels[:75])),
               rr.range_(q, INF, ("allow", labels[70:80])), rr.range_(q, INF, ("allow", [])), rr.remove(labels), rr.range_(q, INF),
               rr.rerank_range(q, segs, INF), rr.put(labels[:2], vec[:2]), rr.range_(q, INF)]
        vmin, step = rr.sq_params(np.concatenate([vec, vec + F32(1)])) if dtype == "sq8" else (None, None)
        cases.append(rr.case(True, dim, dtype, ops, vmin, step))
        names.append("keyed dim %d %s" % (dim, dtype))
    check(driver, tmp_path, cases, names)


def test_the_cases_hold_what_they_are_built_for(driver, tmp_path):
    rng = np.random.default_rng(5)
    vec = rng.normal(size=(40, 4)).astype(F32)
    q = vec[:1] + F32(0.25)
    c = rr.dense_case(4, "f32", 100, vec, [])
    base = rr.run_twin(driver, tmp_path, [dict(c, ops=c["ops"] + [rr.range_(q, INF)])])[0][0]
    assert rr.kept(base).tolist() == [40] and (np.diff(base["dist"]) > 0).all()
    r5 = rr.radius_keeping(base, 0, 5)
    ops = [rr.range_(q, r) for r in (r5, np.nextafter(r5, INF), np.nan, 0.0, -0.0, -3.0, rr.FLT_MAX, rr.SUBNORMAL)]
    ops += [rr.rerank_range(q, [[100, 100, 139, 140, 99, 0xFFFFFFFF, 139]], INF), rr.rerank_range(q, [[]], INF)]
    got = rr.run_twin(driver, tmp_path, [dict(c, ops=c["ops"] + ops)])[0]
    assert [int(rr.kept(g)[0]) for g in got[:8]] == [5, 6, 0, 0, 0, 0, 40, 0]                 # the row AT the radius is out
    assert np.array_equal(got[0]["keys"], base["keys"][:5]) and got[1]["keys"][5] == base["keys"][5]
    assert sorted(got[8]["keys"].tolist()) == [100, 139] and got[8]["missing"] == 3 and got[9]["lims"].tolist() == [0, 0]
    nf = rc.nonfinite_case(rng, 65, "f32")
    n = rr.run_twin(driver, tmp_path, [rr.dense_case(65, "f32", 0, nf["adds"][0][1], [rr.range_(nf["queries"], INF)])])[0][0]
    assert rr.kept(n).tolist() == [27, 0, 0, 0] and np.isfinite(n["dist"]).all()                # no NaN and no +inf distance is kept


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "refine_range_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           rr.EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(9)
    vec = rng.normal(size=(60, 65)).astype(F32)
    labels = rng.choice(2 ** 32 - 1, 60, replace=False).astype(np.uint32)
    q = rng.normal(size=(2, 65)).astype(F32)
    segs = [np.concatenate([labels[:20], labels[:3], [5]]), []]
    cases = [rr.dense_case(65, "f16", 2 ** 32 - 60, vec, [rr.range_(q, INF), rr.range_(q, 120.0, ("exclude", [2 ** 32 - 1])), rr.range_(q, np.nan),
                                                           rr.rerank_range(q, [[2 ** 32 - 1, 0], [2 ** 32 - 60] * 3], 130.0)]),
             rr.dense_case(65, "sq8", 0, vec, [rr.range_(q, 130.0), rr.rerank_range(q, [np.arange(70), [0xFFFFFFFF]], INF)]),
             rr.case(False, 3, "f32", [rr.range_(q[:, :3], INF), rr.rerank_range(q[:, :3], [[], [1]], INF)]),
             rr.case(True, 65, "f32", [rr.put(labels, vec), rr.remove(labels[::3]), rr.range_(q, INF, ("exclude", labels[:7])),
                                       rr.rerank_range(q, segs, 125.0), rr.remove(labels), rr.range_(q, INF), rr.rerank_range(q, segs, INF)])]
    for c, got in zip(cases, rr.run_twin(exe, tmp_path, cases)):
        rr.assert_same(got, rr.run_numpy(c))
