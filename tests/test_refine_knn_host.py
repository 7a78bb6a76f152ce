"""CPU: the host twin of the exhaustive search (refine::knn of quick-adc_amd/host/refine.hpp, driver tests/cpp/refine_knn_host.cpp) —
the written definition of qadc_refine_knn, to which the GPU is held bit for bit.

The twin is compared, bit for bit, with an independent numpy restatement (tests/refine_knn_cases.py: refine_cases.np_distance over
all held rows, the filter applied in numpy, a sort of (distance image, key) words) and with the twin's own rerank fed every held key
that passes, from a key list the driver keeps itself."""
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_knn_cases as kc


@pytest.fixture(scope="module")
def driver():
    return kc.build_driver()


def check(exe, tmp_path, cases, names):
    for name, c, got in zip(names, cases, kc.run_twin(exe, tmp_path, cases)):
        kc.assert_same(got, kc.run_numpy(c), name)
        for i, g in enumerate(got):
            diff = kc.same(g, dict(keys=g["rr_keys"], dist=g["rr_dist"], sizes=g["rr_sizes"]))
            assert diff is None, "%s knn %d: %s differs from rerank of every held key" % (name, i, diff)


def filter_ops(rng, q, R, lo, rows):
    """knn under filters whose spans lie inside, across and outside the key range [lo, lo + rows), an empty ALLOW set, an empty
    EXCLUDE set and EXCLUDE of everything"""
    keys = np.arange(lo, lo + rows, dtype=np.int64)
    inside = rng.choice(keys, rows // 3, replace=False)
    across = np.concatenate([np.arange(max(0, lo - 5), lo + 7), np.arange(lo + rows - 7, min(2 ** 32, lo + rows + 5))])
    outside = np.array([k for k in (lo - 40, lo - 1, lo + rows, lo + rows + 33) if 0 <= k < 2 ** 32], np.int64)
    edges = np.array([lo, lo + rows - 1])                                   # the first and the last key held
    word = np.arange(lo + 32 - lo % 32, lo + 64 - lo % 32)                  # one whole bitmap word of an aligned span
    ops = []
    for mode in ("exclude", "allow"):
        ops += [kc.knn(q, R, (mode, s)) for s in (inside, across, outside, edges, word, np.zeros(0, np.uint32), keys)]
    return ops


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_twin_equals_the_numpy_restatement_on_a_dense_store(driver, tmp_path, dtype):
    rng = np.random.default_rng(31 + rc.DTYPES[dtype])
    cases, names = [], []
    for dim in rc.DIMS:
        small = dim < 4096
        rows = 200 if small else 40
        cases += [kc.from_rerank_case(rc.random_case(rng, dim, dtype, rows, 3, 1, 1), (1, 10, rows - 1, rows, rows + 5)),
                  kc.from_rerank_case(rc.random_case(rng, dim, dtype, 90, 2, 1, 1, lo=2 ** 32 - 90, scale=100.0), (30, 95)),   # keys up to 2^32 - 1
                  kc.tie_case(rng, dim, dtype, 15), kc.from_rerank_case(rc.nonfinite_case(rng, dim, dtype), (7, 32))]
        names += ["%s dim %d %s" % (what, dim, dtype) for what in ("random", "high keys", "ties", "non-finite")]
        if dtype == "f16":
            cases.append(kc.from_rerank_case(rc.half_range_case(rng, dim), (48, 50)))
            names.append("half range dim %d" % dim)
        if small:
            vec = rng.normal(size=(rows, dim)).astype(np.float32)
            q = rng.normal(size=(2, dim)).astype(np.float32)
            for lo in (0, 1000):
                cases.append(kc.case(False, dim, dtype, [kc.add(lo, vec)] + filter_ops(rng, q, 20, lo, rows)))
                names.append("filters dim %d lo %d" % (dim, lo))
    cases.append(kc.case(False, 8, dtype, [kc.knn(np.zeros((3, 8), np.float32), 4), kc.knn(np.zeros((1, 8), np.float32), 1, ("allow", [3]))]))
    names.append("an empty store")
    check(driver, tmp_path, cases, names)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_twin_equals_the_numpy_restatement_on_a_keyed_store(driver, tmp_path, dtype):
    rng = np.random.default_rng(41 + rc.DTYPES[dtype])
    cases, names = [], []
    for dim in (1, 65, 128):
        labels = rng.choice(2 ** 32 - 1, 150, replace=False).astype(np.uint32)
        labels[:3] = (0, 0xFFFFFFFE, 0xFFFFFFFD)
        vec = rng.normal(size=(150, dim)).astype(np.float32)
        q = rng.normal(size=(3, dim)).astype(np.float32)
        ops = [kc.knn(q, 5), kc.put(labels[:100], vec[:100]), kc.knn(q, 100), kc.remove(labels[10:60:2]), kc.knn(q, 101),
               kc.put(labels[50:], vec[:100] + np.float32(1)), kc.knn(q, 7), kc.knn(q, 9, ("exclude", labels[:75])),
               kc.knn(q, 9, ("allow", labels[70:80])), kc.knn(q, 9, ("allow", [])), kc.knn(q, 200, ("exclude", [])),
               kc.remove(labels), kc.knn(q, 3), kc.put(labels[:2], vec[:2]), kc.knn(q, 3)]
        cases.append(kc.case(True, dim, dtype, ops))
        names.append("keyed dim %d %s" % (dim, dtype))
    check(driver, tmp_path, cases, names)


def test_the_cases_hold_what_they_are_built_for(driver, tmp_path):
    rng = np.random.default_rng(5)
    tie = kc.tie_case(rng, 96, "f32", 15)
    nonfinite = kc.from_rerank_case(rc.nonfinite_case(rng, 65, "f32"), (32,))
    vec = rng.normal(size=(20, 4)).astype(np.float32)
    flt = kc.case(False, 4, "f32", [kc.add(100, vec), kc.knn(vec[:1], 25, ("allow", [])), kc.knn(vec[:1], 25, ("exclude", np.arange(100, 120))),
                                    kc.knn(vec[:1], 25, ("allow", [99, 100, 119, 120])), kc.knn(vec[:1], 25, ("exclude", [100, 119]))])
    t, n, f = kc.run_twin(driver, tmp_path, [tie, nonfinite, flt])
    lo = 50
    assert t[1]["keys"][0].tolist() == [lo + 10 + i for i in range(5)] and (t[1]["dist"][0].view(np.uint32) == 0).all()
    assert t[2]["keys"][0].tolist() == [lo + 10 + i for i in range(10)] and t[3]["keys"][0, :10].tolist() == t[2]["keys"][0].tolist()
    assert t[3]["dist"][0, 10] > 0 and t[0]["sizes"].tolist() == [15] * 3
    img = n[0]["dist"].view(np.uint32)
    assert n[0]["sizes"].tolist() == [30] * 4 and (n[0]["keys"][:, 30:] == kc.NO_KEY).all() and np.isposinf(n[0]["dist"][:, 30:]).all()
    assert n[0]["keys"][0, 29] == 3 and img[0, 29] == rc.NAN_IMAGE and (img[1, :30] == rc.NAN_IMAGE).all()
    assert n[0]["keys"][1, :30].tolist() == list(range(30))
    assert [int(r["sizes"][0]) for r in f] == [0, 0, 2, 18]
    assert (f[0]["keys"] == kc.NO_KEY).all() and np.isposinf(f[1]["dist"]).all()
    assert sorted(f[2]["keys"][0, :2].tolist()) == [100, 119] and f[2]["keys"][0, 0] == 100 and f[2]["dist"][0, 0] == 0


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "refine_knn_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           kc.EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(9)
    vec = rng.normal(size=(60, 65)).astype(np.float32)
    labels = rng.choice(2 ** 32 - 1, 60, replace=False).astype(np.uint32)
    q = rng.normal(size=(2, 65)).astype(np.float32)
    cases = [kc.tie_case(rng, 65, "f16", 15), kc.from_rerank_case(rc.nonfinite_case(rng, 1, "f32"), (5, 40)),
             kc.case(False, 65, "f32", [kc.knn(q, 3), kc.add(2 ** 32 - 60, vec)] + filter_ops(rng, q, 70, 2 ** 32 - 60, 60)),
             kc.case(True, 65, "f16", [kc.put(labels, vec), kc.remove(labels[::3]), kc.knn(q, 50, ("exclude", labels[:7])), kc.remove(labels),
                                       kc.knn(q, 2)])]
    for c, got in zip(cases, kc.run_twin(exe, tmp_path, cases)):
        kc.assert_same(got, kc.run_numpy(c))
