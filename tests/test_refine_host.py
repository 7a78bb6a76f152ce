"""CPU: the host twin of exact re-ranking (quick-adc_amd/host/refine.hpp, driver tests/cpp/refine_host.cpp) — the written
definition of qadc_refine_rerank, to which the GPU store is held bit for bit.

The twin is compared, bit for bit, with an independent numpy restatement of the definition (tests/refine_cases.py: the distance
as 64 strided partial sums plus six halvings, the selection as a sort of (distance image, key) words), and its distance with
float64 on the same float32 inputs."""
import subprocess

import numpy as np
import pytest

import refine_cases as rc


@pytest.fixture(scope="module")
def driver():
    return rc.build_driver()


def check(exe, tmp_path, cases, names):
    for name, c, got in zip(names, cases, rc.run_twin(exe, tmp_path, cases)):
        assert got["refused"] == 0, name
        diff = rc.same(got, rc.np_rerank(c))
        assert diff is None, "%s: %s differs" % (name, diff)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_twin_equals_the_numpy_restatement(driver, tmp_path, dtype):
    rng = np.random.default_rng(11 + rc.DTYPES[dtype])
    cases, names = [], []
    for dim in rc.DIMS:
        small = dim < 4096
        cases += [rc.random_case(rng, dim, dtype, 200 if small else 40, 3, 65 if small else 20, 10, lo=0),
                  rc.random_case(rng, dim, dtype, 90, 2, 17, 30, lo=2 ** 32 - 90, scale=100.0),   # R above the survivors; keys up to 2^32 - 1
                  rc.edge_case(rng, dim, dtype), rc.nonfinite_case(rng, dim, dtype)]
        names += ["%s dim %d %s" % (what, dim, dtype) for what in ("random", "high keys", "edges", "non-finite")]
        if dtype == "f16":
            cases.append(rc.half_range_case(rng, dim))
            names.append("half range dim %d" % dim)
    check(driver, tmp_path, cases, names)


def test_the_edge_case_holds_what_it_is_built_for(driver, tmp_path):
    c = rc.edge_case(np.random.default_rng(5), 96, "f32")
    (got,) = rc.run_twin(driver, tmp_path, [c])
    lo = c["adds"][0][0]
    assert got["missing"] == 4
    assert got["sizes"].tolist()[1:] == [1, 6, 0, 0] and got["sizes"][0] == 6
    assert got["keys"][0].tolist() == [lo + 10 + i for i in range(6)] and (got["dist"][0].view(np.uint32) == 0).all()   # the tie, by key
    assert got["keys"][1].tolist() == [lo + 7] + [rc.NO_KEY] * 5 and np.isposinf(got["dist"][1, 1:]).all()
    for q in (3, 4):
        assert (got["keys"][q] == rc.NO_KEY).all() and np.isposinf(got["dist"][q]).all()
    assert (np.diff(got["dist"][2].astype(np.float64)) >= 0).all() and len(set(got["keys"][2].tolist())) == 6


def test_nan_distances_come_last_as_the_canonical_nan(driver, tmp_path):
    c = rc.nonfinite_case(np.random.default_rng(6), 65, "f32")
    (got,) = rc.run_twin(driver, tmp_path, [c])
    img = got["dist"].view(np.uint32)
    assert got["sizes"].tolist() == [30] * 4
    assert got["keys"][0, 29] == 3 and img[0, 29] == rc.NAN_IMAGE and np.isposinf(got["dist"][0, 27:29]).all()
    assert (img[1, :30] == rc.NAN_IMAGE).all() and got["keys"][1, :30].tolist() == list(range(30))
    assert got["keys"][2, 29] in (3, 4) and (img[2, 28:30] == rc.NAN_IMAGE).all() and np.isposinf(got["dist"][2, :28]).all()
    assert (got["keys"][:, 30:] == rc.NO_KEY).all() and np.isposinf(got["dist"][:, 30:]).all()


def test_an_add_must_continue_the_store(driver, tmp_path):
    dim = 8
    v = np.random.default_rng(7).normal(size=(10, dim)).astype(np.float32)
    q, keys = v[:1], np.arange(100, 110, dtype=np.uint32)
    ok = rc.case(dim, "f32", [(100, v[:4]), (104, v[4:])], q, keys, 10)
    gap = rc.case(dim, "f32", [(100, v[:4]), (105, v[4:])], q, keys, 10)
    back = rc.case(dim, "f32", [(100, v[:4]), (100, v[4:])], q, keys, 10)
    past = rc.case(dim, "f32", [(2 ** 32 - 9, v)], q, keys, 10)
    got = rc.run_twin(driver, tmp_path, [ok, gap, back, past])
    assert [g["refused"] for g in got] == [0, 1, 1, 1]
    assert got[0]["sizes"][0] == 10 and got[1]["sizes"][0] == 4 and got[1]["missing"] == 6 and got[3]["sizes"][0] == 0


@pytest.mark.parametrize("dim", rc.DIMS)
def test_the_twin_distance_is_close_to_float64(driver, tmp_path, dim):
    """relative error at most (ceil(dim / 64) + 10) * 2^-24 on finite cases: three roundings per term (the difference, the product,
    its add) and one per add along the longest chain of non-negative sums, ceil(dim / 64) strip adds and six halvings"""
    rng = np.random.default_rng(dim)
    rows = 64
    c = rc.random_case(rng, dim, "f32", rows, 4, rows, rows)
    c["keys"][:] = np.arange(rows, dtype=np.uint32)
    (got,) = rc.run_twin(driver, tmp_path, [c])
    vec = c["adds"][0][1].astype(np.float64)
    bound = (-(-dim // 64) + 10) * 2.0 ** -24
    for q in range(4):
        exact = ((c["queries"][q].astype(np.float64)[None, :] - vec) ** 2).sum(1)
        d = got["dist"][q].astype(np.float64)
        assert got["sizes"][q] == rows
        rel = np.abs(d - exact[got["keys"][q]]) / exact[got["keys"][q]]
        assert rel.max() <= bound, (dim, rel.max(), bound)


def test_the_half_conversion_equals_numpy_on_every_finite_half_boundary(driver, tmp_path):
    """every half value, the float midway to its successor and the floats next to that midpoint, as one-dimensional rows: the
    distance to the query 0 is the stored value squared, so a wrong rounding of any of them shows"""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    nxt = np.arange(1, 0x7C01, dtype=np.uint16).view(np.float16).astype(np.float64)
    mid = ((h.astype(np.float64) + np.where(np.isinf(nxt), 65536.0, nxt)) / 2).astype(np.float32)      # exact in float32
    vals = np.concatenate([h, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))]).astype(np.float32)
    vals = np.concatenate([vals, -vals])
    cases = []
    for first in range(0, len(vals), 8192):
        chunk = vals[first:first + 8192]
        cases.append(rc.case(1, "f16", [(0, chunk.reshape(-1, 1))], np.zeros((1, 1), np.float32), np.arange(len(chunk), dtype=np.uint32), len(chunk)))
    for c, got in zip(cases, rc.run_twin(driver, tmp_path, cases)):
        assert rc.same(got, rc.np_rerank(c)) is None


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "refine_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           rc.EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(9)
    cases = [rc.edge_case(rng, 65, "f16"), rc.nonfinite_case(rng, 1, "f32"), rc.half_range_case(rng, 63),
             rc.random_case(rng, 128, "f32", 300, 2, 64, 70, lo=2 ** 32 - 300)]
    for c, got in zip(cases, rc.run_twin(exe, tmp_path, cases)):
        assert rc.same(got, rc.np_rerank(c)) is None
