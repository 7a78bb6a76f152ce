"""GPU: the probed exact search over a refine store (pyqadc.Refine.knn_probed over qadc_refine_knn_probed)
against its host twin (refine::knn_probed of quick-adc_amd/host/refine.hpp through tests/cpp/refine_probe_host.cpp): keys, the
distances' bit patterns, sizes and the missing count, for equality — there is no tolerance anywhere.  The index has five partitions of
0, 1, 63, 300 and 700 rows; the shapes sit on the edges of the plan (host/refine_probe_plan.hpp): the strips of 64 components a lane
walks, the register and the LDS tile, partitions probed by no query, by one, by a full tile and by one more, and R against the entries."""
import numpy as np
import pytest

import refine_probe_cases as pc
from helpers import path_independent

pytestmark = pytest.mark.gpu
K = len(pc.SIZES)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return pc.build_driver()


def check(pyqadc, twin, tmp_path, cases, names=None, **how):
    wants = pc.run_twin(twin, tmp_path, cases)
    for i, (c, want) in enumerate(zip(cases, wants)):
        pc.assert_same(pc.run_gpu(pyqadc, c, **how), want, names[i] if names else "case %d" % i)
    return wants


def tile_calls(rng, q, nqs, R=10):
    """per nq: ma = 1 with every query on partition 4 (probed by nq queries: short tiles, a full one, a second one; the others by
    none); ma = 2 with query 0 alone on (3, 2), the last query on the empty partition twice and the others on (4, 0); ma = K"""
    calls = []
    for n in nqs:
        two = np.tile(np.array([4, 0], np.int32), (n, 1))
        two[0] = (3, 2)
        two[n - 1] = (0, 0)
        calls += [pc.call(q[:n], np.full((n, 1), 4, np.int32), R), pc.call(q[:n], two, R), pc.call(q[:n], pc.probes(rng, n, K, K), R)]
    return calls


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 128, 4096])
def test_dims_tiles_probes_and_R(pyqadc, twin, tmp_path, dim, dtype):
    rng = np.random.default_rng(dim + pc.DTYPES[dtype])
    nqs = (1, 3, 4, 5, 31, 32, 33, 65) if dim < 4096 else (1, 3, 4, 5, 9)      # (LDS tiles hold 4 queries at dim 4096)
    q = rng.normal(size=(max(nqs), dim)).astype(np.float32)
    rows = pc.SIZES[2] + pc.SIZES[3]                                         # the entries of a query on partitions 2 and 3

    def calls(vec, labels):
        on23 = np.tile(np.array([2, 3], np.int32), (5, 1))
        return (tile_calls(rng, q, nqs) + [pc.call(q[:5], on23, R) for R in (1, rows - 1, rows, rows + 5, 1024)] +
                [pc.call(q[:5], pc.probes(rng, 5, K, K), 1024)])
    c = pc.dense_case(rng, dim, dtype, calls, lo=7)
    (want,) = check(pyqadc, twin, tmp_path, [c])
    n = len(nqs) * 3
    assert want[1]["sizes"][0] == 0 and (want[1]["keys"][0] == pc.NO_KEY).all()                # nq = 1, ma = 2: (0, 0), nothing to rank
    assert want[4]["sizes"].tolist() == [10, 10, 0] and np.isposinf(want[4]["dist"][2]).all()  # nq = 3: the last query alone has nothing
    assert [int(w["sizes"][0]) for w in want[n:n + 5]] == [1, rows - 1, rows, rows, rows]
    assert want[n + 5]["sizes"].tolist() == [1024] * 5 and all(w["missing"] == 0 for w in want)


@path_independent
@pytest.mark.parametrize("keyed", [False, True])
def test_missing_labels_and_filters(pyqadc, twin, tmp_path, keyed):
    rng = np.random.default_rng(17 + keyed)
    dim = 96
    q = rng.normal(size=(33, dim)).astype(np.float32)

    def calls(vec, labels):
        pick = rng.choice(labels, 300, replace=False)
        return [pc.call(q, pc.probes(rng, 33, ma, K), R, f) for ma in (1, 2, K) for R in (7, 400)
                for f in (None, ("exclude", pick), ("allow", pick), ("allow", []))]
    c = pc.dense_case(rng, dim, "f32", calls, lo=100, keyed=keyed)
    lab = [np.array(p[0]) for p in c["parts"]]
    lab[3][::7] = np.arange(50000, 50000 + len(lab[3][::7]))                 # labels the store does not hold
    lab[4][5] = 0xFFFFFFFF
    c["parts"] = [pc.part(l) for l in lab]
    want = check(pyqadc, twin, tmp_path, [c])[0]
    assert want[0]["missing"] > 0 and want[3]["sizes"].max() == 0
    c["index_filter"] = ("exclude", lab[4][:300])
    check(pyqadc, twin, tmp_path, [c])
