"""GPU: the exhaustive search over a refine store (pyqadc.Refine.knn over qadc_refine_knn) against its host
twin (refine::knn of quick-adc_amd/host/refine.hpp through tests/cpp/refine_knn_host.cpp): keys, the distances' bit patterns and
sizes, for equality — there is no tolerance anywhere.  The shapes sit on the edges of the plan (host/refine_knn_plan.hpp): the
strips of 64 components a lane walks, the register and the LDS tile, the tiles of 32 and of 4 queries, the chunks, groups and
launches the rows are walked in, and R against the rows held."""
import numpy as np
import pytest

import refine_cases as rc
import refine_knn_cases as kc
from helpers import path_independent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return kc.build_driver()


def check(pyqadc, twin, tmp_path, cases, names=None, **how):
    wants = kc.run_twin(twin, tmp_path, cases)
    for i, (c, want) in enumerate(zip(cases, wants)):
        kc.assert_same(kc.run_store(pyqadc, c, **how), want, names[i] if names else "case %d" % i)
    return wants


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 128, 4096])
def test_dims_tiles_and_R(pyqadc, twin, tmp_path, dim, dtype):
    """nq at the edges of the plan's tile — 32 queries in registers up to dim 128 (4 for calls of at most 4 queries), 4 in LDS at
    dim 4096 — and R against the rows held"""
    rng = np.random.default_rng(dim + rc.DTYPES[dtype])
    rows = 300 if dim < 4096 else 600
    nqs = (1, 3, 4, 5, 9, 31, 32, 33, 65) if dim < 4096 else (1, 3, 4, 5, 9)
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    q = rng.normal(size=(max(nqs), dim)).astype(np.float32)
    ops = [kc.add(7, vec)] + [kc.knn(q[:n], R) for n in nqs for R in (1, rows - 1, rows, rows + 5)] + [kc.knn(q[:5], kc.MAX_R)]
    (want,) = check(pyqadc, twin, tmp_path, [kc.case(False, dim, dtype, ops)])
    assert want[2]["sizes"].tolist() == [rows] and want[3]["sizes"].tolist() == [rows] and (want[3]["keys"][0, rows:] == kc.NO_KEY).all()


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("rows", [kc.CHUNK - 1, kc.CHUNK, kc.CHUNK + 1, 3 * kc.CHUNK + 1, 8 * kc.CHUNK + 1],
                         ids=["chunk-1", "chunk", "chunk+1", "3chunk+1", "8chunk+1"])
def test_rows_at_the_default_chunks_edges(pyqadc, twin, tmp_path, rows, dtype):
    """one group, a second group of one row, four groups, and (eight groups of 7168 rows being a launch) a second launch of one row"""
    rng = np.random.default_rng(rows)
    dim = 3
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    q = rng.normal(size=(5, dim)).astype(np.float32)
    check(pyqadc, twin, tmp_path, [kc.case(False, dim, dtype, [kc.add(2 ** 32 - rows, vec), kc.knn(q, 10), kc.knn(q[:1], kc.MAX_R)])])


@path_independent
@pytest.mark.parametrize("order", ["far-to-near", "near-to-far"])
def test_rows_ordered_by_distance(pyqadc, twin, tmp_path, order):
    """far to near every chunk beats the bound its group has so far; near to far none does after the first"""
    rng = np.random.default_rng(3)
    dim, rows = 4, 20000
    radius = np.sort(rng.random(rows).astype(np.float32) * 100 + 1)
    if order == "far-to-near":
        radius = radius[::-1]
    unit = rng.normal(size=(rows, dim))
    vec = (unit / np.linalg.norm(unit, axis=1, keepdims=True) * radius[:, None]).astype(np.float32)
    q = (rng.normal(size=(3, dim)) * 0.01).astype(np.float32)
    c = kc.case(False, dim, "f32", [kc.add(0, vec), kc.knn(q, 100), kc.knn(q, 1)])
    (want,) = check(pyqadc, twin, tmp_path, [c])
    kc.assert_same(kc.run_store(pyqadc, c, plan=(64, 0)), want, "chunks of 64 rows")
    near = want[0]["keys"][0]
    assert (near >= rows - 200).all() if order == "far-to-near" else (near < 200).all()


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ties_and_non_finite_and_half_range(pyqadc, twin, tmp_path, dtype):
    rng = np.random.default_rng(21)
    cases, names = [], []
    for dim in rc.DIMS:
        cases += [kc.tie_case(rng, dim, dtype, 15), kc.from_rerank_case(rc.nonfinite_case(rng, dim, dtype), (7, 32))]
        names += ["ties dim %d" % dim, "non-finite dim %d" % dim]
        if dtype == "f16":
            cases.append(kc.from_rerank_case(rc.half_range_case(rng, dim), (48, 50)))
            names.append("half range dim %d" % dim)
    wants = check(pyqadc, twin, tmp_path, cases, names)
    assert wants[0][1]["keys"][0].tolist() == [60, 61, 62, 63, 64]                           # R = 5 cuts the tie, by key
    assert (wants[1][1]["dist"].view(np.uint32)[1, :30] == rc.NAN_IMAGE).all()


@path_independent
def test_a_tie_across_chunks_groups_and_launches(pyqadc, twin, tmp_path):
    """ten identical rows spread over the store so that, in chunks of 64 rows, they lie in different chunks, groups and launches"""
    rng = np.random.default_rng(22)
    dim, rows = 96, 1500
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    same = np.array([0, 63, 64, 65, 127, 511, 512, 1023, 1024, 1499])
    vec[same] = vec[0]
    q = np.stack([vec[0], vec[1]])
    c = kc.case(False, dim, "f32", [kc.add(100, vec)] + [kc.knn(q, R) for R in (1, 5, 9, 10, 11)])
    (want,) = check(pyqadc, twin, tmp_path, [c], plan=(64, 0))
    assert want[3]["keys"][0].tolist() == (same + 100).tolist() and (want[3]["dist"][0].view(np.uint32) == 0).all()
    kc.assert_same(kc.run_store(pyqadc, c), want, "the default plan")


@path_independent
def test_no_plan_shows_in_the_result(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(23)
    dim, rows, nq = 65, 3000, 33
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[1000:1010] = vec[20]
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    q[0] = vec[20]
    c = kc.case(False, dim, "f16", [kc.add(0, vec), kc.knn(q, 7), kc.knn(q, 1000)])
    (want,) = kc.run_twin(twin, tmp_path, [c])
    for plan in [(0, 0), (64, 0), (64, 1), (100, 7), (1000, 32), (7168, 33), (1, 16), (65, 31)]:
        kc.assert_same(kc.run_store(pyqadc, c, plan=plan), want, "chunk_rows %d, pass_nq %d" % plan)


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_knn_is_rerank_of_every_key(pyqadc, dtype):
    rng = np.random.default_rng(24)
    dim, rows, lo, nq = 128, 8192, 1000, 5
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[100:110] = vec[5]
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    st = pyqadc.Refine(dim, dtype)
    st.add(vec, lo)
    keys = np.tile(np.arange(lo, lo + rows, dtype=np.uint32), (nq, 1))
    for R in (1, 100, 1024):
        k, d, s, missing = st.rerank(q, keys, R)
        gk, gd, gs = st.knn(q, R)
        assert missing == 0 and kc.same(dict(keys=gk, dist=gd, sizes=gs), dict(keys=k, dist=d, sizes=s)) is None, R
    st.close()


@path_independent
def test_corner_cases_and_refusals(pyqadc):
    E = "qadc error %d:" % pyqadc.QADC_E_ARG
    q = np.zeros((3, 8), np.float32)
    for keyed in (False, True):
        st = pyqadc.Refine(8, "f32", keyed=keyed)
        k, d, s = st.knn(q, 4)                                                                 # an empty store
        assert s.tolist() == [0, 0, 0] and (k == kc.NO_KEY).all() and np.isposinf(d).all()
        k, d, s = st.knn_raw(0, None, 4, outputs=False)                                        # nq = 0: a no-op, no array needed
        for R in (0, -1, kc.MAX_R + 1):
            with pytest.raises(pyqadc.QadcError, match=E):
                st.knn(q, R)
        with pytest.raises(pyqadc.QadcError, match=E):
            st.knn_raw(3, None, 4)
        with pytest.raises(pyqadc.QadcError, match=E):
            st.knn_raw(3, q, 4, outputs=False)
        with pytest.raises(pyqadc.QadcError, match=E):
            st.knn_raw(-1, q, 4)
        with pytest.raises(pyqadc.QadcError, match=E):
            st.set_knn_plan(kc.CHUNK + 1, 0)
        with pytest.raises(pyqadc.QadcError, match=E):
            st.set_knn_plan(0, -1)
        st.close()
    assert pyqadc.lib().qadc_refine_knn(None, 3, None, 4, None, None, None, None) == pyqadc.QADC_E_ARG
    assert pyqadc.lib().qadc_refine_set_knn_plan(None, 0, 0) == pyqadc.QADC_E_ARG
