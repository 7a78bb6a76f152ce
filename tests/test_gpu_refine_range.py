"""GPU: the exact range search over a refine store (pyqadc.Refine.range over qadc_refine_range) against its
host twin (refine::range of quick-adc_amd/host/refine.hpp through tests/cpp/refine_range_host.cpp): lims, keys and the distances'
bit patterns, for equality — there is no tolerance anywhere.  The shapes sit on the edges of the plan
(host/refine_range_plan.hpp): the strips of 64 components a lane walks, the register and the LDS tile (dim 256 | 257), the tiles of
32 and of 4 queries, the regions and their re-run, the chunks, groups and launches the rows are walked in, the LDS and the radix form
of the sort, and every kind of radius."""
import numpy as np
import pytest

import refine_cases as rc
import refine_range_cases as rr
from helpers import path_independent

pytestmark = pytest.mark.gpu

INF, F32 = rr.INF, np.float32


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return rr.build_driver()


def check(pyqadc, twin, tmp_path, cases, names=None, **how):
    wants = rr.run_twin(twin, tmp_path, cases)
    for i, (c, want) in enumerate(zip(cases, wants)):
        rr.assert_same(rr.run_store(pyqadc, c, **how), want, names[i] if names else "case %d" % i)
    return wants


def quantile_radii(rng, vec, q, lo=0.05, hi=0.6):
    d = ((vec[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(-1)
    return np.array([np.quantile(d[i], rng.uniform(lo, hi)) for i in range(len(q))], F32)


def radii_keeping(twin, tmp_path, c, q, counts):
    """per query of q a radius under which it keeps exactly counts[i] rows of case c's store (its distances there are distinct)"""
    base = rr.run_twin(twin, tmp_path, [dict(c, ops=c["ops"] + [rr.range_(q, INF)])])[0][-1]
    return np.array([rr.radius_keeping(base, i, n) for i, n in enumerate(counts)], F32)


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 128, 256, 257, 4096])
def test_dims_tiles_and_queries(pyqadc, twin, tmp_path, dim, dtype):
    """nq at the edges of the plan's tile — 32 queries in registers (16 above dim 128, 4 for calls of at most 4 queries), in LDS above
    dim 256 — on the host form and on the device form"""
    rng = np.random.default_rng(dim + rr.DTYPES[dtype])
    rows = 300 if dim < 4096 else 100
    nqs = (1, 3, 4, 5, 31, 32, 33, 65)                                   # (dim 4096: tiles of 4 queries in LDS)
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(max(nqs), dim)).astype(F32)
    radius = quantile_radii(rng, vec, q)
    c = rr.dense_case(dim, dtype, 7, vec, [rr.range_(q[:n], radius[:n]) for n in nqs] + [rr.range_(q[:5], INF)])
    (want,) = check(pyqadc, twin, tmp_path, [c])
    check(pyqadc, twin, tmp_path, [c], device=True)
    assert rr.kept(want[-1]).tolist() == [rows] * 5 and 0 < rr.kept(want[-2]).min() and rr.kept(want[-2]).max() < rows


@path_independent
def test_regions_at_their_edges_and_the_rerun(pyqadc, twin, tmp_path):
    """regions of 64 words: queries that keep 0, 1, 63, 64, 65 and all rows in one call; range_reruns moves exactly when a region
    overflowed; the result is the default plan's"""
    rng = np.random.default_rng(1)
    dim, rows = 3, 400
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(6, dim)).astype(F32)
    c = rr.dense_case(dim, "f32", 0, vec, [])
    counts = [0, 1, 63, 64, 65, rows]
    radius = radii_keeping(twin, tmp_path, c, q, counts)
    ops = [rr.range_(q[:4], radius[:4]), rr.range_(q, radius), rr.range_(q[3:5], radius[3:5]), rr.range_(q[:4], radius[:4])]
    c = dict(c, ops=c["ops"] + ops)
    want = rr.run_twin(twin, tmp_path, [c])[0]
    assert [rr.kept(w).tolist() for w in want] == [counts[:4], counts, counts[3:5], counts[:4]]
    reruns = []
    rr.assert_same(rr.run_store(pyqadc, c, plan=(64, 0, 0), reruns=reruns), want, "regions of 64")
    assert reruns == [0, 1, 2, 2]                                        # 64 rows fill a region, 65 overflow it
    reruns = []
    rr.assert_same(rr.run_store(pyqadc, c, plan=(64, 0, 2), reruns=reruns), want, "regions of 64, passes of 2 queries")
    assert reruns == [0, 1, 2, 2]                                        # of the passes (0, 1), (63, 64), (65, all) only the last re-runs
    reruns = []
    rr.assert_same(rr.run_store(pyqadc, c, reruns=reruns), want, "the default plan")
    assert reruns == [0, 0, 0, 0]
    rr.assert_same(rr.run_store(pyqadc, c, plan=(1, 0, 0), device=True), want, "regions of 1")


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("rows", [rr.CHUNK - 1, rr.CHUNK, rr.CHUNK + 1, 8 * rr.CHUNK + 1], ids=["chunk-1", "chunk", "chunk+1", "8chunk+1"])
def test_rows_at_the_default_chunks_edges(pyqadc, twin, tmp_path, rows, dtype):
    """one group, a second group of one row, and (eight groups of 7168 rows being a launch) a second launch of one row"""
    rng = np.random.default_rng(rows)
    dim = 3
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(5, dim)).astype(F32)
    q[4] = vec[rows - 1]                                                 # the last row is at distance 0 from query 4
    radius = np.array([0.05, 0.3, np.inf, 1e-3, 1e-4], F32)
    (want,) = check(pyqadc, twin, tmp_path, [rr.dense_case(dim, dtype, 2 ** 32 - rows, vec, [rr.range_(q, radius)])])
    assert rr.kept(want[0])[2] == rows and want[0]["keys"][int(want[0]["lims"][4])] == 2 ** 32 - 1


@path_independent
def test_identical_rows_across_chunks_groups_and_launches(pyqadc, twin, tmp_path):
    """ten identical rows spread over the store so that, in chunks of 64 rows, they lie in different chunks, groups and launches:
    they come out side by side, by key"""
    rng = np.random.default_rng(22)
    dim, rows = 96, 1500
    vec = rng.normal(size=(rows, dim)).astype(F32)
    at = np.array([0, 63, 64, 130, 511, 512, 700, 1023, 1024, 1499])
    vec[at] = vec[0]
    q = rng.normal(size=(3, dim)).astype(F32)
    q[0] = vec[0]
    c = rr.dense_case(dim, "f32", 100, vec, [rr.range_(q, np.array([1e-9, np.inf, 150.0], F32))])
    (want,) = check(pyqadc, twin, tmp_path, [c], plan=(0, 64, 0))
    check(pyqadc, twin, tmp_path, [c], plan=(16, 1, 2))
    assert want[0]["keys"][:10].tolist() == (at + 100).tolist() and rr.kept(want[0])[0] == 10


@path_independent
def test_a_query_keeps_4095_4096_and_4097_rows(pyqadc, twin, tmp_path):
    """the LDS form of the sort up to 4096 words, the radix form above"""
    rng = np.random.default_rng(4)
    dim, rows = 3, 6000
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = np.tile(rng.normal(size=(1, dim)).astype(F32), (4, 1))
    c = rr.dense_case(dim, "f32", 0, vec, [])
    counts = [rr.SORT_LDS - 1, rr.SORT_LDS, rr.SORT_LDS + 1, 2]
    radius = radii_keeping(twin, tmp_path, c, q, counts)
    c = dict(c, ops=c["ops"] + [rr.range_(q, radius)])
    (want,) = check(pyqadc, twin, tmp_path, [c])
    assert rr.kept(want[0]).tolist() == counts
    check(pyqadc, twin, tmp_path, [c], plan=(5000, 0, 0), device=True)    # no re-run: the first run's regions hold them


@path_independent
def test_the_radix_sort_with_every_digit_and_with_key_digits_alone(pyqadc, twin, tmp_path):
    """a keyed store of random 32-bit labels whose distances span many binades: every byte of the word differs somewhere, so every
    radix pass runs; and rows that are all the same vector: only the key's digits differ"""
    rng = np.random.default_rng(6)
    n = 5000
    labels = rng.choice(2 ** 32 - 1, n, replace=False).astype(np.uint32)
    x = (np.exp2(rng.uniform(-60, 60, n)) * (1 + rng.random(n))).astype(F32).reshape(n, 1)
    q = np.zeros((1, 1), F32)
    spread = rr.case(True, 1, "f32", [rr.put(labels, x), rr.range_(q, INF)])
    flat = rr.dense_case(3, "f32", 0, np.tile(rng.normal(size=(1, 3)).astype(F32), (n, 1)), [rr.range_(np.ones((2, 3), F32), INF)])
    want = check(pyqadc, twin, tmp_path, [spread, flat])
    w = (want[0][0]["dist"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | want[0][0]["keys"].astype(np.uint64)
    differ = int(np.bitwise_or.reduce(w) ^ np.bitwise_and.reduce(w))
    assert len(w) == n and all((differ >> (8 * d)) & 255 for d in range(8)), "a digit of the word is the same everywhere"
    assert len(set(want[1][0]["dist"].view(np.uint32).tolist())) == 1 and rr.kept(want[1][0]).tolist() == [n, n]


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_every_kind_of_radius(pyqadc, twin, tmp_path, dtype):
    """NaN, +inf, 0, -0, negative, FLT_MAX and a subnormal; a radius equal to one row's distance bit for bit; rows and queries with NaN
    and infinite components; f16 rows at the half range"""
    rng = np.random.default_rng(8 + rr.DTYPES[dtype])
    dim, rows = 65, 200
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(7, dim)).astype(F32)
    q[6] = vec[11]                                                        # distance +0 to row 11 (exactly, on an f32 store)
    c = rr.dense_case(dim, dtype, 50, vec, [])
    edge = np.array([np.nan, np.inf, 0.0, -0.0, -1.0, rr.FLT_MAX, 0.0], F32)
    edge.view(np.uint32)[6] = 1                                           # the smallest subnormal, by its bits: no conversion may flush it
    base = rr.run_twin(twin, tmp_path, [dict(c, ops=c["ops"] + [rr.range_(q, INF)])])[0][-1]
    exact = np.array([rr.radius_keeping(base, i, 9, strict=False) for i in range(7)], F32)
    ops = [rr.range_(q, edge), rr.range_(q, exact), rr.range_(q, np.nextafter(exact, INF)), rr.range_(q, np.roll(edge, 3))]
    nf = rc.nonfinite_case(rng, dim, "f32")
    cases = [dict(c, ops=c["ops"] + ops),
             rr.dense_case(dim, dtype, 0, nf["adds"][0][1], [rr.range_(nf["queries"], r) for r in (INF, rr.FLT_MAX, 60.0)])]
    if dtype == "f16":
        h = rc.half_range_case(rng, dim)
        cases.append(rr.case(False, dim, "f16", [rr.add(0, h["adds"][0][1]), rr.range_(h["queries"], INF), rr.range_(h["queries"], 1e-9),
                                                 rr.range_(h["queries"], 4.0e9)]))
    want = check(pyqadc, twin, tmp_path, cases)
    k = rr.kept(want[0][0])
    assert k[[0, 2, 3, 4]].tolist() == [0] * 4 and k[1] == rows and k[5] == rows        # NaN, 0, -0, negative; +inf and FLT_MAX keep all
    if dtype == "f32":
        assert k[6] == 1 and rr.kept(want[0][1]).tolist() == [9] * 7 and rr.kept(want[0][2]).tolist() == [10] * 7   # the row AT the radius is out
    assert np.isfinite(want[1][0]["dist"]).all() and rr.kept(want[1][0])[1:].tolist() == [0, 0, 0]


@path_independent
@pytest.mark.parametrize("lo", [0, 1000, 2 ** 32 - 300])
def test_filters(pyqadc, twin, tmp_path, lo):
    """ALLOW and EXCLUDE with spans inside, across and outside the key range, an empty ALLOW set and an EXCLUDE of everything; keys
    up to 2^32 - 1"""
    rng = np.random.default_rng(lo % 1000 + 9)
    dim, rows = 65, 300
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(5, dim)).astype(F32)
    radius = quantile_radii(rng, vec, q, 0.3, 0.9)
    keys = np.arange(lo, lo + rows, dtype=np.int64)
    inside = rng.choice(keys, rows // 3, replace=False)
    across = np.concatenate([np.arange(max(0, lo - 5), lo + 7), np.arange(lo + rows - 7, min(2 ** 32, lo + rows + 5))])
    outside = np.array([k for k in (lo - 40, lo - 1, lo + rows, lo + rows + 33) if 0 <= k < 2 ** 32], np.int64)
    word = np.arange(lo + 32 - lo % 32, lo + 64 - lo % 32)
    ops = [rr.range_(q, radius, (mode, s)) for mode in ("exclude", "allow")
           for s in (inside, across, outside, keys[[0, -1]], word, np.zeros(0, np.uint32), keys)]
    (want,) = check(pyqadc, twin, tmp_path, [rr.dense_case(dim, "f16", lo, vec, ops)])
    assert int(want[12]["lims"][-1]) == 0 and int(want[6]["lims"][-1]) == 0 and int(want[13]["lims"][-1]) == int(want[5]["lims"][-1]) > 0
    assert np.isin(want[7]["keys"], inside).all() and not np.isin(want[0]["keys"], inside).any()


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_range_under_an_infinite_radius_is_knn_of_all_rows(pyqadc, dtype):
    """against code this change does not touch: on finite data Refine.range(+inf) equals Refine.knn(R = rows)"""
    rng = np.random.default_rng(24)
    dim, rows, lo, nq = 128, 1024, 1000, 5
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(nq, dim)).astype(F32)
    c = rr.dense_case(dim, dtype, lo, vec, [])
    st = rr.make_store(pyqadc, c)
    st.add(vec, lo)
    f = pyqadc.AdcFilter(np.arange(lo, lo + rows, 3), "exclude")
    for flt, n in ((None, rows), (f, rows - len(range(0, rows, 3)))):
        lims, keys, dist = st.range(q, INF, filter=flt)
        kk, kd, ks = st.knn(q, rows, filter=flt)
        assert lims.tolist() == [n * i for i in range(nq + 1)] and ks.tolist() == [n] * nq
        assert np.array_equal(keys.reshape(nq, n), kk[:, :n]) and np.array_equal(dist.view(np.uint32).reshape(nq, n), kd[:, :n].view(np.uint32))
    f.close()
    st.close()


@path_independent
def test_no_plan_shows_in_the_result(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(23)
    dim, rows, nq = 65, 3000, 33
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(nq, dim)).astype(F32)
    radius = quantile_radii(rng, vec, q, 0.0, 0.5)
    c = rr.dense_case(dim, "f32", 5, vec, [rr.range_(q, radius)])
    (want,) = rr.run_twin(twin, tmp_path, [c])
    for plan in ((0, 0, 0), (7, 100, 1), (64, 1000, 32), (100000, 1 << 24, 5), (1, 64, 33)):
        for device in (False, True):
            rr.assert_same(rr.run_store(pyqadc, c, plan=plan, device=device), want, "plan %s" % (plan,))


@path_independent
def test_the_held_result(pyqadc, twin, tmp_path):
    """collect twice; a short capacity is QADC_E_CAPACITY and the result stays; QADC_E_STATE before any range call; a refused call
    drops the result; add, knn and rerank in between leave it as it is"""
    import torch
    rng = np.random.default_rng(25)
    dim, rows = 8, 500
    vec = rng.normal(size=(rows, dim)).astype(F32)
    q = rng.normal(size=(3, dim)).astype(F32)
    st = pyqadc.Refine(dim, "f32")
    rc_, _, _ = st.range_collect_raw(10)
    assert rc_ == pyqadc.QADC_E_STATE
    st.add(vec[:400], 0)
    lims, keys, dist = st.range(q, 6.0)
    n = int(lims[-1])
    assert n > 7
    for _ in range(2):
        k2, d2 = st.range_collect(lims)
        assert np.array_equal(k2, keys) and np.array_equal(d2.view(np.uint32), dist.view(np.uint32))
    rc_, k3, _ = st.range_collect_raw(n - 1)
    assert rc_ == pyqadc.QADC_E_CAPACITY and not k3.any(), "a short capacity copies nothing"
    st.add(vec[400:])                                                     # calls in between leave the held result as it is
    st.knn(q, 10)
    st.rerank(q, np.tile(np.arange(20, dtype=np.uint32), (3, 1)), 5)
    st.get(np.arange(4))
    k4, d4 = st.range_collect(lims)
    assert np.array_equal(k4, keys) and np.array_equal(d4.view(np.uint32), dist.view(np.uint32))
    dk, dd = st._range_collect_device(lims)
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), keys) and np.array_equal(dd.cpu().numpy().view(np.uint32), dist.view(np.uint32))
    assert pyqadc.lib().qadc_refine_range(st._h, 3, None, None, None, None) == pyqadc.QADC_E_ARG     # a refused call drops the result
    assert st.range_collect_raw(n)[0] == pyqadc.QADC_E_STATE
    lims, keys, dist = st.range_device(torch.from_numpy(q).cuda(), 6.0)    # now over all 500 rows
    (want,) = rr.run_twin(twin, tmp_path, [rr.dense_case(dim, "f32", 0, vec, [rr.range_(q, 6.0)])])
    assert rr.same(dict(lims=lims, keys=keys.cpu().numpy().view(np.uint32), dist=dist.cpu().numpy(), missing=0), want[0]) is None
    st.close()


@path_independent
def test_corner_cases_and_refusals(pyqadc):
    import torch
    E = "qadc error %d:" % pyqadc.QADC_E_ARG
    q = np.zeros((3, 8), F32)
    L = pyqadc.lib()
    for keyed in (False, True):
        st = pyqadc.Refine(8, "f32", keyed=keyed)
        lims, keys, dist = st.range(q, INF)                               # an empty store: all-zero lims
        assert lims.tolist() == [0, 0, 0, 0] and len(keys) == 0 and st.range_collect_raw(0)[0] == 0
        lims, keys, dist = st.range(np.zeros((0, 8), F32), INF)           # nq = 0: an empty result is held
        assert lims.tolist() == [0] and st.range_collect_raw(0)[0] == 0
        if keyed:
            st.put(np.ones((5, 8), F32), np.arange(5))
            st.remove(np.arange(5))                                       # allocated rows, none live
            assert st.range(q, INF)[0].tolist() == [0, 0, 0, 0]
        with pytest.raises(pyqadc.QadcError, match=E):
            st.set_range_plan(0, (1 << 24) + 1, 0)
        with pytest.raises(pyqadc.QadcError, match=E):
            st.set_range_plan(0, 0, -1)
        r = np.ones(3, F32)
        lims = np.zeros(4, np.uint64)
        fp, up = lambda a: a.ctypes.data_as(pyqadc.f32p), lambda a: a.ctypes.data_as(pyqadc.u64p)
        assert L.qadc_refine_range(st._h, -1, fp(q), fp(r), None, up(lims)) == pyqadc.QADC_E_ARG
        assert L.qadc_refine_range(st._h, 3, None, fp(r), None, up(lims)) == pyqadc.QADC_E_ARG
        assert L.qadc_refine_range(st._h, 3, fp(q), None, None, up(lims)) == pyqadc.QADC_E_ARG
        assert L.qadc_refine_range(st._h, 3, fp(q), fp(r), None, None) == pyqadc.QADC_E_ARG
        dq = torch.zeros(3 * 8 + 1, dtype=torch.float32, device="cuda")
        assert L.qadc_refine_range_device(st._h, 3, dq.data_ptr() + 2, fp(r), None, up(lims)) == pyqadc.QADC_E_ARG   # 4-byte alignment
        assert L.qadc_refine_range_device(st._h, 3, dq.data_ptr() + 4, fp(r), None, up(lims)) == 0
        st.close()
    assert L.qadc_refine_range(None, 3, None, None, None, None) == pyqadc.QADC_E_ARG
    assert L.qadc_refine_set_range_plan(None, 0, 0, 0) == pyqadc.QADC_E_ARG and L.qadc_refine_range_reruns(None) == 0
    assert L.qadc_refine_range_collect(None, 0, None, None) == pyqadc.QADC_E_ARG
