"""GPU: range results re-ranked by exact L2 (pyqadc.Refine.rerank_range over qadc_refine_rerank_range)
against the host twin (refine::rerank_range through tests/cpp/refine_range_host.cpp): lims, keys, the distances' bit patterns and
the missing count, for equality.  Segments that are empty, of one candidate and of more than 8192; keys listed several times, in the
LDS form and in the radix form of the sort; missing keys and key 0xFFFFFFFF; every element type; and, against code this change does
not touch, rerank_range under radius +inf cut at R equals rerank."""
import numpy as np
import pytest

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


def check(pyqadc, twin, tmp_path, cases, **how):
    wants = rr.run_twin(twin, tmp_path, cases)
    for i, (c, want) in enumerate(zip(cases, wants)):
        rr.assert_same(rr.run_store(pyqadc, c, **how), want, "case %d" % i)
    return wants


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 128, 257, 4096])
def test_dims_and_segments(pyqadc, twin, tmp_path, dim, dtype):
    """segments of 0, 1, 3, 4, 5, 63, 64, 65 and 300 candidates (a workgroup's chunk is 4 to 64 of them), with keys outside the store
    and keys listed twice"""
    rng = np.random.default_rng(dim + 10 * rr.DTYPES[dtype])
    rows, lo = (300, 1000) if dim < 4096 else (60, 1000)
    vec = rng.normal(size=(rows, dim)).astype(F32)
    sizes = [0, 1, 3, 4, 5, 63, 64, 65, 300, 0]
    q = rng.normal(size=(len(sizes), dim)).astype(F32)
    segs = [rng.integers(lo - 3, lo + rows + 3, n) for n in sizes]
    segs[8][:20] = segs[8][20:40]
    d = ((vec[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(-1)
    part = np.quantile(d, 0.5, axis=1).astype(F32)
    c = rr.dense_case(dim, dtype, lo, vec, [rr.rerank_range(q, segs, INF), rr.rerank_range(q, segs, part), rr.rerank_range(q[:1], segs[:1], INF),
                                            rr.rerank_range(q, segs, np.nan)])
    (want,) = check(pyqadc, twin, tmp_path, [c])
    check(pyqadc, twin, tmp_path, [c], device=True, plan=(0, 0, 3))
    assert want[0]["missing"] > 0 and 0 < int(want[1]["lims"][-1]) < int(want[0]["lims"][-1]) < sum(sizes) and int(want[3]["lims"][-1]) == 0


@path_independent
def test_long_segments_duplicates_missing_keys_and_the_filler_key(pyqadc, twin, tmp_path):
    """a segment of more than 8192 candidates (more than rerank takes), duplicates in the radix form (a segment above 4096), a segment
    of exactly 4096 and one of 4097, missing keys counted, key 0xFFFFFFFF outside the store"""
    rng = np.random.default_rng(7)
    dim, rows, lo = 3, 9000, 1000
    vec = rng.normal(size=(rows, dim)).astype(F32)
    keys = np.arange(lo, lo + rows, dtype=np.int64)
    segs = [np.concatenate([keys, keys[:500]]),                                           # 9500 > 8192, 500 keys twice
            np.concatenate([rng.choice(keys, 3000), rng.choice(keys, 3000), [0xFFFFFFFF] * 5, [5, lo - 1]]),   # radix form, repeats, misses
            rng.choice(keys, rr.SORT_LDS, replace=False), rng.choice(keys, rr.SORT_LDS + 1, replace=False),
            [0xFFFFFFFF], np.full(5000, lo + 17), []]
    q = rng.normal(size=(len(segs), dim)).astype(F32)
    c = rr.dense_case(dim, "f32", lo, vec, [rr.rerank_range(q, segs, INF), rr.rerank_range(q, segs, 1.5)])
    (want,) = check(pyqadc, twin, tmp_path, [c])
    check(pyqadc, twin, tmp_path, [c], device=True, plan=(0, 0, 2))
    k = rr.kept(want[0])
    assert k[0] == rows and k[2] == rr.SORT_LDS and k[3] == rr.SORT_LDS + 1 and k[4] == 0 and k[5] == 1 and k[6] == 0
    assert want[0]["missing"] == 5 + 2 + 1 and k[1] == len(np.unique(segs[1])) - 3
    assert 0 < rr.kept(want[1])[0] < rows


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_rerank_range_under_an_infinite_radius_cut_at_R_is_rerank(pyqadc, dtype, keyed):
    """against code this change does not touch"""
    import torch
    rng = np.random.default_rng(30 + keyed)
    dim, rows, nq, r_in, R = 96, 2000, 6, 700, 100
    vec = rng.normal(size=(rows, dim)).astype(F32)
    labels = rng.choice(2 ** 32 - 1, rows, replace=False).astype(np.uint32) if keyed else np.arange(50, 50 + rows, dtype=np.uint32)
    c = rr.case(keyed, dim, dtype, [], *(rr.sq_params(vec) if dtype == "sq8" else (None, None)))
    st = rr.make_store(pyqadc, c)
    if keyed:
        st.put(vec, labels)
    else:
        st.add(vec, 50)
    q = rng.normal(size=(nq, dim)).astype(F32)
    cand = labels[rng.integers(0, rows, (nq, r_in))]
    cand[:, :7] = (3, 0xFFFFFFFF, 49, 50 + rows, 3, 3, 3) if not keyed else cand[:, 7:14]
    lims, keys, dist, missing = st.rerank_range(q, np.arange(nq + 1) * r_in, cand.reshape(-1), INF)
    rk, rd, rs, rmissing = st.rerank(q, cand, R)
    assert missing == rmissing and (np.diff(lims) >= R).all()
    for i in range(nq):
        assert np.array_equal(keys[lims[i]:lims[i] + R], rk[i]) and np.array_equal(dist[lims[i]:lims[i] + R].view(np.uint32), rd[i].view(np.uint32))
    dl, dk, dd, dm = st.rerank_range_device(torch.from_numpy(q).cuda(), np.arange(nq + 1) * r_in, torch.from_numpy(cand.reshape(-1).view(np.int32)).cuda(), INF)
    assert dm == missing and np.array_equal(dl, lims) and np.array_equal(dk.cpu().numpy().view(np.uint32), keys)
    assert np.array_equal(dd.cpu().numpy().view(np.uint32), dist.view(np.uint32))
    st.close()


@path_independent
def test_corner_cases_and_refusals(pyqadc):
    E = pyqadc.QADC_E_ARG
    L = pyqadc.lib()
    st = pyqadc.Refine(8, "f32")
    st.add(np.ones((10, 8), F32), 0)
    q = np.zeros((2, 8), F32)
    lims, keys, dist, missing = st.rerank_range(np.zeros((0, 8), F32), [0], [], INF)       # nq = 0: an empty result is held
    assert lims.tolist() == [0] and missing == 0 and st.range_collect_raw(0)[0] == 0
    lims, keys, dist, missing = st.rerank_range(q, [0, 0, 0], [], INF)                     # no candidates at all
    assert lims.tolist() == [0, 0, 0] and missing == 0
    lims, keys, dist, missing = st.rerank_range(q, [0, 3, 3], [1, 1, 12], 9.0)
    assert lims.tolist() == [0, 1, 1] and keys.tolist() == [1] and dist.tolist() == [8.0] and missing == 1
    fp, up, kp = (lambda a: a.ctypes.data_as(pyqadc.f32p)), (lambda a: a.ctypes.data_as(pyqadc.u64p)), (lambda a: a.ctypes.data_as(pyqadc.u32p))
    r, out, k = np.full(2, 9.0, F32), np.zeros(3, np.uint64), np.arange(4, dtype=np.uint32)
    good = np.array([0, 2, 4], np.uint64)
    assert L.qadc_refine_rerank_range(st._h, 2, fp(q), up(good), kp(k), fp(r), up(out), None) == 0 and out.tolist() == [0, 2, 4]
    for bad in ([1, 2, 4], [0, 3, 2]):                                                     # not from 0; decreasing
        assert L.qadc_refine_rerank_range(st._h, 2, fp(q), up(np.array(bad, np.uint64)), kp(k), fp(r), up(out), None) == E
        assert st.range_collect_raw(4)[0] == pyqadc.QADC_E_STATE, "a refused call drops the held result"
    assert L.qadc_refine_rerank_range(st._h, 2, fp(q), None, kp(k), fp(r), up(out), None) == E
    assert L.qadc_refine_rerank_range(st._h, 2, fp(q), up(good), None, fp(r), up(out), None) == E
    assert L.qadc_refine_rerank_range(st._h, 2, fp(q), up(good), kp(k), None, up(out), None) == E
    assert L.qadc_refine_rerank_range(st._h, 2, fp(q), up(good), kp(k), fp(r), None, None) == E
    assert L.qadc_refine_rerank_range(st._h, -1, fp(q), up(good), kp(k), fp(r), up(out), None) == E
    assert L.qadc_refine_rerank_range(None, 2, fp(q), up(good), kp(k), fp(r), up(out), None) == E
    import torch
    dq, dk = torch.zeros(17, dtype=torch.float32, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    assert L.qadc_refine_rerank_range_device(st._h, 2, dq.data_ptr() + 1, up(good), dk.data_ptr(), fp(r), up(out), None) == E
    assert L.qadc_refine_rerank_range_device(st._h, 2, dq.data_ptr(), up(good), dk.data_ptr() + 2, fp(r), up(out), None) == E
    assert L.qadc_refine_rerank_range_device(st._h, 2, dq.data_ptr() + 4, up(good), dk.data_ptr() + 4, fp(r), up(out), None) == 0
    st.close()
