"""GPU: the metric as state of a refine store (qadc_refine_set_metric, qadc_refine_metric): L2 by default;
inner product and back to L2 gives what a store that was never told otherwise gives, on rerank, knn and knn_probed; under "ip" the
four range calls return QADC_E_STATE and leave a held result as it is; bad arguments; and search_refined* under "ip" is the search
followed by rerank under "ip" (which the twin confirms)."""
import ctypes as C

import numpy as np
import pytest

import refine_ip_cases as ic
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DIM, N, K = 16, 900, 4


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return ic.build_driver()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def data(rng):
    vec = rng.normal(size=(N, DIM)).astype(np.float32)
    q = rng.normal(size=(7, DIM)).astype(np.float32)
    parts = ic.split(rng.permutation(N).astype(np.uint32), (100, 0, 500, 300))
    return vec, q, parts


def answers(st, idx, q):
    """what a store answers to one rerank, one knn and one knn_probed"""
    keys = np.tile(np.arange(0, N + 10, 3, dtype=np.uint32), (len(q), 1))
    assign = np.tile(np.array([2, 0], np.int32), (len(q), 1))
    return [st.rerank(q, keys, 40), st.knn(q, 40) + (0,), st.knn_probed(idx, q, assign, 40)]


def equal(a, b):
    return all(ic.same(dict(zip(("keys", "dist", "sizes", "missing"), x)), dict(zip(("keys", "dist", "sizes", "missing"), y))) is None
               for x, y in zip(a, b))


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_l2_by_default_and_ip_then_back_to_l2_is_a_fresh_l2_store(pyqadc, dtype, keyed):
    rng = np.random.default_rng(1)
    vec, q, parts = data(rng)
    c = ic.case(DIM, dtype, vec, [], labels=np.arange(N, dtype=np.uint32) if keyed else None)
    fresh, st, idx = ic.make_store(pyqadc, c), ic.make_store(pyqadc, c), ic.make_index(pyqadc, parts)
    try:
        m = C.c_int(-1)
        assert pyqadc.lib().qadc_refine_metric(st._h, C.byref(m)) == 0 and m.value == 0 and st.metric == "l2"
        want = answers(fresh, idx, q)
        assert equal(answers(st, idx, q), want)
        st.set_metric("ip")
        assert st.metric == "ip" and fresh.metric == "l2"
        ip = answers(st, idx, q)
        assert not equal(ip, want) and (np.diff(ip[1][1][0]) <= 0).all() and (np.diff(want[1][1][0]) >= 0).all()
        assert ip[0][3] == want[0][3] > 0                                       # the missing count knows no metric
        st.set_metric("l2")
        assert st.metric == "l2" and equal(answers(st, idx, q), want)
        again = pyqadc.Refine.from_vectors(vec, dtype, metric="ip") if not keyed else None     # the constructors' metric=
        if again is not None:
            assert again.metric == "ip" and (dtype == "sq8" or equal(answers(again, idx, q), ip))
            again.close()
    finally:
        idx.close()
        st.close()
        fresh.close()


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_range_calls_are_refused_under_ip_and_a_held_result_stays(pyqadc, keyed):
    rng = np.random.default_rng(2)
    vec, q, _ = data(rng)
    c = ic.case(DIM, "f32", vec, [], labels=np.arange(N, dtype=np.uint32) if keyed else None)
    st = ic.make_store(pyqadc, c)
    L, E = pyqadc.lib(), pyqadc.QADC_E_STATE
    f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    try:
        lims, keys, dist = st.range(q, 20.0)
        assert lims[-1] > 50
        st.set_metric("ip")
        radius = np.full(len(q), 20.0, np.float32)
        cand = np.arange(N, dtype=np.uint32)
        in_lims = (np.arange(len(q) + 1) * 100).astype(np.uint64)
        out = np.full(len(q) + 1, 77, np.uint64)
        missing = C.c_uint64(77)
        dq, dk = dev(q), dev(cand)
        p = lambda a, t: a.ctypes.data_as(t)
        assert L.qadc_refine_range(st._h, len(q), p(q, f32p), p(radius, f32p), None, p(out, u64p)) == E
        assert b"L2 only" in L.qadc_last_error()
        assert L.qadc_refine_range_device(st._h, len(q), dq.data_ptr(), p(radius, f32p), None, p(out, u64p)) == E
        assert L.qadc_refine_rerank_range(st._h, len(q), p(q, f32p), p(in_lims, u64p), p(cand, u32p), p(radius, f32p), p(out, u64p), C.byref(missing)) == E
        assert L.qadc_refine_rerank_range_device(st._h, len(q), dq.data_ptr(), p(in_lims, u64p), dk.data_ptr(), p(radius, f32p), p(out, u64p),
                                                 C.byref(missing)) == E
        assert (out == 77).all() and missing.value == 77                       # no output was touched
        with pytest.raises(pyqadc.QadcError, match="qadc error %d:" % E):
            st.range(q, 20.0)
        k2, d2 = st.range_collect(lims)                                        # the result held from before: still there, unchanged
        assert np.array_equal(k2, keys) and np.array_equal(d2.view(np.uint32), dist.view(np.uint32))
        dk2, dd2 = st._range_collect_device(lims)
        assert np.array_equal(dk2.cpu().numpy().view(np.uint32), keys) and np.array_equal(dd2.cpu().numpy().view(np.uint32), dist.view(np.uint32))
        st.set_metric("l2")
        lims3, keys3, dist3 = st.range(q, 20.0)
        assert np.array_equal(lims3, lims) and np.array_equal(keys3, keys) and np.array_equal(dist3.view(np.uint32), dist.view(np.uint32))
    finally:
        st.close()


@path_independent
def test_bad_arguments(pyqadc):
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    st = pyqadc.Refine(8, "f32")
    try:
        m = C.c_int(5)
        assert L.qadc_refine_set_metric(None, 0) == E and L.qadc_refine_metric(None, C.byref(m)) == E and L.qadc_refine_metric(st._h, None) == E
        for bad in (-1, 2, 7):
            assert L.qadc_refine_set_metric(st._h, bad) == E
        assert st.metric == "l2" and m.value == 5
        st.set_metric("ip")
        assert L.qadc_refine_set_metric(st._h, 2) == E and st.metric == "ip"   # a refused call leaves the metric as it was
        with pytest.raises(ValueError):
            st.set_metric("cosine")
        with pytest.raises(ValueError):
            pyqadc.Refine(8, "f32", metric="dot")
    finally:
        st.close()


@path_independent
def test_search_refined_under_ip_is_search_then_rerank_under_ip(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(3)
    vec, q, parts = data(rng)
    st = pyqadc.Refine.from_vectors(vec, "f32", metric="ip")
    idx = ic.make_index(pyqadc, parts)
    idx.set_pq(rng.normal(size=(8, 256, DIM // 8)).astype(np.float32))
    idx.set_coarse(rng.normal(size=(K, DIM)).astype(np.float32))
    src = pyqadc.Index(16)
    src.add_partitions([rng.integers(0, 256, (len(p), 8), dtype=np.uint8) for p in parts], list(parts))
    src.set_pq(rng.normal(size=(16, 16, DIM // 16)).astype(np.float32))
    src.set_coarse(rng.normal(size=(K, DIM)).astype(np.float32))
    src.finalize(0.01)
    try:
        r_in, R, ma = 120, 30, 3
        keys, vals, _, _ = idx.search(q, ma, r_in)
        got = idx.search_refined(q, ma, R, r_in, st)
        c = ic.case(DIM, "f32", vec, [ic.rerank("ip", q, keys, R, values=vals)])
        (want,) = ic.run_twin(twin, tmp_path, [c])
        names = ("keys", "dist", "sizes", "missing")
        assert ic.same(dict(zip(names, got)), want[0]) is None and ic.same(dict(zip(names, st.rerank(q, keys, R, values=vals))), want[0]) is None
        assert (np.diff(got[1][0, :got[2][0]]) <= 0).all() and got[2].min() > 0
        dk, dd, ds, dm = idx.search_refined_device(dev(q), ma, R, r_in, st)
        assert ic.same(dict(keys=dk.cpu().numpy().view(np.uint32), dist=dd.cpu().numpy(), sizes=ds.cpu().numpy(), missing=dm), want[0]) is None
        found = src.search(q, ma, r_in)                                        # the 4-bit engine: counts in place of values
        got4 = src.search_refined(q, ma, R, r_in, st)
        c4 = ic.case(DIM, "f32", vec, [ic.rerank("ip", q, found["keys"], R, counts=found["sizes"])])
        (want4,) = ic.run_twin(twin, tmp_path, [c4])
        assert ic.same(dict(zip(names, got4)), want4[0]) is None
    finally:
        src.close()
        idx.close()
        st.close()
