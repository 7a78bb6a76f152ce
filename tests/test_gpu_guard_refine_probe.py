"""GPU: the memory behaviour of qadc_refine_knn_probed_device, qadc_adc_index_assign_device and qadc_adc_search_exact_device at the
C-ABI (DESIGN.md sections 6.1 and 11.22) on guard-band arenas (tests/guard_arena.py), through raw ctypes calls, on stores of floats,
halves and bytes, dense and keyed.  The rules are those of tests/test_gpu_guard_refine_knn.py:

W  every byte outside the declared outputs is unchanged (the probe lists a call only reads among them);
R  the results under the two guard poisons are bit-identical and equal the host form on the same data;
F  every [nq][R] slot, every d_out_sizes[q] and every d_assign_out[q][j] is written: the 0xFFFFFFFF / +inf fillers behind
   out_sizes[q] are asserted under the 0x5A output poison as well as the 0xFF one (which is itself the filler key);
A  every buffer at 4 bytes and nothing coarser, and at 256."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
import refine_probe_cases as pc
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = [4, 256]
STORES = [("f32", False), ("f16", True), ("sq8", False)]
STORE_IDS = ["%s-%s" % (d, "keyed" if k else "dense") for d, k in STORES]
NO_KEY = 0xFFFFFFFF
K = len(pc.SIZES)
N = sum(pc.SIZES)
SHAPES = [(3, 65, 2, 305), (33, 16, K, 7), (2, 4096, 1, 1024)]                                # (nq, dim, ma, R)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def setup(pyqadc, rng, dim, dtype, keyed):
    vec = rng.normal(size=(N, dim)).astype(np.float32)
    keys = np.arange(16, 16 + N, dtype=np.uint32)
    kw = dict(zip(("vmin", "step"), pc.sq_params(vec))) if dtype == "sq8" else {}
    st = pyqadc.Refine(dim, dtype, keyed=keyed, **kw)
    if keyed:
        st.put(vec, keys)
        st.remove(keys[::7])                                                 # free rows between live ones: missing entries
    else:
        st.add(vec, 16)
    labels = rng.permutation(keys)
    labels[::50] = labels[1::50]                                             # keys reached through two rows
    idx = pc.make_index(pyqadc, pc.split_labels(labels))
    return st, idx


def fillers_hold(got, nq, R):
    for qi in range(nq):                                                     # F, under this poison: the fillers behind out_sizes[q]
        size = int(got["sizes"][qi])
        assert 0 <= size <= R and (got["keys"][qi, size:] == NO_KEY).all() and np.isposinf(got["dist"][qi, size:]).all()
        assert (got["keys"][qi, :size] != NO_KEY).all() and (got["keys"][qi, :size] != 0x5A5A5A5A).all()
        assert np.isfinite(got["dist"][qi, :size]).all()


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("nq,dim,ma,R", SHAPES, ids=["nq%d-dim%d-ma%d-R%d" % k for k in SHAPES])
@pytest.mark.parametrize("dtype,keyed", STORES, ids=STORE_IDS)
def test_knn_probed_device(pyqadc, dtype, keyed, nq, dim, ma, R, align):
    rng = np.random.default_rng(nq + 7 * keyed)
    st, idx = setup(pyqadc, rng, dim, dtype, keyed)
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    assign = pc.probes(rng, nq, ma, K)
    assign[0, 0] = 4
    if ma > 1:
        assign[nq - 1, 0] = K + 3                                            # the device form skips it

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        da = a.place(assign, align, "in", name="d_assign")
        ok = a.place(np.empty((nq, R), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, R), np.float32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        a.snapshot()
        missing = C.c_uint64(0)
        rc = pyqadc.lib().qadc_refine_knn_probed_device(st._h, idx._h, nq, a.ptr(q), ma, a.ptr(da), R, None, a.ptr(ok), a.ptr(od), a.ptr(osz),
                                                        C.byref(missing))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz])
        got = dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz), missing=int(missing.value))
        fillers_hold(got, nq, R)
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    valid = np.where((assign >= 0) & (assign < K), assign, assign[:, -1:])   # (a repeat of a valid probe counts once)
    hk, hd, hs, hm = st.knn_probed(idx, queries, valid, R)
    assert pc.same(got, dict(keys=hk, dist=hd, sizes=hs, missing=hm)) is None, "differs from the host form"
    assert (got["missing"] > 0) == keyed and got["sizes"][0] == min(R, len(np.unique(hk[0][hk[0] != NO_KEY]))) > 0
    idx.close()
    st.close()


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("with_assign", [True, False], ids=["assign-out", "no-assign-out"])
def test_assign_device_and_search_exact_device(pyqadc, with_assign, align):
    rng = np.random.default_rng(11)
    nq, dim, ma, R = 33, 16, 3, 20
    st, idx = setup(pyqadc, rng, dim, "f32", False)
    idx.set_pq(rng.normal(size=(8, 256, dim // 8)).astype(np.float32))
    idx.set_coarse(rng.normal(size=(K, dim)).astype(np.float32))
    queries = rng.normal(size=(nq, dim)).astype(np.float32)

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        ok = a.place(np.empty((nq, R), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, R), np.float32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        da = a.place(np.empty((nq, ma), np.int32), align, "out", name="d_assign_out")
        db = a.place(np.empty((nq, ma), np.int32), align, "out", name="d_assign_out of assign_device")
        a.snapshot()
        missing = C.c_uint64(0)
        rc = pyqadc.lib().qadc_adc_search_exact_device(idx._h, st._h, nq, a.ptr(q), ma, R, 1, None, a.ptr(ok), a.ptr(od), a.ptr(osz),
                                                       C.byref(missing), a.ptr(da) if with_assign else None)
        assert rc == 0, pyqadc.lib().qadc_last_error()
        rc = pyqadc.lib().qadc_adc_index_assign_device(idx._h, nq, a.ptr(q), ma, 1, a.ptr(db))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz, db] + ([da] if with_assign else []))
        got = dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz), missing=int(missing.value), assign=a.host(db))
        fillers_hold(got, nq, R)
        assert not with_assign or np.array_equal(a.host(da), got["assign"])
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    hk, hd, hs, hm, ha = idx.search_exact(queries, ma, R, st)
    assert pc.same(got, dict(keys=hk, dist=hd, sizes=hs, missing=hm)) is None and np.array_equal(got["assign"], ha)
    assert ((ha >= 0) & (ha < K)).all() and (got["sizes"] > 0).any()
    idx.close()
    st.close()
