"""GPU: the memory behaviour of the refine store's device entry points under the inner-product metric (DESIGN.md sections 6.1 and
11.23) on guard-band arenas (tests/guard_arena.py): qadc_refine_rerank_device, _knn_device, _knn_probed_device and
qadc_adc_search_exact_device on a store whose metric is QADC_REFINE_IP, through raw ctypes calls, on stores of floats, halves and
bytes, dense and keyed.  The rules are those of tests/test_gpu_guard_refine.py:

W  every byte outside the declared outputs is unchanged;
R  the results under the two guard poisons are bit-identical and equal the host form on the same data;
F  every [nq][R] slot and every d_out_sizes[q] is written: the 0xFFFFFFFF / -inf fillers behind out_sizes[q] are asserted under the
   0x5A output poison as well as the 0xFF one (which is itself the filler key);
A  every buffer at 4 bytes and nothing coarser, and at 256."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
import refine_ip_cases as ic
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = [4, 256]
STORES = [("f32", False), ("f16", True), ("sq8", False)]
STORE_IDS = ["%s-%s" % (d, "keyed" if k else "dense") for d, k in STORES]
NO_KEY = 0xFFFFFFFF
SIZES = (0, 1, 63, 300, 436)
K, N = len(SIZES), sum(SIZES)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def quiet(labels):
    """the labels none of whose bytes is 0xFF: what a P2 guard may cycle through"""
    labels = np.ascontiguousarray(labels, np.uint32)
    return labels[~(labels[:, None].view(np.uint8) == 0xFF).any(1)]


def setup(pyqadc, rng, dim, dtype, keyed):
    """a store of the keys 16 .. 16 + N under "ip" (keyed: every seventh key removed) and an index whose labels hold some keys twice"""
    vec = rng.normal(size=(N, dim)).astype(np.float32)
    keys = np.arange(16, 16 + N, dtype=np.uint32)
    st = ic.make_store(pyqadc, ic.case(dim, dtype, vec, [], lo=16, labels=keys if keyed else None), metric="ip")
    if keyed:
        st.remove(keys[::7])
    labels = rng.permutation(keys)
    labels[::50] = labels[1::50]
    return st, keys, ic.make_index(pyqadc, ic.split(labels, SIZES))


def fillers_hold(got, nq, R):
    for qi in range(nq):                                                     # F, under this poison: the fillers behind out_sizes[q]
        size = int(got["sizes"][qi])
        assert 0 <= size <= R and (got["keys"][qi, size:] == NO_KEY).all() and (got["dist"][qi, size:].view(np.uint32) == ic.NEG_INF_BITS).all()
        assert (got["keys"][qi, :size] != NO_KEY).all() and (got["keys"][qi, :size] != 0x5A5A5A5A).all()
        assert np.isfinite(got["dist"][qi, :size]).all() and (np.diff(got["dist"][qi, :size]) <= 0).all()


RERANK = [(65, 3, 65), (513, 1, 1)]                                          # (r_in, nq, dim)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "counts-values"])
@pytest.mark.parametrize("r_in,nq,dim", RERANK, ids=["rin%d-nq%d-dim%d" % r for r in RERANK])
@pytest.mark.parametrize("dtype,keyed", STORES, ids=STORE_IDS)
def test_rerank_device(pyqadc, dtype, keyed, r_in, nq, dim, extras, align):
    rng = np.random.default_rng(r_in + 7 * keyed)
    R = r_in + 5
    st, labels, idx = setup(pyqadc, rng, dim, dtype, keyed)
    idx.close()
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    keys = labels[rng.integers(0, N, (nq, r_in))]
    keys[0, :3] = (3, NO_KEY, labels[1])                                     # two missing keys; duplicates come with the draw
    counts = values = None
    if extras:
        counts = np.array([r_in, 10, 0][:nq], np.int32) if nq > 1 else np.array([r_in - 3], np.int32)
        values = rng.random((nq, r_in)).astype(np.float32)
        values[0, 5:9] = ic.FLT_MAX                                          # skipped
    held = quiet(labels[1::7])                                               # (held by the keyed store too)

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        k = a.place(keys, align, "in", guard=held, name="d_keys")
        c = a.place(counts, align, "in", guard=np.array([r_in], np.int32), name="d_counts") if extras else None
        v = a.place(values, align, "in", name="d_values") if extras else None
        ok = a.place(np.empty((nq, R), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, R), np.float32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        missing = C.c_uint64(77)
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_rerank_device(st._h, nq, a.ptr(q), r_in, a.ptr(k), a.ptr(c) if extras else None, a.ptr(v) if extras else None,
                                                    R, a.ptr(ok), a.ptr(od), a.ptr(osz), C.byref(missing))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz])
        got = dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz), missing=np.int64(missing.value))
        fillers_hold(got, nq, R)
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    hk, hd, hs, hm = st.rerank(queries, keys, R, counts=counts, values=values)
    host = dict(keys=hk, dist=hd, sizes=hs, missing=np.int64(hm))
    assert ga.same(got, host) is None, "%s differs from the host form" % ga.same(got, host)
    assert host["missing"] >= 2 and host["sizes"][0] > 1
    st.close()


KNN = [(3, 65, 305), (33, 16, 7), (2, 4096, 1024)]                           # (nq, dim, R)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("nq,dim,R", KNN, ids=["nq%d-dim%d-R%d" % k for k in KNN])
@pytest.mark.parametrize("dtype,keyed", STORES, ids=STORE_IDS)
def test_knn_device_and_knn_probed_device(pyqadc, dtype, keyed, nq, dim, R, align):
    rng = np.random.default_rng(nq + 7 * keyed)
    st, labels, idx = setup(pyqadc, rng, dim, dtype, keyed)
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    ma = 2
    assign = np.stack([rng.permutation(K)[:ma] for _ in range(nq)]).astype(np.int32)
    assign[0] = (4, 3)
    assign[nq - 1, 0] = K + 3                                                # the device form skips it

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        da = a.place(assign, align, "in", name="d_assign")
        outs = [a.place(np.empty((nq, R), t), align, "out", name=n) for t, n in ((np.uint32, "d_out_keys"), (np.float32, "d_out_dist"))]
        outs.append(a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes"))
        pouts = [a.place(np.empty((nq, R), t), align, "out", name=n + " (probed)") for t, n in ((np.uint32, "d_out_keys"), (np.float32, "d_out_dist"))]
        pouts.append(a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes (probed)"))
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_knn_device(st._h, nq, a.ptr(q), R, None, a.ptr(outs[0]), a.ptr(outs[1]), a.ptr(outs[2]))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched(outs)
        missing = C.c_uint64(0)
        rc = pyqadc.lib().qadc_refine_knn_probed_device(st._h, idx._h, nq, a.ptr(q), ma, a.ptr(da), R, None, a.ptr(pouts[0]), a.ptr(pouts[1]),
                                                        a.ptr(pouts[2]), C.byref(missing))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched(outs + pouts)
        got = dict(keys=a.host(outs[0]), dist=a.host(outs[1]), sizes=a.host(outs[2]), pkeys=a.host(pouts[0]), pdist=a.host(pouts[1]),
                   psizes=a.host(pouts[2]), missing=np.int64(missing.value))
        fillers_hold(got, nq, R)
        fillers_hold(dict(keys=got["pkeys"], dist=got["pdist"], sizes=got["psizes"]), nq, R)
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    hk, hd, hs = st.knn(queries, R)
    valid = np.where((assign >= 0) & (assign < K), assign, assign[:, -1:])   # (a repeat of a valid probe counts once)
    pk, pd, ps, pm = st.knn_probed(idx, queries, valid, R)
    host = dict(keys=hk, dist=hd, sizes=hs, pkeys=pk, pdist=pd, psizes=ps, missing=np.int64(pm))
    assert ga.same(got, host) is None, "%s differs from the host form" % ga.same(got, host)
    assert (got["missing"] > 0) == keyed and got["psizes"][0] > 0 and got["sizes"][0] == min(R, N - (len(labels[::7]) if keyed else 0))
    idx.close()
    st.close()


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
def test_search_exact_device(pyqadc, align):
    rng = np.random.default_rng(11)
    nq, dim, ma, R = 33, 16, 3, 20
    st, _, idx = setup(pyqadc, rng, dim, "f32", False)
    idx.set_pq(rng.normal(size=(8, 256, dim // 8)).astype(np.float32))
    idx.set_coarse(rng.normal(size=(K, dim)).astype(np.float32))
    queries = rng.normal(size=(nq, dim)).astype(np.float32)

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        ok = a.place(np.empty((nq, R), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, R), np.float32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        da = a.place(np.empty((nq, ma), np.int32), align, "out", name="d_assign_out")
        a.snapshot()
        missing = C.c_uint64(0)
        rc = pyqadc.lib().qadc_adc_search_exact_device(idx._h, st._h, nq, a.ptr(q), ma, R, 1, None, a.ptr(ok), a.ptr(od), a.ptr(osz),
                                                       C.byref(missing), a.ptr(da))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz, da])
        got = dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz), missing=np.int64(missing.value), assign=a.host(da))
        fillers_hold(got, nq, R)
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    hk, hd, hs, hm, ha = idx.search_exact(queries, ma, R, st)
    assert ga.same(got, dict(keys=hk, dist=hd, sizes=hs, missing=np.int64(hm), assign=ha)) is None
    assert (got["sizes"] > 0).any()
    idx.close()
    st.close()
