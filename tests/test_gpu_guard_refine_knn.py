"""GPU: the memory behaviour of qadc_refine_knn_device at the C-ABI (DESIGN.md sections 6.1 and 11.16) on guard-band arenas
(tests/guard_arena.py), through raw ctypes calls, on stores of floats and halves, dense and keyed, with and without a filter.  The
rules are those of tests/test_gpu_guard_refine.py:

W  every byte outside the declared outputs is unchanged;
R  the results under the two guard poisons are bit-identical and equal the host form on the same data;
F  every [nq][R] slot and every d_out_sizes[q] is written: the 0xFFFFFFFF / +inf fillers behind out_sizes[q] are asserted under the
   0x5A output poison as well as the 0xFF one (which is itself the filler key);
A  every buffer at 4 bytes and nothing coarser, and at 256."""
import numpy as np
import pytest

import guard_arena as ga
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = [4, 256]
STORES = [(d, k) for d in ("f32", "f16") for k in (False, True)]
STORE_IDS = ["%s-%s" % (d, "keyed" if k else "dense") for d, k in STORES]
NO_KEY = 0xFFFFFFFF
KNN = [(3, 65, 300, 305), (33, 1, 9000, 7), (2, 4096, 100, 1024)]                           # (nq, dim, rows, R)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])
@pytest.mark.parametrize("nq,dim,rows,R", KNN, ids=["nq%d-dim%d-rows%d-R%d" % k for k in KNN])
@pytest.mark.parametrize("dtype,keyed", STORES, ids=STORE_IDS)
def test_knn_device(pyqadc, dtype, keyed, nq, dim, rows, R, filtered, align):
    rng = np.random.default_rng(nq + 7 * keyed)
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    labels = (rng.permutation(4 * rows)[:rows].astype(np.uint32) + 16) if keyed else np.arange(rows, dtype=np.uint32) + 16
    st = pyqadc.Refine(dim, dtype, keyed=keyed)
    if keyed:
        st.put(vec, labels)
        st.remove(labels[::7])                                               # free rows between live ones
    else:
        st.add(vec, 16)
    held = rows - len(labels[::7]) if keyed else rows
    f = pyqadc.AdcFilter(labels[1::2], "allow") if filtered else None
    queries = rng.normal(size=(nq, dim)).astype(np.float32)

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        ok = a.place(np.empty((nq, R), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, R), np.float32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_knn_device(st._h, nq, a.ptr(q), R, None if f is None else f._h, a.ptr(ok), a.ptr(od), a.ptr(osz))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz])
        got = dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz))
        for qi in range(nq):                                                 # F, under this poison: the fillers behind out_sizes[q]
            size = int(got["sizes"][qi])
            assert 0 <= size <= min(R, held) and (got["keys"][qi, size:] == NO_KEY).all() and np.isposinf(got["dist"][qi, size:]).all()
            assert (got["keys"][qi, :size] != NO_KEY).all() and (got["keys"][qi, :size] != 0x5A5A5A5A).all()
            assert np.isfinite(got["dist"][qi, :size]).all()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    hk, hd, hs = st.knn(queries, R, filter=f)
    host = dict(keys=hk, dist=hd, sizes=hs)
    assert ga.same(got, host) is None, "%s differs from the host form" % ga.same(got, host)
    wk, wd, ws = st.knn_device(torch.from_numpy(queries).cuda(), R, filter=f)
    wrapper = dict(keys=wk.cpu().numpy().view(np.uint32), dist=wd.cpu().numpy(), sizes=ws.cpu().numpy())
    assert ga.same(got, wrapper) is None, "%s differs from the wrapper's call" % ga.same(got, wrapper)
    if not filtered:
        assert (host["sizes"] == min(R, held)).all()
    else:
        assert 0 < host["sizes"][0] <= min(R, held)
    if f is not None:
        f.close()
    st.close()
