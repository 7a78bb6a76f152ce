"""GPU: qadc_refine_knn_device through pyqadc.Refine.knn_device: torch tensors in, torch tensors out, equal
to the host form bit for bit on dense and keyed stores of floats and halves; a refused call leaves its outputs untouched."""
import numpy as np
import pytest

import refine_knn_cases as kc
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def filled(pyqadc, rng, dim, dtype, keyed, rows):
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    labels = rng.permutation(4 * rows)[:rows].astype(np.uint32) + 16 if keyed else np.arange(rows, dtype=np.uint32) + 16
    st = pyqadc.Refine(dim, dtype, keyed=keyed)
    if keyed:
        st.put(vec, labels)
        st.remove(labels[::5])
    else:
        st.add(vec, 16)
    return st, labels


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_device_form_equals_the_host_form(pyqadc, dtype, keyed):
    rng = np.random.default_rng(81)
    dim, rows, nq = 96, 9000, 37
    st, labels = filled(pyqadc, rng, dim, dtype, keyed, rows)
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    dq = torch.from_numpy(q).cuda()
    f = pyqadc.AdcFilter(labels[1::3], "exclude")
    for R, flt in ((1, None), (50, None), (1024, None), (50, f)):
        hk, hd, hs = st.knn(q, R, filter=flt)
        dk, dd, ds = st.knn_device(dq, R, filter=flt)
        assert dk.is_cuda and dk.dtype == torch.int32 and tuple(dk.shape) == (nq, R) and dd.dtype == torch.float32 and tuple(ds.shape) == (nq,)
        got = dict(keys=dk.cpu().numpy().view(np.uint32), dist=dd.cpu().numpy(), sizes=ds.cpu().numpy())
        assert kc.same(got, dict(keys=hk, dist=hd, sizes=hs)) is None, (R, flt is not None)
        assert (hs == R).all()
    f.close()
    st.close()


@path_independent
def test_a_refused_call_leaves_its_outputs_untouched(pyqadc):
    rng = np.random.default_rng(82)
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    dim, nq = 8, 3
    st, _ = filled(pyqadc, rng, dim, "f32", False, 100)
    q = torch.from_numpy(rng.normal(size=(nq, dim)).astype(np.float32)).cuda()
    R = kc.MAX_R + 1
    ok = torch.full((nq, R), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    od = torch.full((nq, R), 7.5, dtype=torch.float32, device="cuda")
    osz = torch.full((nq,), -3, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((ok == 0x5A5A5A5A).all()) and bool((od == 7.5).all()) and bool((osz == -3).all())

    with pytest.raises(pyqadc.QadcError, match="qadc error %d:" % E):
        st.knn_device(q, R, out=(ok, od, osz))                                                 # R above QADC_REFINE_KNN_MAX_R
    assert untouched()
    p = (q.data_ptr(), ok.data_ptr(), od.data_ptr(), osz.data_ptr())
    assert L.qadc_refine_knn_device(st._h, nq, p[0], 0, None, p[1], p[2], p[3]) == E          # R = 0
    assert L.qadc_refine_knn_device(None, nq, p[0], 4, None, p[1], p[2], p[3]) == E           # no store
    assert L.qadc_refine_knn_device(st._h, -1, p[0], 4, None, p[1], p[2], p[3]) == E
    for bad in range(4):                                                                       # a required array NULL; two bytes off its 4
        null = [None if i == bad else v for i, v in enumerate(p)]
        assert L.qadc_refine_knn_device(st._h, nq, null[0], 4, None, null[1], null[2], null[3]) == E, bad
        off = [v + (2 if i == bad else 0) for i, v in enumerate(p)]
        assert L.qadc_refine_knn_device(st._h, nq, off[0], 4, None, off[1], off[2], off[3]) == E, bad
        assert b"must be 4-byte aligned" in L.qadc_last_error()
    assert untouched()
    assert L.qadc_refine_knn_device(st._h, 0, None, 4, None, None, None, None) == 0            # nq = 0: a no-op
    assert untouched()
    assert L.qadc_refine_knn_device(st._h, nq, p[0], 4, None, p[1], p[2], p[3]) == 0
    torch.cuda.synchronize()
    assert osz.tolist() == [4, 4, 4] and bool((ok.view(-1)[:nq * 4] != 0x5A5A5A5A).all()) and bool((ok.view(-1)[nq * 4:] == 0x5A5A5A5A).all())
    st.close()
