"""GPU: the memory behaviour of the device entry points that came with SQ8 rows (DESIGN.md sections 6.1 and 11.20), on guard-band
arenas (tests/guard_arena.py), in the manner of test_gpu_guard_refine.py: qadc_refine_get_device, qadc_refine_sq_range_device, and
qadc_refine_rerank_device / _knn_device on an SQ8 store through raw ctypes calls.

W  every byte outside the declared outputs is unchanged (sq_range_device writes no device buffer at all: its outputs are host memory);
R  the results under the two guard poisons are bit-identical and equal the host form on the same data;
F  every output element is written: the NaN rows of keys not held are asserted under the 0x5A poison as well;
A  every buffer at 4 bytes and nothing coarser, and at 256 (found_out, bytes, at 1 as well).

The rows of a store are the library's own allocation, so no arena can end where they end; the SQ8 stores here are reserved to exactly
rows x dim bytes with rows x dim no multiple of 4 (dim 1, 63, 65), so that a load wider than the last row's bytes would leave the
allocation."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
import refine_sq_cases as sq
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = [4, 256]
F32 = np.float32
NO_KEY = 0xFFFFFFFF
ODD = [(1, 301), (63, 299), (65, 301)]                                               # rows x dim is no multiple of 4


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def sq_store(pyqadc, rng, dim, rows, keyed):
    v, vmin, step = sq.data_params(rng, rows, dim)
    labels = (rng.permutation(4 * rows)[:rows].astype(np.uint32) + 16) if keyed else np.arange(rows, dtype=np.uint32) + 16
    st = pyqadc.Refine(dim, "sq8", keyed=keyed, vmin=vmin, step=step)
    st.reserve(rows)
    st.put(v, labels) if keyed else st.add(v, 16)
    assert st.relocations() == 0
    return st, labels


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("found_align", [1, 4])
@pytest.mark.parametrize("dtype,keyed", [("sq8", False), ("sq8", True), ("f16", False), ("f32", True)])
def test_get_device(pyqadc, dtype, keyed, found_align, align):
    rng = np.random.default_rng(5 + keyed)
    dim, rows = 65, 301
    if dtype == "sq8":
        st, labels = sq_store(pyqadc, rng, dim, rows, keyed)
    else:
        labels = np.arange(rows, dtype=np.uint32) + 16
        st = pyqadc.Refine(dim, dtype, keyed=keyed)
        v = rng.normal(size=(rows, dim)).astype(F32)
        st.put(v, labels) if keyed else st.add(v, 16)
    keys = labels[rng.integers(0, rows, 130)]
    keys[:3] = (3, NO_KEY, labels[0])
    held = labels[~(labels[:, None].view(np.uint8) == 0xFF).any(1)]

    def call(a):
        k = a.place(keys, align, "in", guard=held, name="d_keys")
        out = a.place(np.empty((len(keys), dim), F32), align, "out", name="d_out_vectors")
        found = a.place(np.empty(len(keys), np.uint8), found_align, "out", name="d_found_out")
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_get_device(st._h, a.ptr(k), len(keys), a.ptr(out), a.ptr(found))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([out, found])
        return dict(rows=a.host(out), found=a.host(found))

    got = ga.under_both_poisons(call, backend="torch", capacity=1 << 20)
    rows_h, found_h = st.get(keys)
    assert ga.same(got, dict(rows=rows_h, found=found_h.astype(np.uint8))) is None
    assert list(got["found"][:3]) == [0, 0, 1] and (got["rows"][:2].view(np.uint32) == 0x7FC00000).all()

    def no_found(a):                                                                  # found_out NULL: the rows alone
        k = a.place(keys, align, "in", guard=held, name="d_keys")
        out = a.place(np.empty((len(keys), dim), F32), align, "out", name="d_out_vectors")
        a.snapshot()
        assert pyqadc.lib().qadc_refine_get_device(st._h, a.ptr(k), len(keys), a.ptr(out), None) == 0
        a.check_untouched([out])
        return dict(rows=a.host(out))

    assert ga.same(ga.under_both_poisons(no_found, backend="torch", capacity=1 << 20), dict(rows=rows_h)) is None
    st.close()


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("dim,n", [(1, 67), (65, 1000), (4096, 67), (63, 0)])
def test_sq_range_device(pyqadc, dim, n, align):
    """the learning set ends at a guard band, at a row count that is no multiple of the kernel's tile of 64 rows"""
    rng = np.random.default_rng(dim)
    v = rng.normal(size=(n, dim)).astype(F32)
    if n:
        v[rng.integers(0, n, 5), rng.integers(0, dim, 5)] = np.nan
    f32p = C.POINTER(C.c_float)

    def call(a):
        d = a.place(v if n else np.zeros((1, dim), F32), align, "in", name="d_vectors")
        vmin, step = np.full(dim, 7, F32), np.full(dim, 7, F32)
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_sq_range_device(a.ptr(d), n, dim, 0, vmin.ctypes.data_as(f32p), step.ctypes.data_as(f32p))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([])
        return dict(vmin=vmin, step=step)

    got = ga.under_both_poisons(call, backend="torch", capacity=4 << 20)
    a, b = pyqadc.refine_sq_range(v)
    assert ga.same(got, dict(vmin=a, step=b)) is None
    wa, wb = sq.np_range(v, dim)
    assert ga.same(got, dict(vmin=wa, step=wb)) is None


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dim,rows", ODD, ids=["dim%d" % d for d, _ in ODD])
def test_rerank_device_and_knn_device_on_an_sq8_store(pyqadc, dim, rows, keyed, align):
    rng = np.random.default_rng(dim + keyed)
    st, labels = sq_store(pyqadc, rng, dim, rows, keyed)
    st.set_knn_plan(64, 2)
    nq, r_in, R = 3, 65, 70
    queries = rng.normal(size=(nq, dim)).astype(F32)
    keys = labels[rng.integers(0, rows, (nq, r_in))]
    keys[0, :4] = (3, NO_KEY, labels[rows - 1], labels[rows - 1])                     # the last row, twice
    held = labels[~(labels[:, None].view(np.uint8) == 0xFF).any(1)]

    def rerank(a):
        q = a.place(queries, align, "in", name="d_queries")
        k = a.place(keys, align, "in", guard=held, name="d_keys")
        ok = a.place(np.empty((nq, R), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, R), F32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        missing = C.c_uint64(77)
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_rerank_device(st._h, nq, a.ptr(q), r_in, a.ptr(k), None, None, R, a.ptr(ok), a.ptr(od), a.ptr(osz),
                                                    C.byref(missing))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz])
        return dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz), missing=np.int64(missing.value))

    got = ga.under_both_poisons(rerank, backend="torch", capacity=2 << 20)
    hk, hd, hs, hm = st.rerank(queries, keys, R)
    assert ga.same(got, dict(keys=hk, dist=hd, sizes=hs, missing=np.int64(hm))) is None
    assert hm == 2 and (hs < R).all()

    Rk = 20

    def knn(a):
        q = a.place(queries, align, "in", name="d_queries")
        ok = a.place(np.empty((nq, Rk), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, Rk), F32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_knn_device(st._h, nq, a.ptr(q), Rk, None, a.ptr(ok), a.ptr(od), a.ptr(osz))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz])
        return dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz))

    got = ga.under_both_poisons(knn, backend="torch", capacity=2 << 20)
    hk, hd, hs = st.knn(queries, Rk)
    assert ga.same(got, dict(keys=hk, dist=hd, sizes=hs)) is None and (hs == Rk).all()
    st.close()
