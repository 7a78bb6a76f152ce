"""GPU: the memory behaviour of qadc_refine_range_device, qadc_refine_rerank_range_device and qadc_refine_range_collect_device at the
C-ABI (DESIGN.md sections 6.1 and 11.21) on guard-band arenas (tests/guard_arena.py), through raw ctypes calls: d_queries, d_keys
and both collect outputs sit in windows of exactly the sizes the header states.  The rules are those of
tests/test_gpu_guard_refine.py:

W  every byte outside the declared outputs is unchanged — the range calls write no caller buffer at all, collect writes lims[nq]
   entries of each output and nothing behind them;
R  the results under the two guard poisons are bit-identical and equal the host form on the same data;
A  every buffer at 4 bytes and nothing coarser, and at 256; a pointer below 4 bytes is refused and nothing is written."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = [4, 256]
STORES = [("f32", False), ("f16", True), ("sq8", False)]
STORE_IDS = ["%s-%s" % (d, "keyed" if k else "dense") for d, k in STORES]
SHAPES = [(3, 65, 300), (33, 1, 9000), (2, 4096, 100)]                                       # (nq, dim, rows)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def make(pyqadc, rng, dtype, keyed, dim, rows):
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    labels = (rng.permutation(4 * rows)[:rows].astype(np.uint32) + 16) if keyed else np.arange(rows, dtype=np.uint32) + 16
    if dtype == "sq8":
        vmin, step = pyqadc.refine_sq_range(vec)
        st = pyqadc.Refine(dim, "sq8", keyed=keyed, vmin=vmin, step=step)
    else:
        st = pyqadc.Refine(dim, dtype, keyed=keyed)
    if keyed:
        st.put(vec, labels)
        st.remove(labels[::7])
    else:
        st.add(vec, 16)
    return st, vec, labels


def collect_cases(pyqadc, st, a, rows, align, want):
    """capacity exact, 7 over and 1 short, from one held result, into fresh windows of the arena"""
    L = pyqadc.lib()
    for name, cap in (("exact", rows), ("over", rows + 7), ("short", rows - 1)):
        k = a.place(np.empty(cap, np.uint32), align, "out", name="d_keys (%s)" % name)
        d = a.place(np.empty(cap, np.float32), align, "out", name="d_dist (%s)" % name)
        a.snapshot()
        rc = L.qadc_refine_range_collect_device(st._h, cap, a.ptr(k), a.ptr(d))
        if name == "short":
            assert rc == pyqadc.QADC_E_CAPACITY
            a.check_untouched([])                                            # nothing is copied ...
        else:
            assert rc == 0, L.qadc_last_error()
            a.check_untouched([(k, rows), (d, rows)])                        # ... and the 7 trailing entries stay
            assert ga.same(dict(keys=a.host(k)[:rows], dist=a.host(d)[:rows]), want) is None, name
    rc, keys, dist = st.range_collect_raw(rows)                              # ... and the result is still held
    assert rc == 0 and ga.same(dict(keys=keys[:rows], dist=dist[:rows]), want) is None


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("nq,dim,rows", SHAPES, ids=["nq%d-dim%d-rows%d" % k for k in SHAPES])
@pytest.mark.parametrize("dtype,keyed", STORES, ids=STORE_IDS)
def test_range_device_and_collect_device(pyqadc, dtype, keyed, nq, dim, rows, align):
    rng = np.random.default_rng(nq + 7 * keyed)
    st, vec, labels = make(pyqadc, rng, dtype, keyed, dim, rows)
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    d = ((vec[None, :, :].astype(np.float64) - queries[:, None, :]) ** 2).sum(-1)
    radius = np.quantile(d, 0.05, axis=1).astype(np.float32)
    radius[0] = np.inf                                                       # (at 9000 rows: a region overflows and the radix form sorts)
    f = pyqadc.AdcFilter(labels[1::5], "exclude")
    wl, wk, wd = st.range(queries, radius, filter=f)
    n = int(wl[-1])
    want = dict(keys=wk, dist=wd)
    assert n > 7 and wl[1] - wl[0] > rows // 2

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        a.snapshot()
        lims = np.zeros(nq + 1, np.uint64)
        rc = pyqadc.lib().qadc_refine_range_device(st._h, nq, a.ptr(q), fp(radius), f._h, up(lims))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([])                                                # the result is held on the store: no caller buffer is written
        assert np.array_equal(lims.astype(np.int64), wl)
        collect_cases(pyqadc, st, a, n, align, want)
        return dict(lims=lims)

    ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    f.close()
    st.close()


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("dtype,keyed", STORES, ids=STORE_IDS)
def test_rerank_range_device_and_collect_device(pyqadc, dtype, keyed, align):
    rng = np.random.default_rng(5 + keyed)
    nq, dim, rows = 5, 65, 6000
    st, vec, labels = make(pyqadc, rng, dtype, keyed, dim, rows)
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    sizes = [0, 1, 4500, 70, 9000]                                           # the LDS and the radix form; more than rerank takes
    in_lims = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    keys = rng.choice(np.concatenate([labels, [3, 0xFFFFFFFF]]), int(in_lims[-1])).astype(np.uint32)
    radius = np.array([np.inf, np.inf, np.inf, 125.0, 130.0], np.float32)
    wl, wk, wd, wm = st.rerank_range(queries, in_lims, keys, radius)
    n = int(wl[-1])
    want = dict(keys=wk, dist=wd)
    assert n > 3000 and wm > 0

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        k = a.place(keys, align, "in", name="d_keys")
        a.snapshot()
        lims, missing = np.zeros(nq + 1, np.uint64), C.c_uint64(0)
        rc = pyqadc.lib().qadc_refine_rerank_range_device(st._h, nq, a.ptr(q), up(in_lims), a.ptr(k), fp(radius), up(lims), C.byref(missing))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([])
        assert np.array_equal(lims.astype(np.int64), wl) and missing.value == wm
        collect_cases(pyqadc, st, a, n, align, want)
        return dict(lims=lims)

    ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    st.close()


@path_independent
def test_range_calls_refuse_pointers_below_the_stated_alignment(pyqadc):
    rng = np.random.default_rng(2)
    st, vec, labels = make(pyqadc, rng, "f32", False, 8, 200)
    queries = vec[:3].copy()
    radius = np.full(3, 4.0, np.float32)
    wl, wk, wd = st.range(queries, radius)
    n, want = int(wl[-1]), dict(keys=wk, dist=wd)
    a = ga.Arena(ga.P1, backend="torch", capacity=1 << 20)
    q = a.place(queries, 4, "in", name="d_queries")
    kin = a.place(wk, 4, "in", name="d_keys in")
    k = a.place(np.empty(n, np.uint32), 4, "out", name="d_keys")
    d = a.place(np.empty(n, np.float32), 4, "out", name="d_dist")
    L = pyqadc.lib()
    lims = np.zeros(4, np.uint64)
    a.snapshot()
    assert L.qadc_refine_range_collect_device(st._h, n, a.ptr(k) + 2, a.ptr(d)) == pyqadc.QADC_E_ARG and b"aligned" in L.qadc_last_error()
    assert L.qadc_refine_range_collect_device(st._h, n, a.ptr(k), a.ptr(d) + 1) == pyqadc.QADC_E_ARG
    a.check_untouched([])
    assert L.qadc_refine_range_collect_device(st._h, n, a.ptr(k), a.ptr(d)) == 0           # the refusals dropped nothing
    a.check_untouched([k, d])
    assert ga.same(dict(keys=a.host(k), dist=a.host(d)), want) is None
    a.snapshot()
    assert L.qadc_refine_range_device(st._h, 3, a.ptr(q) + 2, fp(radius), None, up(lims)) == pyqadc.QADC_E_ARG and b"d_queries" in L.qadc_last_error()
    in_lims = wl.astype(np.uint64)
    assert L.qadc_refine_rerank_range_device(st._h, 3, a.ptr(q) + 2, up(in_lims), a.ptr(kin), fp(radius), up(lims), None) == pyqadc.QADC_E_ARG
    assert L.qadc_refine_rerank_range_device(st._h, 3, a.ptr(q), up(in_lims), a.ptr(kin) + 2, fp(radius), up(lims), None) == pyqadc.QADC_E_ARG
    a.check_untouched([])
    assert L.qadc_refine_rerank_range_device(st._h, 3, a.ptr(q), up(in_lims), a.ptr(kin), fp(radius), up(lims), None) == 0
    a.check_untouched([])
    assert np.array_equal(lims, in_lims), "the exhaustive result re-ranked under the same radius is itself"
    st.close()
