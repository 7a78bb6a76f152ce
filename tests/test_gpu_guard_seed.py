"""GPU: the memory behaviour of qadc_kmeans_seed_device and qadc_kmeans_seed_host at the C-ABI, on guard-band
arenas (tests/guard_arena.py).  d_vectors is the only device pointer: the learning set is a window of a device arena.  centres_out and
rows_out are host memory: windows of a host arena, so that a byte written beside them shows.

W  no byte of the device arena changes, and of the host arena exactly centres_out and rows_out; R  centres, rows and fallbacks are
bit-identical under the two guard poisons and equal the host form's; A  d_vectors at 4 bytes and at 256; a refused call writes
nothing.  n is no multiple of a wave's 64 rows, dim no multiple of the 32-column window, and two workgroups run."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
import kmeans_seed_compose as ks
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32P, U32P = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
N, DIM, SQ, K, SEED = 4096 + 77, 20, 4, 9, 31


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def call(L, name, vectors, host, centres, rows, fallbacks, n=N, k=K, coarse=None):
    co = None if coarse is None else coarse.ctypes.data_as(F32P)
    vec = vectors if name.endswith("device") else C.cast(vectors, F32P)
    return getattr(L, name)(vec, n, DIM, SQ, k, 0 if coarse is None else len(coarse), co, None, SEED,
                            C.cast(C.c_void_p(host.ptr(centres)), F32P), C.cast(C.c_void_p(host.ptr(rows)), U32P), C.byref(fallbacks), 0)


@path_independent
@pytest.mark.parametrize("align", [4, 256])
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
def test_outputs_are_written_exactly_and_the_learning_set_is_left_alone(pyqadc, align, ivf):
    L = pyqadc.lib()
    v = ks.real_set(N, DIM)
    coarse = np.ascontiguousarray(v[[5, 900, 4100]] + np.float32(0.5)) if ivf else None
    want = dict(zip(("centres", "rows", "fallbacks"), pyqadc.kmeans_seed(v, K, sq_count=SQ, seed=SEED, coarse=coarse, return_rows=True)))

    def run(dev):
        host = ga.Arena(dev.poison, backend="numpy", capacity=1 << 20)
        d_v = dev.place(v, align, "in", name="d_vectors")
        centres = host.place(np.zeros((SQ, K, DIM // SQ), np.float32), 4, "out", name="centres_out")
        rows = host.place(np.zeros((SQ, K), np.uint32), 4, "out", name="rows_out")
        dev.snapshot()
        host.snapshot()
        fallbacks = C.c_uint64(12345)
        assert call(L, "qadc_kmeans_seed_device", C.c_void_p(dev.ptr(d_v)), host, centres, rows, fallbacks, coarse=coarse) == 0, L.qadc_last_error()
        dev.check_untouched([])
        host.check_untouched([centres, rows])
        return dict(centres=host.host(centres), rows=host.host(rows), fallbacks=fallbacks.value)

    got = ga.under_both_poisons(run, backend="torch", capacity=v.nbytes + (1 << 20))
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
def test_the_host_form_writes_its_outputs_exactly(pyqadc):
    L = pyqadc.lib()
    v = ks.real_set(N, DIM)
    want = dict(zip(("centres", "rows", "fallbacks"), pyqadc.kmeans_seed(v, K, sq_count=SQ, seed=SEED, return_rows=True)))

    def run(host):
        h_v = host.place(v, 4, "in", name="vectors")
        centres = host.place(np.zeros((SQ, K, DIM // SQ), np.float32), 4, "out", name="centres_out")
        rows = host.place(np.zeros((SQ, K), np.uint32), 4, "out", name="rows_out")
        host.snapshot()
        fallbacks = C.c_uint64(12345)
        assert call(L, "qadc_kmeans_seed_host", C.c_void_p(host.ptr(h_v)), host, centres, rows, fallbacks) == 0, L.qadc_last_error()
        host.check_untouched([centres, rows])
        return dict(centres=host.host(centres), rows=host.host(rows), fallbacks=fallbacks.value)

    got = ga.under_both_poisons(run, backend="numpy", capacity=v.nbytes + (1 << 20))
    assert ga.same(got, want) is None, "%s differs" % ga.same(got, want)


@path_independent
def test_a_refused_call_writes_nothing(pyqadc):
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    v = ks.real_set(N, DIM)
    dev = ga.Arena(ga.P1, backend="torch", capacity=v.nbytes + (1 << 20))
    host = ga.Arena(ga.P1, backend="numpy", capacity=1 << 20)
    d_v = dev.place(v, 4, "in", name="d_vectors")
    centres = host.place(np.zeros((SQ, K, DIM // SQ), np.float32), 4, "out", name="centres_out")
    rows = host.place(np.zeros((SQ, K), np.uint32), 4, "out", name="rows_out")
    assert dev.ptr(d_v) % 8 == 4
    dev.snapshot()
    host.snapshot()
    fallbacks = C.c_uint64(12345)
    for kw, message in ((dict(k=0), b"1 <= k <= n"), (dict(k=N + 1), b"1 <= k <= n"), (dict(n=0), b"0 < n < 2^32")):
        rc = call(L, "qadc_kmeans_seed_device", C.c_void_p(dev.ptr(d_v)), host, centres, rows, fallbacks, **kw)
        assert rc == E and message in L.qadc_last_error()
    rc = call(L, "qadc_kmeans_seed_device", C.c_void_p(dev.ptr(d_v) + 2), host, centres, rows, fallbacks)   # 2 (mod 4): no float lies there
    assert rc == E and b"d_vectors must be 4-byte aligned" in L.qadc_last_error()
    dev.check_untouched([])
    host.check_untouched([])
    assert fallbacks.value == 12345
    assert call(L, "qadc_kmeans_seed_device", C.c_void_p(dev.ptr(d_v)), host, centres, rows, fallbacks) == 0   # the refusals left nothing behind
    want = pyqadc.kmeans_seed(v, K, sq_count=SQ, seed=SEED, return_rows=True)
    assert np.array_equal(host.host(rows), want[1]) and np.array_equal(ga.bits(host.host(centres)), ga.bits(want[0])) and fallbacks.value == want[2]
