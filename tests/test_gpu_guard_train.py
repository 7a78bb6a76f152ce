"""GPU: the memory behaviour of the learning entry points at the C-ABI, on guard-band arenas
(tests/guard_arena.py): qadc_pq_train_device, qadc_pq_train16_device, qadc_opq_cross_device and qadc_opq_train_device.  d_vectors is
their only device pointer, so the learning set is a window of an arena handed to pyqadc's *_device functions, which pass its address
on unchanged and allocate nothing on the device themselves.

W  no byte of the arena changes; R  codebooks, codes, rotation and cross matrix are bit-identical under the two guard poisons and
equal the host form's; A  d_vectors at 4 bytes (the 16-bit training at 16: its encoder loads 16 bytes), and at 256.
One round, and an n that is no multiple of the OPQ block of 2048 nor of a workgroup's tile."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = ["min", 256]
K = 3


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def al(align, minimum):
    return minimum if align == "min" else align


def learning_set(nsq, bits, n, ds=8, seed=0):
    rng = np.random.default_rng(1000 * nsq + bits + seed)
    dim = nsq * ds
    return (rng.normal(size=(n, dim)).astype(np.float32), rng.normal(size=(nsq, 1 << bits, ds)).astype(np.float32),
            rng.normal(size=(K, dim)).astype(np.float32))


def named(names, values):
    return {k: np.asarray(v) for k, v in zip(names, values)}


def on_arena(vectors, minimum, align, run, capacity=None):
    def call(a):
        v = a.place(vectors, al(align, minimum), "in", name="d_vectors")
        a.snapshot()
        got = run(v)
        a.check_untouched([])
        return got
    return ga.under_both_poisons(call, backend="torch", capacity=capacity or vectors.nbytes + (1 << 20))


TRAIN = [(8, 8), (16, 4)]


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("nsq,bits", TRAIN, ids=["%dx%d" % t for t in TRAIN])
def test_pq_train_device(pyqadc, nsq, bits, ivf, align):
    v, seed, coarse = learning_set(nsq, bits, 301)
    names = ("codebooks", "codes", "empty")
    want = named(names, pyqadc.train_pq(v, seed, 1, coarse=coarse if ivf else None))
    got = on_arena(v, 4, align, lambda t: named(names, pyqadc.train_pq_device(t, seed, 1, coarse=coarse if ivf else None)))
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
def test_pq_train16_device(pyqadc, ivf, align):
    v, seed, coarse = learning_set(2, 16, 301)
    names = ("codebooks", "codes", "empty")
    want = named(names, pyqadc.train_pq16(v, seed, 1, coarse=coarse if ivf else None))
    got = on_arena(v, 16, align, lambda t: named(names, pyqadc.train_pq16_device(t, seed, 1, coarse=coarse if ivf else None)))
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("nsq,bits", TRAIN, ids=["%dx%d" % t for t in TRAIN])
def test_opq_cross_device_and_train_device(pyqadc, nsq, bits, ivf, align):
    n = pyqadc.QADC_OPQ_BLOCK + 1
    v, seed, coarse = learning_set(nsq, bits, n, ds=2 if bits == 4 else 4)
    co = coarse if ivf else None
    cb, codes, _ = pyqadc.train_pq(v, seed, 1, coarse=co)
    want = dict(M=pyqadc.opq_cross(v, codes, cb, coarse=co))
    names = ("rotation", "codebooks", "codes", "empty", "rounds_done")
    want.update(named(names, pyqadc.train_opq(v, seed, 1, coarse=co)))

    def run(t):
        got = dict(M=pyqadc.opq_cross_device(t, codes, cb, coarse=co))
        got.update(named(names, pyqadc.train_opq_device(t, seed, 1, coarse=co)))
        return got

    got = on_arena(v, 4, align, run)
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
def test_learning_calls_refuse_a_learning_set_below_the_stated_alignment(pyqadc):
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    v8, seed8, _ = learning_set(8, 8, 40)
    v16, seed16, _ = learning_set(2, 16, 40)
    n, dim = v8.shape
    a = ga.Arena(ga.P1, backend="torch", capacity=1 << 20)
    good8 = a.place(v8, 4, "in", name="d_vectors")
    low16 = a.place(v16, 4, "in", name="d_vectors (16-bit) at 4 bytes")
    mid16 = a.place(v16, 8, "in", name="d_vectors (16-bit) at 8 bytes")
    assert a.ptr(good8) % 8 == 4 and a.ptr(low16) % 8 == 4 and a.ptr(mid16) % 16 == 8
    cb, codes, _ = pyqadc.train_pq(v8, seed8, 1)
    a.snapshot()
    for t in (low16, mid16):                                                 # through the wrapper: the same C check
        with pytest.raises(pyqadc.QadcError, match="d_vectors must be 16-byte aligned"):
            pyqadc.train_pq16_device(t, seed16, 1)
    f32p = C.POINTER(C.c_float)
    off = C.c_void_p(a.ptr(good8) + 2)                                       # 2 (mod 4) bytes: no float lies there
    seed, rot, out_codes = seed8.copy(), np.eye(dim, dtype=np.float32), np.zeros((n, 8), np.uint8)
    M, empty, done = np.zeros((dim, dim), np.float64), C.c_uint64(0), C.c_int32(0)
    assert L.qadc_pq_train_device(off, n, dim, 8, 8, 0, None, None, seed.ctypes.data_as(f32p), 1, out_codes.ctypes.data_as(C.c_void_p),
                                  C.byref(empty), 1, 1, 0) == E and b"d_vectors must be 4-byte aligned" in L.qadc_last_error()
    assert L.qadc_opq_cross_device(off, n, dim, 8, 8, 0, None, codes.ctypes.data_as(C.c_void_p), cb.ctypes.data_as(f32p),
                                   M.ctypes.data_as(C.POINTER(C.c_double)), 1, 0) == E and b"d_vectors must be 4-byte aligned" in L.qadc_last_error()
    assert L.qadc_opq_train_device(off, n, dim, 8, 8, 0, None, rot.ctypes.data_as(f32p), seed.ctypes.data_as(f32p), 1, 1,
                                   out_codes.ctypes.data_as(C.c_void_p), C.byref(empty), C.byref(done), 1, 1, 0) == E
    assert b"d_vectors must be 4-byte aligned" in L.qadc_last_error()
    a.check_untouched([])
    assert np.array_equal(seed, seed8) and not out_codes.any() and not M.any() and np.array_equal(rot, np.eye(dim, dtype=np.float32))
    got = pyqadc.train_pq_device(good8, seed8, 1)                            # the refusals left nothing behind
    assert np.array_equal(got[0].view(np.uint32), cb.view(np.uint32)) and np.array_equal(got[1], codes)
