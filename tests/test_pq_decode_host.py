"""CPU: the PQ decoder without a GPU (include/qadc.h "Reconstruction").

1. The numpy definition's fused step: fma() equals the exactly rounded a * b + c (in rationals).
2. The host twin (quick-adc_amd/host/pq_decode.hpp, driver tests/cpp/pq_decode_host.cpp) against the definition in numpy
   (tests/pq_decode_compose.py) for every (sq_count, sq_bits) pair, with and without rotation, coarse quantizer and error, on
   missing rows and on NaN and infinite centroids, bit for bit; the lookup twin against a dictionary.
3. The exactness fixtures: on small-integer quantizers decode(encode(x)) == x and encode(decode(codes)) == codes under the CPU
   statements of the encoders — what the GPU round trip relies on.
4. The refusals of qadc_pq_decode_host / _device and of the index forms' null index, which come before the first HIP call."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import pq_decode_compose as pdc
from test_pq_repair_host import _round_f32


@pytest.fixture(scope="module")
def driver():
    return pdc.build_driver()


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pyqadc


def test_fma_is_the_exactly_rounded_fused_step():
    rng = np.random.default_rng(3)
    a, b, c = ((rng.normal(size=400) * 10.0 ** rng.integers(-18, 18, 400)).astype(np.float32) for _ in range(3))
    c[:50] = -(a[:50].astype(np.float64) * b[:50]).astype(np.float32)       # cancellation: the product's low bits decide
    got = pdc.fma(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        want = np.float32(0) if exact == 0 else (_round_f32(exact) if exact > 0 else -_round_f32(-exact))
        assert np.float32(want).view(np.uint32) == got[i].view(np.uint32), (i, a[i], b[i], c[i], want, got[i])


SHAPES = [(nsq, bits, nsq * ds) for nsq, bits in pdc.PAIRS for ds in ((1, 3) if bits != 16 else (2,))]


@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("K", [0, 5], ids=["flat", "ivf"])
@pytest.mark.parametrize("nsq,bits,dim", SHAPES, ids=["%dx%d-dim%d" % s for s in SHAPES])
def test_twin_equals_the_definition(driver, tmp_path, nsq, bits, dim, K, rotated):
    rng = np.random.default_rng(dim + bits + K)
    c = pdc.random_case(rng, nsq, bits, dim, 37, K, rotated)
    if K:
        c["assign"][[3, 20]] = (-1, K)                                      # missing rows
    want = pdc.restate(c["cb"], c["codes"], c["assign"], c["coarse"], c["rotation"], c["vectors"])
    got = pdc.twin(driver, tmp_path, c["cb"], c["codes"], c["assign"], c["coarse"], c["rotation"], c["vectors"])
    pdc.same_floats(got[0], want[0], "out")
    pdc.same_floats(got[1], want[1], "err")
    plain = pdc.twin(driver, tmp_path, c["cb"], c["codes"], c["assign"], c["coarse"], c["rotation"])
    pdc.same_floats(plain, want[0], "out without err")
    if K:
        assert (got[0][[3, 20]].view(np.uint32) == pdc.NAN_BITS).all() and np.isnan(got[1][[3, 20]]).all()
    if not rotated and not K:                                               # a copy: every float is a codebook float
        a = pdc.unpack(c["codes"], bits)
        ds = dim // nsq
        for m in range(nsq):
            pdc.same_floats(got[0][:, m * ds:(m + 1) * ds], c["cb"][m][a[:, m]], "gather")


@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
def test_nonfinite_centroids(driver, tmp_path, rotated):
    """Without a rotation a NaN or infinite centroid component stays in its component; under one it reaches the whole row."""
    rng = np.random.default_rng(9)
    c = pdc.random_case(rng, 4, 8, 12, 30, 3, rotated)
    a = pdc.unpack(c["codes"], 8)
    a[[2, 5, 9], 1] = (10, 11, 12)
    c["codes"] = pdc.pack(a, 8)
    for row, val in ((2, np.nan), (5, np.inf), (9, -np.inf)):
        c["cb"][1, a[row, 1], 2] = val
    want = pdc.restate(c["cb"], c["codes"], c["assign"], c["coarse"], c["rotation"], c["vectors"])
    got = pdc.twin(driver, tmp_path, c["cb"], c["codes"], c["assign"], c["coarse"], c["rotation"], c["vectors"])
    nan_any = np.isnan(got[0])
    pdc.same_floats(got[0], want[0], "out")
    pdc.same_floats(got[1], want[1], "err")
    assert (got[0].view(np.uint32)[nan_any] == pdc.NAN_BITS).all()          # arithmetic was done (K > 0): the canonical NaN
    if rotated:
        assert nan_any[2].all() and not np.isfinite(got[0][[5, 9]]).any()    # every chain passes the component: the whole row
    else:
        assert nan_any[2].sum() == 1 and np.isposinf(got[0][5, 5]) and np.isneginf(got[0][9, 5])


def test_lookup_twin(driver, tmp_path):
    rng = np.random.default_rng(4)
    sizes = [5, 0, 7, 3]
    labels = [rng.integers(0, 12, n).astype(np.uint32) for n in sizes]      # repeats inside and across partitions
    labels[2][1] = 0xFFFFFFFF
    keys = np.concatenate([np.arange(14, dtype=np.uint32), [0xFFFFFFFF, 3, 3]]).astype(np.uint32)
    want = pdc.where_numpy(sizes, labels, None, keys)
    assert np.array_equal(pdc.twin_where(driver, tmp_path, sizes, labels, None, keys), want)
    assert (want == pdc.MISSING).any() and (want != pdc.MISSING).any()
    base = [100, 0, 103, 2]                                                 # unlabelled: key_base + position, partitions share keys
    keys = np.array([100, 104, 105, 106, 109, 110, 2, 4, 5, 0], np.uint32)
    want = pdc.where_numpy(sizes, None, base, keys)
    assert np.array_equal(pdc.twin_where(driver, tmp_path, sizes, None, base, keys), want)
    assert want[1] == (0 << 32 | 4) and want[3] == (2 << 32 | 3)            # 104: partition 0 row 4 beats partition 2 row 1


EXACT = [(16, 4, 32), (32, 4, 32), (4, 8, 8), (4, 8, 4), (8, 8, 16), (16, 8, 32), (2, 16, 4), (2, 16, 8)]


@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("K", [0, 6], ids=["flat", "ivf"])
@pytest.mark.parametrize("nsq,bits,dim", EXACT, ids=["%dx%d-dim%d" % s for s in EXACT])
def test_exactness_fixtures_round_trip_under_the_twins(driver, po, tmp_path, nsq, bits, dim, K, rotated):
    """decode(encode(x)) == x for x made of centroid rows, and encode(decode(codes)) == codes: pq_decode_compose.exact_fixture argues
    why every product and sum is an exact integer; here the encoders' CPU statements are held to it before the GPU relies on it."""
    fx = pdc.exact_fixture(nsq, bits, dim, K, rotated)
    n = 40 if bits != 16 else 6                                             # (the 16-bit oracle distances cost 65536 per row)
    codes, assign = pdc.exact_rows(fx, n)
    x = pdc.twin(driver, tmp_path, fx["cb"], codes, assign, fx["coarse"], fx["rotation"])
    pdc.same_floats(x, pdc.restate(fx["cb"], codes, assign, fx["coarse"], fx["rotation"]), "decode")
    assert np.array_equal(x, np.round(x)) and (x != 0).all() and np.abs(x).max() <= 2 * fx["S"] + fx["A"]
    got_assign, got_codes = pdc.encode_twin(po, fx, x)
    assert np.array_equal(np.asarray(got_codes).view(np.uint8), np.asarray(codes).view(np.uint8)), "encode(decode(codes)) != codes"
    if K:
        assert np.array_equal(got_assign, assign)
    again, err = pdc.twin(driver, tmp_path, fx["cb"], got_codes, got_assign, fx["coarse"], fx["rotation"], x)
    pdc.same_floats(again, x, "decode(encode(x))")
    assert (err.view(np.uint32) == 0).all()                                 # +0.0 exactly


F32P = C.POINTER(C.c_float)
I32P = C.POINTER(C.c_int32)


def test_refusals_come_before_the_first_hip_call(pyqadc):
    L = pyqadc.lib()
    cb = np.zeros((4, 256, 2), np.float32)
    codes = np.zeros((10, 4), np.uint8)
    assign = np.zeros(10, np.int32)
    coarse = np.zeros((3, 8), np.float32)
    v = np.zeros((10, 8), np.float32)
    out = np.full((10, 8), 7, np.float32)
    err = np.full(10, 7, np.float32)
    cp, kp, ap, qp, vp, op, ep = (cb.ctypes.data_as(F32P), codes.ctypes.data_as(C.c_void_p), assign.ctypes.data_as(I32P),
                                  coarse.ctypes.data_as(F32P), v.ctypes.data_as(F32P), out.ctypes.data_as(F32P), err.ctypes.data_as(F32P))

    def refused(word, *args):
        for fn in (L.qadc_pq_decode_host, L.qadc_pq_decode_device):
            a = list(args)
            if fn is L.qadc_pq_decode_device:                                # its device pointers are void*: pass the addresses
                for i in (7, 8, 10, 11, 12):
                    a[i] = None if a[i] is None else C.cast(a[i], C.c_void_p)
            assert fn(*a) == pyqadc.QADC_E_ARG, (word, fn.__name__)
            assert word in L.qadc_last_error().decode(), L.qadc_last_error()

    #        sq_count, sq_bits, dim, codebooks, rotation, K, coarse, assign, codes, n, vectors, out, err_out, device
    refused("sq_bits", 4, 5, 8, cp, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("sq_count", 7, 8, 14, cp, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("sq_count", 4, 4, 8, cp, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("sq_count", 16, 16, 32, cp, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("multiple", 4, 8, 9, cp, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("<= 2048", 16, 4, 2064, cp, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("<= 4096", 4, 8, 4100, cp, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("codebooks", 4, 8, 8, None, None, 0, None, None, kp, 10, None, op, None, 0)
    refused("K must", 4, 8, 8, cp, None, -1, None, None, kp, 10, None, op, None, 0)
    refused("coarse", 4, 8, 8, cp, None, 3, None, ap, kp, 10, None, op, None, 0)
    refused("assign", 4, 8, 8, cp, None, 3, qp, None, kp, 10, None, op, None, 0)
    refused("vectors", 4, 8, 8, cp, None, 0, None, None, kp, 10, None, op, ep, 0)
    refused("codes", 4, 8, 8, cp, None, 0, None, None, None, 10, None, op, None, 0)
    refused("out", 4, 8, 8, cp, None, 0, None, None, kp, 10, None, None, None, 0)
    assert (out == 7).all() and (err == 7).all()
    # a pointer below the stated alignment (device form only)
    off = C.c_void_p(out.ctypes.data + 2)
    assert L.qadc_pq_decode_device(4, 8, 8, cp, None, 0, None, None, kp, 10, None, off, None, 0) == pyqadc.QADC_E_ARG
    assert b"d_out must be 4-byte aligned" in L.qadc_last_error()
    # n = 0 touches nothing, not even the device
    assert L.qadc_pq_decode_host(4, 8, 8, cp, None, 0, None, None, None, 0, None, None, None, 0) == 0
    # the index forms on a null index
    for fn, args in ((L.qadc_adc_index_reconstruct, (None, None, 0, None, None)), (L.qadc_adc_index_reconstruct_device, (None, None, 0, None, None)),
                     (L.qadc_adc_index_reconstruct_rows, (None, 0, 0, 0, None)), (L.qadc_adc_index_reconstruct_rows_device, (None, 0, 0, 0, None))):
        assert fn(*args) == pyqadc.QADC_E_ARG and b"null" in L.qadc_last_error()
