"""CPU: the empty-cluster repair without a GPU.

1. The numpy definition's own distance: chain() equals kmeans_seed_compose's integer form on integer data and the exactly rounded
   fused step (in rationals) on floats.
2. The host twin (quick-adc_amd/host/pq_repair.hpp, driver tests/cpp/pq_repair_host.cpp) against the definition in numpy
   (tests/pq_repair_compose.py) on the crafted cases, codes and moved bit for bit; after a repair every cluster has a member wherever
   moved == E, and the non-empty clusters grow by exactly moved.
3. The `repair` overloads of the training twins (host/db_build.hpp) against the rounds composed from the oracle's assignment, the
   repair and the pinned update.
4. The argument refusals of qadc_pq_repair_host and of the repair flag, which come before the first HIP call."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import pq_repair_compose as prc
import pq_train_compose as ptc

NS = [1, 255, 1025]


@pytest.fixture(scope="module")
def driver():
    return prc.build_driver()


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pyqadc


def test_chain_is_the_integer_form_on_integer_data():
    rng = np.random.default_rng(1)
    sub, cen = (rng.integers(0, 1024, (500, 16)).astype(np.float32) for _ in range(2))
    assert np.array_equal(prc.chain(sub, cen), prc.int_distance(sub, cen))


def test_chain_is_the_exactly_rounded_fused_step():
    rng = np.random.default_rng(2)
    sub = (rng.normal(size=(300, 5)) * 10.0 ** rng.integers(-20, 18, (300, 5))).astype(np.float32)
    cen = (rng.normal(size=(300, 5)) * 10.0 ** rng.integers(-20, 18, (300, 5))).astype(np.float32)
    got = prc.chain(sub, cen)
    for i in range(len(sub)):
        acc = np.float32(0)
        for d in range(sub.shape[1]):
            t = np.float32(sub[i, d] - cen[i, d])
            exact = Fraction(float(t)) ** 2 + Fraction(float(acc))
            acc = np.float32(0) if exact == 0 else _round_f32(exact)
        assert acc.view(np.uint32) == got[i].view(np.uint32), (i, acc, got[i])


def _round_f32(q):
    """a positive rational to the nearest float32, ties to even; +inf past the largest"""
    if q >= Fraction(2) ** 128:
        return np.float32(np.inf)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)                                                         # subnormals share the smallest exponent
    scaled = q / Fraction(2) ** (e - 23)
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m & 1):
        m += 1
    with np.errstate(over="ignore"):
        return np.float32(np.ldexp(np.float64(m), e - 23))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("nsq,bits,dim", prc.SHAPES)
def test_twin_equals_the_definition_on_the_crafted_cases(driver, tmp_path, nsq, bits, dim, n):
    hit = set()
    for pattern in prc.PATTERNS:
        if pattern == "both_nibbles" and bits != 4:
            continue
        x, cb, codes = prc.crafted(pattern, nsq, bits, dim, n)
        want, want_moved = prc.repair(x, cb, codes)
        got, moved = prc.twin(driver, tmp_path, x, cb, codes)
        prc.same_codes(got, want, pattern)
        assert np.array_equal(moved, want_moved), pattern
        before, after = prc.counts(codes, nsq, bits), prc.counts(got, nsq, bits)
        E = (before == 0).sum(axis=1)
        assert np.array_equal((after > 0).sum(axis=1) - (before > 0).sum(axis=1), moved), pattern   # grows by exactly moved
        assert ((after > 0) >= (before > 0)).all(), pattern                 # a repair never empties a cluster
        assert (after[moved == E] > 0).all(), pattern                       # all alive wherever moved == E
        assert (moved <= E).all()
        if (moved < E).any():
            hit.add("fewer eligible than E")
        if ((moved == E) & (E > 0)).any():
            hit.add("full")
        if pattern == "all_alive" and n >= 1 << bits:
            assert moved.sum() == 0 and np.array_equal(got, codes)
        if pattern == "both_nibbles":
            a, b = prc.unpack(codes, 4), prc.unpack(got, 4)
            both = (a[:, 0::2] != b[:, 0::2]) & (a[:, 1::2] != b[:, 1::2])
            assert both.any() or n == 1                                     # both nibbles of one byte rewritten in one call
    # every vector in one cluster is E = K - 1 against n - 1 eligible: across NS both branches are taken
    assert ("fewer eligible than E" if n < 1 << bits else "full") in hit


def test_definition_by_hand():
    # one sub-space, K = 16: clusters 2 and 5 alive.  Distances to the assigned centroid: row 0: 9 (first of 2), 1: 4, 2: 9, 3: 0,
    # 4: 9 (first of 5), 5: 1.  Eligible: 1, 2, 5 (3 is at distance 0; 0 and 4 are firsts).  E = 14 > 3: all three move, in
    # ascending index onto empties 0, 1, 3.
    x = np.zeros((6, 2), np.float32)
    x[:, 0] = [3, 2, -3, 0, 13, 11]
    cb = np.zeros((1, 16, 2), np.float32)
    cb[0, 5, 0] = 10
    a = np.array([2, 2, 2, 2, 5, 5])
    got, moved = prc.repair_slice(x, cb[0], a)
    assert got.tolist() == [2, 0, 1, 2, 5, 3] and moved == 3
    # E = 1 (K = 4, clusters 0, 2, 3 alive): the farthest eligible is row 2 (9, against 4 and 1); with row 1 at 9 too the lower index wins
    cb4 = np.zeros((4, 2), np.float32)
    cb4[3, 0] = 10
    a4 = np.array([0, 0, 0, 2, 3, 3])
    assert prc.repair_slice(x, cb4, a4)[0].tolist() == [0, 0, 1, 2, 3, 3]
    x[1, 0] = -3
    assert prc.repair_slice(x, cb4, a4)[0].tolist() == [0, 1, 0, 2, 3, 3]


@pytest.mark.parametrize("kind", ["repeated", "nan"])
@pytest.mark.parametrize("nsq,bits,dim,n,iters", [(16, 4, 32, 300, 3), (4, 8, 8, 700, 3), (2, 16, 4, 300, 2)])
def test_training_twins_run_repaired_rounds(driver, po, tmp_path, nsq, bits, dim, n, iters, kind):
    v, seed = prc.train_case(nsq, bits, dim, n, kind)
    want = prc.train(po, v, seed, iters)
    got = prc.twin_train(driver, tmp_path, v, seed, iters, True)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    prc.same_codes(got[1], want[1])
    assert got[2:] == want[2:] and got[3] > 0
    plain = prc.twin_train(driver, tmp_path, v, seed, iters, False)
    unrepaired = prc.train(po, v, seed, iters, repair=False)
    assert np.array_equal(plain[0].view(np.uint32), unrepaired[0].view(np.uint32)) and plain[3] == 0
    # the repair leaves fewer NaN centroids.  (At 16 bits a set this small cannot fill 65536 clusters: the NaN centroids that remain
    # after round 1 take every vector in round 2 with or without the repair, so the count is compared after one round.)
    if bits == 16:
        assert plain[2] == unrepaired[2] >= got[2]
        assert prc.twin_train(driver, tmp_path, v, seed, 1, False)[2] > prc.twin_train(driver, tmp_path, v, seed, 1, True)[2]
    else:
        assert plain[2] == unrepaired[2] > got[2]


F32P = C.POINTER(C.c_float)


def test_refusals_come_before_the_first_hip_call(pyqadc):
    L = pyqadc.lib()
    v = np.zeros((10, 32), np.float32)
    cb = np.zeros((16, 16, 2), np.float32)
    codes = np.zeros((10, 8), np.uint8)
    vp, cp, kp = v.ctypes.data_as(F32P), cb.ctypes.data_as(F32P), codes.ctypes.data_as(C.c_void_p)

    def refused(word, *args):
        assert L.qadc_pq_repair_host(*args) == -1                           # QADC_E_ARG
        assert word in L.qadc_last_error().decode(), L.qadc_last_error()

    refused("sq_bits", vp, 10, 32, 16, 5, cp, kp, None, 0)
    refused("sq_count", vp, 10, 32, 7, 4, cp, kp, None, 0)
    refused("sq_count", vp, 10, 32, 3, 16, cp, kp, None, 0)
    refused("multiple", vp, 10, 33, 16, 4, cp, kp, None, 0)
    refused("NULL", None, 10, 32, 16, 4, cp, kp, None, 0)
    refused("NULL", vp, 10, 32, 16, 4, None, kp, None, 0)
    refused("codes", vp, 10, 32, 16, 4, cp, None, None, 0)
    refused("n <", vp, 0, 32, 16, 4, cp, kp, None, 0)
    refused("n <", vp, 1 << 32, 32, 16, 4, cp, kp, None, 0)
    empty, rep = C.c_uint64(0), C.c_uint64(0)
    for flag in (2, -1):
        assert L.qadc_pq_train_repair_host(vp, 10, 32, 16, 4, 0, None, None, cp, 1, kp, C.byref(empty), 1, 1, flag, C.byref(rep), 0) != 0
        assert "repair" in L.qadc_last_error().decode()
        assert L.qadc_pq_train16_repair_host(vp, 10, 32, 2, 0, None, None, cp, 1, kp, C.byref(empty), 1, 1, flag, C.byref(rep), 0) != 0
        assert "repair" in L.qadc_last_error().decode()
