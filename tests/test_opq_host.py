"""CPU: OPQ learning without a GPU.

1. qadc_procrustes_host through the library, in a process that never opens a device: orthogonality and optimality against
   numpy.linalg.svd with bounds from the float rounding of the result, the rank-deficient cases, the refusals.
2. The host twins (quick-adc_amd/host/db_build.hpp: opq_cross, opq_train_iterations; driver tests/cpp/opq_host.cpp): the cross matrix
   against a plain std::fmaf restatement bit for bit, and the learned rotation against plain PQ training on the issue's learning set.
3. The argument refusals of the C entry points, which come before the first HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

import adc_compose as ac
import opq_compose as oc
import pq_train_compose as ptc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORTHO = 2.0 ** -22      # rows of the double R are unit vectors; rounding to float moves a row by <= 2^-25 of its norm, so an entry of
                        # R R^T moves by <= 2^-24: a 4x margin for the Jacobi stop


@pytest.fixture(scope="module")
def driver():
    return oc.build_driver()


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pyqadc


def check_rotation(pyqadc, M):
    dim = M.shape[0]
    R, sweeps = pyqadc.procrustes(M)
    assert R.dtype == np.float32 and R.shape == (dim, dim) and 1 <= sweeps <= 64
    assert oc.orthogonality(R) <= ORTHO, oc.orthogonality(R)
    # the float rounding E has |E|_F <= 2^-25 sqrt(dim) and |M|_F <= sum(sigma): the loss is <= 2^-25 sqrt(dim) sum(sigma); 8x margin
    sigma = float(np.linalg.svd(M, compute_uv=False).sum())
    got = float(np.trace(R.astype(np.float64) @ M))
    assert got >= sigma * (1 - 2.0 ** -22 * np.sqrt(dim)), (got, sigma)
    again, sweeps2 = pyqadc.procrustes(M)
    assert np.array_equal(R, again) and sweeps == sweeps2        # deterministic
    return R


@pytest.mark.parametrize("dim", [2, 3, 32, 96, 128])
def test_procrustes_on_random_matrices(pyqadc, dim):
    rng = np.random.default_rng(dim)
    check_rotation(pyqadc, rng.normal(size=(dim, dim)))
    check_rotation(pyqadc, rng.normal(size=(dim, dim)) * 10.0 ** rng.integers(-6, 7, size=(1, dim)))   # columns of very different scale


@pytest.mark.parametrize("dim", [2, 3, 32])
def test_procrustes_on_rank_deficient_matrices(pyqadc, dim):
    rng = np.random.default_rng(100 + dim)
    check_rotation(pyqadc, rng.normal(size=(dim, 1)) @ rng.normal(size=(1, dim)))          # rank 1
    if dim > 3:
        check_rotation(pyqadc, rng.normal(size=(dim, 5)) @ rng.normal(size=(5, dim)))      # rank 5
    R = check_rotation(pyqadc, np.zeros((dim, dim)))
    assert np.array_equal(R, np.eye(dim, dtype=np.float32))      # nothing to align: the unit vectors in index order
    one = np.zeros((dim, dim))
    one[dim - 1, 0] = 2.0                                         # a single entry: rank 1 on the unit vectors themselves
    check_rotation(pyqadc, one)


@pytest.mark.parametrize("dim", [2, 3, 32, 128])
def test_a_positive_diagonal_gives_the_identity_exactly(pyqadc, dim):
    rng = np.random.default_rng(dim)
    R, sweeps = pyqadc.procrustes(np.diag(rng.uniform(0.1, 1e3, dim)))
    assert np.array_equal(R, np.eye(dim, dtype=np.float32)) and sweeps == 1


def test_procrustes_recovers_a_known_rotation(pyqadc):
    rng = np.random.default_rng(1)
    dim = 32
    Q = ac.random_rotation(rng, dim).astype(np.float64)
    x = rng.normal(size=(500, dim))
    R = check_rotation(pyqadc, x.T @ (x @ Q.T))                  # Y = X Q^T exactly: the best rotation is Q
    assert np.abs(R - Q).max() <= 1e-6


def test_procrustes_refusals(pyqadc):
    lib = pyqadc.lib()
    f64p, f32p = C.POINTER(C.c_double), C.POINTER(C.c_float)
    for bad in (np.nan, np.inf, -np.inf):
        M = np.eye(4)
        M[2, 1] = bad
        R = np.full((4, 4), 7.0, np.float32)
        assert lib.qadc_procrustes_host(M.ctypes.data_as(f64p), 4, R.ctypes.data_as(f32p), None) == pyqadc.QADC_E_ARG
        assert "non-finite" in lib.qadc_last_error().decode() and (R == 7.0).all()     # untouched
        with pytest.raises(pyqadc.QadcError, match="non-finite"):
            pyqadc.procrustes(M)
    M, R = np.eye(4), np.zeros((4, 4), np.float32)
    assert lib.qadc_procrustes_host(None, 4, R.ctypes.data_as(f32p), None) == pyqadc.QADC_E_ARG
    assert lib.qadc_procrustes_host(M.ctypes.data_as(f64p), 4, None, None) == pyqadc.QADC_E_ARG
    assert lib.qadc_procrustes_host(M.ctypes.data_as(f64p), 0, R.ctypes.data_as(f32p), None) == pyqadc.QADC_E_ARG
    assert lib.qadc_procrustes_host(M.ctypes.data_as(f64p), 1025, R.ctypes.data_as(f32p), None) == pyqadc.QADC_E_ARG
    with pytest.raises(pyqadc.QadcError):
        pyqadc.procrustes(np.zeros((3, 4)))


CROSS = {"16x4-d32": (16, 4, 32, 700), "32x4-d96": (32, 4, 96, 300), "4x8-d32": (4, 8, 32, 2049), "8x8-d24-two-blocks": (8, 8, 24, 2 * 2048 + 5)}


@pytest.mark.parametrize("coarse", [False, True], ids=["flat", "residual"])
@pytest.mark.parametrize("shape", sorted(CROSS))
def test_the_cross_twin_equals_the_plain_restatement(driver, po, tmp_path, shape, coarse):
    nsq, bits, dim, n = CROSS[shape]
    rng = np.random.default_rng([nsq, bits, dim, int(coarse)])
    v = rng.normal(size=(n, dim)).astype(np.float32)
    v[rng.choice(n, n // 10, replace=False)] *= np.float32(1e3)  # the order of a chain's terms shows
    co = v[rng.choice(n, 9, replace=False)].copy() if coarse else None
    cb = rng.normal(size=(nsq, 1 << bits, dim // nsq)).astype(np.float32)
    a = rng.integers(0, 1 << bits, (n, nsq))
    a[0], a[-1] = 0, (1 << bits) - 1                             # centroid 0 and the last one
    codes = ptc.pack(a, bits)
    x0, y = oc.x0_of(po, v, co), oc.reconstruction(cb, codes)
    M = oc.twin_cross(driver, tmp_path, v, codes, cb, co)
    want = oc.chain(driver, tmp_path, x0, y)
    oc.same_doubles(M, want, "the twin against the fmaf chains")
    assert (want != oc.chain(driver, tmp_path, x0, y, descending=True)).any()
    # (a sanity check of the orientation only — row a = X0, column b = Y: the float chains are far inside 1 % of the largest entry)
    np.testing.assert_allclose(M, x0.astype(np.float64).T @ y.astype(np.float64), rtol=0, atol=1e-2 * np.abs(M).max())


def test_the_train_twin_with_no_outer_round_is_pq_training(driver, po, tmp_path):
    rng = np.random.default_rng(4)
    n, nsq, bits, dim = 500, 16, 4, 32
    v = rng.normal(size=(n, dim)).astype(np.float32)
    seed = ptc.seed_rows(v, nsq, bits, rng.choice(n, 16, replace=False))
    rot = ac.random_rotation(rng, dim)
    x = ac.residuals(v, None, ac.assign(po, v, None, 1), rot)[:, 0, :]
    want_cb, want_codes, _ = ptc.train(po, x, seed, 2)
    got = oc.twin_train(driver, tmp_path, v, seed, 0, 2, rot)
    assert np.array_equal(got[0], rot) and got[4] == 0
    ac.assert_same_floats(got[1], want_cb)
    assert np.array_equal(got[2], want_codes) and got[3] == ptc.empty_count(want_cb)


def test_the_learned_rotation_beats_plain_pq_on_the_sketch_set(driver, tmp_path):
    """ten k-means rounds in both arms (the closing round of OPQ learning is its tenth): strict inequality, no figure"""
    v, seed = oc.sketch_set()
    eye = np.eye(32, dtype=np.float32)
    _, pq_cb, pq_codes, _, _ = oc.twin_train(driver, tmp_path, v, seed, 0, 10, eye)
    rot, cb, codes, empty, done = oc.twin_train(driver, tmp_path, v, seed, 9, 1, eye)
    assert done == 9                                             # (clusters may empty out as the rotation moves: nothing repairs them)
    assert oc.orthogonality(rot) <= ORTHO
    plain = ptc.reconstruction_error(v, pq_cb, pq_codes)
    learned = ptc.reconstruction_error(oc.rotated(v, rot), cb, codes)
    print("reconstruction error: plain PQ %.1f, learned OPQ %.1f, empty centroids %d" % (plain, learned, empty))
    assert learned < plain, (learned, plain)


def _cross_call(fn, pyqadc, vectors=1, n=100, dim=32, nsq=16, bits=4, K=0, coarse=None, codes=1, cb=1, M=1, sum_mode=1):
    f32p = C.POINTER(C.c_float)
    v, c, m = np.zeros((100, 64), np.float32), np.zeros(65536, np.float32), np.zeros(1 << 21, np.float64)
    k = np.zeros(100 * 32, np.uint8)
    vp = (v.ctypes.data_as(C.c_void_p) if fn.__name__.endswith("device") else v.ctypes.data_as(f32p)) if vectors else None
    return fn(vp, n, dim, nsq, bits, K, coarse, k.ctypes.data_as(C.c_void_p) if codes else None, c.ctypes.data_as(f32p) if cb else None,
              m.ctypes.data_as(C.POINTER(C.c_double)) if M else None, sum_mode, 0)


def _train_call(fn, pyqadc, vectors=1, n=100, dim=32, nsq=16, bits=4, K=0, coarse=None, rot=1, cb=1, outer=1, inner=1, div_mode=1, sum_mode=1):
    f32p = C.POINTER(C.c_float)
    v, c, r = np.zeros((100, 64), np.float32), np.zeros(65536, np.float32), np.zeros(1 << 21, np.float32)
    vp = (v.ctypes.data_as(C.c_void_p) if fn.__name__.endswith("device") else v.ctypes.data_as(f32p)) if vectors else None
    return fn(vp, n, dim, nsq, bits, K, coarse, r.ctypes.data_as(f32p) if rot else None, c.ctypes.data_as(f32p) if cb else None, outer, inner,
              None, None, None, div_mode, sum_mode, 0)


@pytest.mark.parametrize("entry", ["qadc_opq_cross_host", "qadc_opq_cross_device", "qadc_opq_train_host", "qadc_opq_train_device"])
def test_argument_refusals_come_before_any_hip_call(pyqadc, entry):
    """none of these reaches the device: they are refused alike with and without a GPU (the device forms are handed a host
    pointer here, which they must not touch)"""
    lib = pyqadc.lib()
    fn = getattr(lib, entry)
    call = _train_call if "train" in entry else _cross_call
    some = np.zeros(64, np.float32).ctypes.data_as(C.POINTER(C.c_float))

    def refused(needle, **kw):
        assert call(fn, pyqadc, **kw) == pyqadc.QADC_E_ARG, kw
        assert needle in lib.qadc_last_error().decode(), (kw, lib.qadc_last_error())

    refused("follow-up", bits=16, nsq=4)
    refused("multiple of sq_count", dim=33)
    refused("sq_count 16 or 32", nsq=8)
    refused("sq_count 4, 8 or 16", bits=8, nsq=32)
    refused("sq_bits must be 4 or 8", bits=5)
    refused("NULL", vectors=0)
    refused("NULL", cb=0)
    refused("coarse", K=20, coarse=None)
    refused("K_coarse", K=-1, coarse=some)
    refused("0 < n < 2^32", n=0)
    refused("0 < n < 2^32", n=2 ** 32)
    refused("<= 1024", dim=1024 + 16)
    refused("<= 1024", bits=8, nsq=4, dim=1028)
    refused("sum_mode", sum_mode=2)
    if "train" in entry:
        refused("rotation", rot=0)
        refused("outer", outer=-1)
        refused("inner", inner=0)
        refused("div_mode", div_mode=-1)
    else:
        refused("codes", codes=0)
        refused("M_out", M=0)


def test_python_front_refuses_bad_shapes(pyqadc):
    v = np.zeros((50, 32), np.float32)
    cb = np.zeros((16, 16, 2), np.float32)
    with pytest.raises(pyqadc.QadcError, match="codes"):
        pyqadc.opq_cross(v, np.zeros((50, 16), np.uint8), cb)     # 4-bit codes are packed: [n][8]
    with pytest.raises(pyqadc.QadcError, match="rotation"):
        pyqadc.train_opq(v, cb, 1, rotation=np.eye(16, dtype=np.float32))
    with pytest.raises(pyqadc.QadcError, match="follow-up"):
        pyqadc.train_opq(np.zeros((50, 32), np.float32), np.zeros((4, 65536, 8), np.float32), 1)
    with pytest.raises(TypeError):
        pyqadc.train_opq_device(v, cb, 1)
    with pytest.raises(TypeError):
        pyqadc.opq_cross_device(v, np.zeros((50, 8), np.uint8), cb)
