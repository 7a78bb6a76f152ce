"""GPU: learning the OPQ rotation (qadc_opq_train_host / _device; pyqadc.train_opq, train_opq_device).

Primary expectation: the same loop written with the public calls (opq_compose.composed: train_pq with the rotation, opq_cross,
procrustes), bit for bit in rotation, codebooks and codes.  Second expectation: the CPU twin opq_train_iterations."""
import ctypes as C

import numpy as np
import pytest

import adc_compose as ac
import opq_compose as oc
import pq_train_compose as ptc
import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

SHAPES = {"16x4-d32": (16, 4, 32, 1500), "8x8-d32": (8, 8, 32, 2500)}
ORTHO = 2.0 ** -22


@pytest.fixture(scope="module")
def driver():
    return oc.build_driver()


def make(shape, coarse, start):
    nsq, bits, dim, n = SHAPES[shape]
    rng = np.random.default_rng([nsq, bits, int(coarse), int(start == "random")])
    v = (rng.normal(size=(n, dim)) * 0.9 ** np.arange(dim)).astype(np.float32) @ ac.random_rotation(rng, dim)
    v = np.ascontiguousarray(v, np.float32)
    co = v[rng.choice(n, 12, replace=False)].copy() if coarse else None
    seed = ptc.seed_rows(v, nsq, bits, rng.choice(n, 1 << bits, replace=False))
    rot = ac.random_rotation(rng, dim) if start == "random" else np.eye(dim, dtype=np.float32)
    return v, seed, co, rot


def same(got, want, what):
    ac.assert_same_floats(got[0], want[0], what + ": rotation")
    ac.assert_same_floats(got[1], want[1], what + ": codebooks")
    assert np.array_equal(got[2], want[2]), what + ": codes"
    assert got[3:] == want[3:], what + ": empty, rounds_done"


@path_independent
@pytest.mark.parametrize("start", ["identity", "random"])
@pytest.mark.parametrize("coarse", [False, True], ids=["flat", "residual"])
@pytest.mark.parametrize("inner", [1, 2])
@pytest.mark.parametrize("outer", [0, 1, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_loop_equals_the_public_calls_and_the_twin(driver, tmp_path, shape, outer, inner, coarse, start):
    v, seed, co, rot0 = make(shape, coarse, start)
    keep = rot0.copy()
    got = pyqadc.train_opq(v, seed, outer, inner, rotation=rot0, coarse=co)
    assert np.array_equal(rot0, keep)                                # the caller's start is copied
    assert got[4] == outer
    same(got, oc.composed(pyqadc, v, seed, outer, inner, rot0, co), "against the public calls")
    same(got, oc.twin_train(driver, tmp_path, v, seed, outer, inner, rot0, co), "against the CPU twin")
    assert oc.orthogonality(got[0]) <= ORTHO
    if outer == 0:
        assert np.array_equal(got[0], rot0)
        cb, codes, empty = pyqadc.train_pq(v, seed, inner, coarse=co, rotation=rot0)
        ac.assert_same_floats(got[1], cb)
        assert np.array_equal(got[2], codes) and got[3] == empty
    elif start == "identity":
        assert not np.array_equal(got[0], rot0)                      # the rotation was learned


@path_independent
def test_the_source_division_and_the_default_rotation(driver, tmp_path):
    v, seed, co, _ = make("16x4-d32", True, "identity")
    got = pyqadc.train_opq(v, seed, 2, coarse=co, div_mode=0)        # rotation None: the identity
    same(got, oc.composed(pyqadc, v, seed, 2, 1, np.eye(32, dtype=np.float32), co, div_mode=0), "div_mode 0")
    same(got, oc.twin_train(driver, tmp_path, v, seed, 2, 1, np.eye(32, dtype=np.float32), co, div_mode=0), "div_mode 0, twin")
    assert (got[1].view(np.uint32) != pyqadc.train_opq(v, seed, 2, coarse=co)[1].view(np.uint32)).any()


@path_independent
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_device_form_equals_the_host_form(shape):
    import torch
    v, seed, co, rot0 = make(shape, True, "random")
    want = pyqadc.train_opq(v, seed, 2, 2, rotation=rot0, coarse=co)
    t = torch.from_numpy(v).to("cuda:0")
    for _ in range(2):
        same(pyqadc.train_opq_device(t, seed, 2, 2, rotation=rot0, coarse=co), want, "the device form")
    assert np.array_equal(t.cpu().numpy(), v)                        # the learning set is read only
    with pytest.raises(pyqadc.QadcError):
        pyqadc.train_opq_device(torch.from_numpy(v), seed, 1)        # a host tensor


@path_independent
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_non_finite_learning_set_stops_the_rotation_updates(shape):
    v, seed, co, rot0 = make(shape, False, "random")
    v[v.shape[0] // 2, 3] = np.inf
    got = pyqadc.train_opq(v, seed, 3, 1, rotation=rot0)
    assert got[4] == 0 and np.array_equal(got[0], rot0)              # no update completed, the rotation untouched
    same(got, oc.composed(pyqadc, v, seed, 3, 1, rot0), "against the public calls")
    cb = pyqadc.train_pq(v, pyqadc.train_pq(v, seed, 1, rotation=rot0)[0], 1, rotation=rot0)[0]
    ac.assert_same_floats(got[1], cb, "one round and the closing round")


@path_independent
def test_the_learned_rotation_beats_plain_pq_on_the_sketch_set():
    """ten k-means rounds in both arms (the closing round of OPQ learning is its tenth): strict inequality, no figure"""
    v, seed = oc.sketch_set()
    pq_cb, pq_codes, _ = pyqadc.train_pq(v, seed, 10)
    rot, cb, codes, empty, done = pyqadc.train_opq(v, seed, 9, 1)
    assert done == 9 and oc.orthogonality(rot) <= ORTHO
    plain = ptc.reconstruction_error(v, pq_cb, pq_codes)
    learned = ptc.reconstruction_error(oc.rotated(v, rot), cb, codes)
    print("reconstruction error: plain PQ %.1f, learned OPQ %.1f, empty centroids %d" % (plain, learned, empty))
    assert learned < plain, (learned, plain)


@path_independent
@pytest.mark.parametrize("bits", [4, 8])
def test_the_learned_pair_serves_an_index(bits):
    shape = "16x4-d32" if bits == 4 else "8x8-d32"
    nsq, _, dim, n = SHAPES[shape]
    v, seed, co, _ = make(shape, True, "identity")
    rot, cb, codes, empty, done = pyqadc.train_opq(v, seed, 3, 1, coarse=co)
    assert done == 3
    idx = pyqadc.Index(nsq) if bits == 4 else pyqadc.AdcIndex(nsq, 8)
    try:
        idx.set_pq(cb)
        idx.set_rotation(rot)
        idx.set_coarse(co)
        idx.add_vectors(v)
        if bits == 4:
            idx.finalize(0.5)
            r = idx.search(v[:4], 3, 10)
            assert (r["status"] == 0).all() and (r["sizes"] == 10).all() and (r["keys"] < n).all()
        else:
            keys, vals, sizes, _ = idx.search(v[:4], 3, 10)
            assert (sizes == 10).all() and (keys < n).all()
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("entry", ["qadc_opq_train_host", "qadc_opq_cross_host"])
def test_refusals_leave_the_outputs_untouched(entry):
    """every refusal comes before any device work (tests/test_opq_host.py walks them without a GPU); here: with a GPU present the
    outputs of a refused call are still untouched"""
    lib = pyqadc.lib()
    f32p = C.POINTER(C.c_float)
    v, cb = np.zeros((100, 32), np.float32), np.full((16, 16, 2), 3.0, np.float32)
    rot, M, codes = np.full((32, 32), 5.0, np.float32), np.full((32, 32), 9.0), np.zeros((100, 8), np.uint8)
    for kw in (dict(bits=16), dict(dim=33), dict(n=0), dict(outer=-1), dict(inner=0), dict(sum_mode=3)):
        a = dict(dict(n=100, dim=32, nsq=16, bits=4, outer=1, inner=1, sum_mode=1), **kw)
        if entry == "qadc_opq_train_host":
            rc = lib.qadc_opq_train_host(v.ctypes.data_as(f32p), a["n"], a["dim"], a["nsq"], a["bits"], 0, None, rot.ctypes.data_as(f32p),
                                         cb.ctypes.data_as(f32p), a["outer"], a["inner"], codes.ctypes.data_as(C.c_void_p), None, None, 1,
                                         a["sum_mode"], 0)
        elif "outer" in kw or "inner" in kw:
            continue
        else:
            rc = lib.qadc_opq_cross_host(v.ctypes.data_as(f32p), a["n"], a["dim"], a["nsq"], a["bits"], 0, None, codes.ctypes.data_as(C.c_void_p),
                                         cb.ctypes.data_as(f32p), M.ctypes.data_as(C.POINTER(C.c_double)), a["sum_mode"], 0)
        assert rc == pyqadc.QADC_E_ARG, kw
        assert (rot == 5.0).all() and (cb == 3.0).all() and (M == 9.0).all() and not codes.any()
