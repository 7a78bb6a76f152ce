"""GPU: training with repaired rounds (qadc_pq_train_repair_*, qadc_pq_train16_repair_*, qadc_opq_train_repair_*; the repair=
keyword of pyqadc.train_pq, train_pq16, train_opq and their _device forms).

Primary expectation: the rounds composed from the oracle's assignment, the repair in numpy and the pinned update
(pq_repair_compose.train) — codebooks, codes, empty and repaired bit for bit, 3 rounds at 4 and 8 bits and 2 at 16, from a seed
holding repeated rows and from one holding a NaN row, on a learning set with a block of identical sub-vectors.  Then: the case the
feature is for (the plain call returns NaN centroids, the repaired one none), repair = 0 through the new entry points against the old
ones, the device forms, OPQ as the loop of the repaired public calls, repeatability and a good call after a refused one."""
import ctypes as C

import numpy as np
import pytest

import adc_compose as ac
import pq_repair_compose as prc
import pq_train_compose as ptc
import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

F32P = C.POINTER(C.c_float)
ROUNDS = [(16, 4, 32, 300, 3), (4, 8, 8, 700, 3), (2, 16, 4, 300, 2)]


def train(v, seed, iters, **kw):
    return (pyqadc.train_pq16 if seed.shape[1] == 65536 else pyqadc.train_pq)(v, seed, iters, **kw)


def same(got, want, what=""):
    ac.assert_same_floats(got[0], want[0], what + ": codebooks")
    prc.same_codes(got[1], want[1], what)
    assert tuple(got[2:]) == tuple(want[2:]), (what, got[2:], want[2:])


@path_independent
@pytest.mark.parametrize("kind", ["repeated", "nan"])
@pytest.mark.parametrize("nsq,bits,dim,n,iters", ROUNDS, ids=["%dx%d" % r[:2] for r in ROUNDS])
def test_repaired_rounds_against_the_composition(po, nsq, bits, dim, n, iters, kind):
    v, seed = prc.train_case(nsq, bits, dim, n, kind)
    want = prc.train(po, v, seed, iters)
    got = train(v, seed, iters, repair=True)
    same(got, want, "repaired")
    assert got[3] > 0


def dying_case(bits):
    """4 and 8 bits: a seed with repeated rows — the later copies of a row never win a vector and die.  16 bits: 1.5 vectors per
    centroid and a seed drawn like the data, not from it — about e^-1.5 of the clusters start empty, and the vectors beyond every
    cluster's first outnumber them, so a repaired round can fill them all."""
    nsq, dim, n = {4: (16, 32, 2000), 8: (8, 16, 5000), 16: (2, 4, 98304)}[bits]
    rng = np.random.default_rng(bits)
    K = 1 << bits
    v = np.ascontiguousarray(rng.normal(size=(n, dim)), np.float32)
    if bits == 16:
        return v, np.ascontiguousarray(rng.normal(size=(nsq, K, dim // nsq)), np.float32)
    rows = rng.choice(n, K, replace=False)
    rows[1::4] = rows[0::4][:len(rows[1::4])]
    return v, np.ascontiguousarray(v[rows].reshape(K, nsq, dim // nsq).transpose(1, 0, 2))


@path_independent
@pytest.mark.parametrize("bits", [4, 8, 16])
def test_the_plain_call_loses_centroids_and_the_repaired_call_keeps_them(bits):
    v, seed = dying_case(bits)
    iters = 2 if bits == 16 else 3
    cb, _, empty = train(v, seed, iters)
    assert empty > 0 and np.isnan(cb).any()                                  # the parent's behaviour
    cb, codes, empty, repaired = train(v, seed, iters, repair=True)
    assert empty == 0 and np.isfinite(cb).all() and repaired > 0             # fails without the feature
    assert (prc.counts(codes, seed.shape[0], bits) > 0).all()                # the returned codes use every centroid


def raw(name, v, seed, *args):
    """a C entry point called directly: -> (codebooks, codes, empty)"""
    L = pyqadc.lib()
    nsq, K, ds = seed.shape
    bits = {16: 4, 256: 8, 65536: 16}[K]
    cb = seed.copy()
    codes = np.zeros((len(v), nsq // 2 if bits == 4 else nsq), "<u2" if bits == 16 else np.uint8)
    empty = C.c_uint64(0)
    head = (v.ctypes.data_as(F32P), len(v), v.shape[1], nsq) + ((bits,) if bits != 16 else ())
    rc = getattr(L, name)(*head, 0, None, None, cb.ctypes.data_as(F32P), *args[:1], codes.ctypes.data_as(C.c_void_p), C.byref(empty), 1, 1,
                          *args[1:], 0)
    assert rc == 0, L.qadc_last_error()
    return cb, codes.astype(np.uint16, copy=False) if bits == 16 else codes, empty.value


@path_independent
@pytest.mark.parametrize("bits", [4, 8, 16])
def test_repair_0_through_the_new_entry_points_is_the_old_call(bits):
    v, seed = prc.train_case(*{4: (16, 4, 32, 300), 8: (4, 8, 8, 700), 16: (2, 16, 4, 300)}[bits], "repeated")
    stem = "qadc_pq_train16" if bits == 16 else "qadc_pq_train"
    old = raw(stem + "_host", v, seed, 2)
    repaired = C.c_uint64(77)
    new = raw(stem + "_repair_host", v, seed, 2, 0, C.byref(repaired))
    same(new, old, "repair = 0")
    assert repaired.value == 0
    same(train(v, seed, 2), old, "the binding")
    assert np.isnan(old[0]).any()                                            # (the case has clusters to lose)


@path_independent
def test_opq_repair_0_is_the_old_call_and_repair_1_is_the_loop_of_the_repaired_calls():
    nsq, bits, dim, n = 8, 8, 16, 3000
    v, seed = prc.train_case(nsq, bits, dim, n, "repeated")
    rot0 = ac.random_rotation(np.random.default_rng(3), dim)
    plain = pyqadc.train_opq(v, seed, 2, 2, rotation=rot0)
    assert len(plain) == 5
    got = pyqadc.train_opq(v, seed, 2, 2, rotation=rot0, repair=True)
    # the loop of include/qadc.h written with the public calls, now the repaired ones
    rot, cb, done, total = rot0.copy(), seed.copy(), 0, 0
    for _ in range(2):
        cb, codes, _, moved = pyqadc.train_pq(v, cb, 2, rotation=rot, repair=True)
        total += moved
        M = pyqadc.opq_cross(v, codes, cb)
        assert np.isfinite(M).all()
        rot = pyqadc.procrustes(M)[0]
        done += 1
    cb, codes, empty, moved = pyqadc.train_pq(v, cb, 2, rotation=rot, repair=True)
    ac.assert_same_floats(got[0], rot, "rotation")
    ac.assert_same_floats(got[1], cb, "codebooks")
    assert np.array_equal(got[2], codes) and got[3:] == (empty, done, total + moved)
    assert got[5] > 0 and got[3] < plain[3]
    # the old entry point is the new one with repair = 0
    L = pyqadc.lib()
    out = []
    for name, tail in (("qadc_opq_train_host", ()), ("qadc_opq_train_repair_host", (0, None))):
        r, c = rot0.copy(), seed.copy()
        k = np.zeros((n, nsq), np.uint8)
        e, d = C.c_uint64(0), C.c_int32(0)
        assert getattr(L, name)(v.ctypes.data_as(F32P), n, dim, nsq, bits, 0, None, r.ctypes.data_as(F32P), c.ctypes.data_as(F32P), 2, 2,
                                k.ctypes.data_as(C.c_void_p), C.byref(e), C.byref(d), 1, 1, *tail, 0) == 0, L.qadc_last_error()
        out.append((r, c, k, e.value, d.value))
    for a, b, p in zip(out[0], out[1], plain):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes() and np.asarray(a).tobytes() == np.asarray(p).astype(np.asarray(a).dtype).tobytes()


@path_independent
@pytest.mark.parametrize("bits", [4, 8, 16])
def test_device_forms_equal_host_forms(bits):
    torch = pytest.importorskip("torch")
    v, seed = prc.train_case(*{4: (16, 4, 32, 300), 8: (4, 8, 8, 700), 16: (2, 16, 4, 300)}[bits], "nan")
    t = torch.from_numpy(v).cuda()
    want = train(v, seed, 2, repair=True)
    got = (pyqadc.train_pq16_device if bits == 16 else pyqadc.train_pq_device)(t, seed, 2, repair=True)
    same(got, want, "device form")
    assert torch.equal(t.cpu(), torch.from_numpy(v))
    if bits == 8:
        rot = np.eye(v.shape[1], dtype=np.float32)
        a, b = pyqadc.train_opq(v, seed, 1, 1, rotation=rot, repair=True), pyqadc.train_opq_device(t, seed, 1, 1, rotation=rot, repair=True)
        ac.assert_same_floats(a[0], b[0])
        ac.assert_same_floats(a[1], b[1])
        assert np.array_equal(a[2], b[2]) and a[3:] == b[3:]


@path_independent
def test_the_same_call_twice_and_a_good_call_after_a_refused_one():
    v, seed = prc.train_case(4, 8, 8, 700, "repeated")
    first = train(v, seed, 3, repair=True)
    L = pyqadc.lib()
    repaired = C.c_uint64(5)
    cb = seed.copy()
    rc = L.qadc_pq_train_repair_host(v.ctypes.data_as(F32P), len(v), 8, 4, 8, 0, None, None, cb.ctypes.data_as(F32P), 3, None, None, 1, 1, 2,
                                     C.byref(repaired), 0)
    assert rc == pyqadc.QADC_E_ARG and b"repair" in L.qadc_last_error() and repaired.value == 5 and np.array_equal(cb, seed)
    with pytest.raises(pyqadc.QadcError):
        train(v[:, :7], seed, 3, repair=True)
    same(train(v, seed, 3, repair=True), first, "again")
