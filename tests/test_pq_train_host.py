"""CPU: PQ training without a GPU.

1. The host twin of qadc_pq_train_host (quick-adc_amd/host/db_build.hpp: pq_train_iterations, driver tests/cpp/pq_train_host.cpp)
   against the numpy / oracle expectation of tests/pq_train_compose.py, bit for bit; where the reference's own loops are compiled
   (oracle/_ref), the update of every slice also equals them.
2. The geometry of the update kernel (host/pq_train_plan.hpp) for every sub-vector size the encoders admit: the chains of a
   workgroup fit its launch bounds, its staged window fits the registers that prefetch it and the LDS, every chain is owned once.
3. The argument refusals of both C entry points, which come before the first HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adc_compose as ac
import pq_train_compose as ptc
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "pq_train_host")


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "pq_train_host.cpp"), EXE, link=False)
    return EXE


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pyqadc


def run_twin(exe, tmp_path, v, seed, iters, div_mode=1, coarse=None, rotation=None):
    nsq, K, ds = seed.shape
    bits = {16: 4, 256: 8}[K]
    n, dim = v.shape
    fin, fout = str(tmp_path / "train.in"), str(tmp_path / "train.out")
    with open(fin, "wb") as f:
        np.array([n, dim, nsq, bits, 0 if coarse is None else len(coarse), rotation is not None, iters, div_mode], np.int32).tofile(f)
        np.ascontiguousarray(v, np.float32).tofile(f)
        np.ascontiguousarray(seed, np.float32).tofile(f)
        if coarse is not None:
            np.ascontiguousarray(coarse, np.float32).tofile(f)
        if rotation is not None:
            np.ascontiguousarray(rotation, np.float32).tofile(f)
    out = subprocess.run([exe, "run", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    with open(fout, "rb") as f:
        cb = np.fromfile(f, np.float32, seed.size).reshape(seed.shape)
        codes = np.fromfile(f, np.uint8, n * (nsq // 2 if bits == 4 else nsq)).reshape(n, -1)
        empty = int(np.fromfile(f, np.uint64, 1)[0])
        assert f.read() == b""
    return cb, codes, empty


@pytest.mark.parametrize("nsq,bits,dim,n", [(16, 4, 32, 700), (32, 4, 96, 500), (4, 8, 32, 1500), (8, 8, 24, 1200)],
                         ids=["16x4-d32", "32x4-d96", "4x8-d32", "8x8-d24"])
@pytest.mark.parametrize("div_mode", [1, 0])
def test_twin_matches_the_oracle_loop(driver, po, tmp_path, nsq, bits, dim, n, div_mode):
    rng = np.random.default_rng(100 * nsq + dim + div_mode)
    v = rng.normal(size=(n, dim)).astype(np.float32)
    seed = ptc.seed_rows(v, nsq, bits, rng.choice(n, 1 << bits, replace=False))
    for iters in (1, 3):
        want_cb, want_codes, before = ptc.train(po, v, seed, iters, div_mode)
        got_cb, got_codes, empty = run_twin(driver, tmp_path, v, seed, iters, div_mode)
        ac.assert_same_floats(got_cb, want_cb, "codebooks after %d rounds" % iters)
        assert np.array_equal(got_codes, want_codes)
        assert empty == ptc.empty_count(want_cb)
    # the update of every slice is the reference's own loops as compiled (they multiply by the reciprocal: div_mode 1)
    if div_mode == 1 and po.have_ref_float():
        ds, a = dim // nsq, ptc.unpack(want_codes, bits)
        for m in range(nsq):
            sub = np.ascontiguousarray(v[:, m * ds:(m + 1) * ds])
            ac.assert_same_floats(po.reff_kmeans_update(sub, a[:, m].astype(np.int32), 1 << bits), want_cb[m], "slice %d" % m)


def test_twin_zero_rounds_and_an_empty_cluster(driver, po, tmp_path):
    rng = np.random.default_rng(5)
    n, nsq, bits, dim = 400, 16, 4, 32
    v = rng.normal(size=(n, dim)).astype(np.float32)
    seed = ptc.seed_rows(v, nsq, bits, rng.choice(n, 16, replace=False))
    cb, _, empty = run_twin(driver, tmp_path, v, seed, 0)
    assert np.array_equal(cb.view(np.uint32), seed.view(np.uint32)) and empty == 0
    seed[3, 1] = seed[3, 0]                                    # centroid 1 of sub-quantizer 3 never wins: an equal distance does not replace
    assert np.isnan(ptc.train(po, v, seed, 1)[0][3, 1]).all()
    want_cb, want_codes, _ = ptc.train(po, v, seed, 3)
    assert np.isnan(want_cb[3, 1]).all() and ptc.empty_count(want_cb) >= 1
    got_cb, got_codes, empty = run_twin(driver, tmp_path, v, seed, 3)
    ac.assert_same_floats(got_cb, want_cb)
    assert np.array_equal(got_codes, want_codes) and empty == ptc.empty_count(want_cb)


@pytest.mark.parametrize("opq", [False, True], ids=["residual", "residual-opq"])
def test_twin_trains_on_the_rotated_residual(driver, po, tmp_path, opq):
    rng = np.random.default_rng(8 + opq)
    n, nsq, bits, dim, K = 600, 16, 4, 32, 20
    v = rng.normal(size=(n, dim)).astype(np.float32)
    coarse = v[rng.choice(n, K, replace=False)].copy()
    rot = ac.random_rotation(rng, dim) if opq else None
    x = ac.residuals(v, coarse, ac.assign(po, v, coarse, 1), rot)[:, 0, :]
    seed = ptc.seed_rows(x, nsq, bits, rng.choice(n, 16, replace=False))
    want_cb, want_codes, _ = ptc.train(po, x, seed, 2)
    got_cb, got_codes, _ = run_twin(driver, tmp_path, v, seed, 2, coarse=coarse, rotation=rot)
    ac.assert_same_floats(got_cb, want_cb)
    assert np.array_equal(got_codes, want_codes)


def _parse(line):
    return None if line == "refused" else dict((k, int(x)) for k, x in (t.split("=") for t in line.split()))


def plan(exe, nsq, bits, dim):
    return _parse(subprocess.run([exe, "plan", str(nsq), str(bits), str(dim)], stdout=subprocess.PIPE, timeout=60).stdout.decode().strip())


def plans(exe, nsq, bits, dmax):
    """the plan of every dim = nsq * dsub, dsub = 1 .. dmax"""
    out = subprocess.run([exe, "plans", str(nsq), str(bits), str(dmax)], stdout=subprocess.PIPE, timeout=60).stdout.decode().splitlines()
    assert len(out) == dmax
    return [_parse(l.strip()) for l in out]


def test_update_kernel_geometry_fits_for_every_sub_vector_size(driver):
    """every dsub up to the encoders' limits (4 bits: dim <= 2048 on 16 sub-quantizers; 8 bits: dim <= 4096 on 4)"""
    seen_chunks = set()
    for nsq, bits, dmax in ((16, 4, 128), (32, 4, 64), (4, 8, 1024), (8, 8, 512), (16, 8, 256)):
        for ds, p in enumerate(plans(driver, nsq, bits, dmax), 1):
            assert p is not None, (nsq, bits, ds)
            assert p["wg"] == 256 and p["K"] == 1 << bits and p["dsub"] == ds
            assert p["mper"] * p["kper"] * p["width"] <= p["wg"]                              # the launch bounds hold the chains
            assert p["width"] * p["dblocks"] >= ds and p["kper"] * p["kblocks"] >= p["K"] and p["mper"] * p["mblocks"] >= nsq
            assert p["width"] * (p["dblocks"] - 1) < ds and p["kper"] * (p["kblocks"] - 1) < p["K"] and p["mper"] * (p["mblocks"] - 1) < nsq
            assert p["mper"] == 1 or (p["kper"] == p["K"] and p["width"] == ds)               # several sub-quantizers: whole ones
            assert p["cols"] == (p["mper"] * ds if p["mper"] > 1 else p["width"])
            assert 1 <= p["chunk"] <= 256 and p["chunk"] * p["cols"] <= p["stage"] and p["chunk"] * p["mper"] <= p["code_stage"]
            assert p["lds"] == 4 * p["chunk"] * p["cols"] + p["chunk"] * p["mper"] <= 48 * 1024
            assert p["grid"] == p["mblocks"] * p["kblocks"] * p["dblocks"]
            seen_chunks.add(p["chunk"])
    assert seen_chunks == {256, 128, 64, 32, 16}
    assert plan(driver, 4, 8, 4 * 1025) is None and plan(driver, 16, 16, 64) is None and plan(driver, 16, 4, 33) is None


def _train_call(fn, vectors=1, n=100, dim=32, nsq=16, bits=4, K=0, coarse=None, rotation=None, cb=1, iters=1, div_mode=1, sum_mode=1):
    v = np.zeros((100, 64), np.float32)
    c = np.zeros(65536, np.float32)
    f32p = C.POINTER(C.c_float)
    vp = (v.ctypes.data_as(C.c_void_p) if fn.__name__.endswith("device") else v.ctypes.data_as(f32p)) if vectors else None
    return fn(vp, n, dim, nsq, bits, K, coarse, rotation, c.ctypes.data_as(f32p) if cb else None, iters, None, None, div_mode, sum_mode, 0)


@pytest.mark.parametrize("entry", ["qadc_pq_train_host", "qadc_pq_train_device"])
def test_argument_refusals_come_before_any_hip_call(pyqadc, entry):
    """none of these reaches the device: they are refused alike with and without a GPU (the device form is handed a host
    pointer here, which it must not touch)"""
    lib = pyqadc.lib()
    fn = getattr(lib, entry)
    some = np.zeros(64, np.float32).ctypes.data_as(C.POINTER(C.c_float))

    def refused(needle, **kw):
        assert _train_call(fn, **kw) == pyqadc.QADC_E_ARG, kw
        assert needle in lib.qadc_last_error().decode(), (kw, lib.qadc_last_error())

    refused("follow-up", bits=16, nsq=4)
    refused("sq_bits 16", bits=16, nsq=16)
    refused("multiple of sq_count", dim=33)
    refused("sq_count 16 or 32", nsq=8)                          # 4 bits with sq_count 8
    refused("sq_count 4, 8 or 16", bits=8, nsq=32)
    refused("sq_bits must be 4 or 8", bits=5)
    refused("NULL", vectors=0)
    refused("NULL", cb=0)
    refused("coarse", K=20, coarse=None)
    refused("K_coarse", K=-1, coarse=some)
    refused("0 < n < 2^32", n=0)
    refused("0 < n < 2^32", n=2 ** 32)
    refused("iters", iters=-1)
    refused("<= 2048", dim=2048 + 16)
    refused("<= 4096", bits=8, nsq=4, dim=4096 + 4)
    refused("div_mode", div_mode=2)
    refused("sum_mode", sum_mode=-1)
    # zero rounds: the seed untouched, no device involved
    cb = np.arange(16 * 16 * 2, dtype=np.float32)
    keep = cb.copy()
    v = np.zeros((10, 32), np.float32)
    empty = C.c_uint64(7)
    vp = v.ctypes.data_as(C.c_void_p) if entry.endswith("device") else v.ctypes.data_as(C.POINTER(C.c_float))
    assert fn(vp, 10, 32, 16, 4, 0, None, None, cb.ctypes.data_as(C.POINTER(C.c_float)), 0, None, C.byref(empty), 1, 1, 0) == 0
    assert np.array_equal(cb, keep) and empty.value == 0


def test_python_front_refuses_bad_shapes_and_seeds_from_distinct_rows(pyqadc):
    rng = np.random.default_rng(2)
    v = rng.normal(size=(300, 32)).astype(np.float32)
    seed = pyqadc.pq_seed(v, 16, 4, rng)
    assert seed.shape == (16, 16, 2) and seed.dtype == np.float32
    rows = seed.transpose(1, 0, 2).reshape(16, 32)
    idx = [int(np.flatnonzero((v == r).all(axis=1))[0]) for r in rows]
    assert len(set(idx)) == 16                                   # whole rows of the learning set, all distinct
    assert pyqadc.pq_seed(v, 8, 8, rng).shape == (8, 256, 4)
    with pytest.raises(pyqadc.QadcError):
        pyqadc.pq_seed(v[:100], 8, 8, rng)                       # fewer vectors than centroids
    with pytest.raises(pyqadc.QadcError):
        pyqadc.train_pq(v, np.zeros((16, 32, 2), np.float32), 1)  # 32 centroids: no such shape
    with pytest.raises(pyqadc.QadcError):
        pyqadc.train_pq(v, np.zeros((16, 16, 3), np.float32), 1)  # 48 columns for 32
    with pytest.raises(pyqadc.QadcError, match="follow-up"):
        pyqadc.train_pq(v, np.zeros((4, 65536, 8), np.float32), 1)
