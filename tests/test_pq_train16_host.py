"""CPU: PQ training for 16-bit sub-quantizers without a GPU.

1. The host twins of qadc_pq_train16_host / qadc_pq_update16_host (quick-adc_amd/host/db_build.hpp: pq_train16_iterations,
   pq_update16; driver tests/cpp/pq_train16_host.cpp) against the numpy / oracle expectation of tests/pq_train16_compose.py, bit
   for bit.
2. The geometry of the sorted update (host/pq_train16_plan.hpp) for every sub-vector size the 16-bit encoder admits: the groups
   of a workgroup fit its launch bounds, the grid deals out every unit, every component of a cluster is owned by exactly one lane.
3. The argument refusals of the three C entry points, which come before the first HIP call.
4. The driver, stand-alone, under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adc_compose as ac
import pq_train16_compose as p16
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pq_train16_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "pq_train16_host")
K16 = 65536


@pytest.fixture(scope="module")
def driver():
    _compile(SRC, EXE, link=False)
    return EXE


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pyqadc


def run_twin(exe, tmp_path, v, seed, iters, div_mode=1, coarse=None, rotation=None):
    nsq = seed.shape[0]
    n, dim = v.shape
    fin, fout = str(tmp_path / "train16.in"), str(tmp_path / "train16.out")
    with open(fin, "wb") as f:
        np.array([n, dim, nsq, 0 if coarse is None else len(coarse), rotation is not None, iters, div_mode], np.int32).tofile(f)
        np.ascontiguousarray(v, np.float32).tofile(f)
        np.ascontiguousarray(seed, np.float32).tofile(f)
        if coarse is not None:
            np.ascontiguousarray(coarse, np.float32).tofile(f)
        if rotation is not None:
            np.ascontiguousarray(rotation, np.float32).tofile(f)
    out = subprocess.run([exe, "run", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    with open(fout, "rb") as f:
        cb = np.fromfile(f, np.float32, seed.size).reshape(seed.shape)
        codes = np.fromfile(f, "<u2", n * nsq if iters > 0 else 0).reshape(-1, nsq)
        empty = int(np.fromfile(f, np.uint64, 1)[0])
        assert f.read() == b""
    return cb, codes, empty


def run_update(exe, tmp_path, v, codes, div_mode=1):
    n, dim = v.shape
    nsq = codes.shape[1]
    fin, fout = str(tmp_path / "update16.in"), str(tmp_path / "update16.out")
    with open(fin, "wb") as f:
        np.array([n, dim, nsq, div_mode], np.int32).tofile(f)
        np.ascontiguousarray(v, np.float32).tofile(f)
        np.ascontiguousarray(codes, "<u2").tofile(f)
    out = subprocess.run([exe, "update", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    with open(fout, "rb") as f:
        cb = np.fromfile(f, np.float32, dim * K16).reshape(nsq, K16, dim // nsq)
        counts = np.fromfile(f, np.uint32, nsq * K16).reshape(nsq, K16)
        assert f.read() == b""
    return cb, counts


SHAPES = {"2x16-d4": (2, 4, 300), "8x16-d16": (8, 16, 200)}


def make(nsq, dim, n, seed=0):
    rng = np.random.default_rng([nsq, dim, n, seed])
    return rng, rng.normal(size=(n, dim)).astype(np.float32), rng.normal(size=(nsq, K16, dim // nsq)).astype(np.float32)


@pytest.mark.parametrize("div_mode", [1, 0])
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_twin_matches_the_compose_helper(driver, po, tmp_path, shape, iters, div_mode):
    _, v, seed = make(*SHAPES[shape])
    want_cb, want_codes, _ = p16.train(po, v, seed, iters, div_mode)
    got_cb, got_codes, empty = run_twin(driver, tmp_path, v, seed, iters, div_mode)
    ac.assert_same_floats(got_cb, want_cb, "codebooks after %d rounds" % iters)
    assert np.array_equal(got_codes, want_codes)
    assert empty == p16.empty_count(want_cb) > 0                 # (fewer vectors than centroids: most clusters are empty)


def test_twin_trains_on_the_rotated_residual(driver, po, tmp_path):
    nsq, dim, n = SHAPES["2x16-d4"]
    rng, v, seed = make(nsq, dim, n, seed=1)
    coarse = v[rng.choice(n, 20, replace=False)].copy()
    rot = ac.random_rotation(rng, dim)
    x = ac.residuals(v, coarse, ac.assign(po, v, coarse, 1), rot)[:, 0, :]
    want_cb, want_codes, _ = p16.train(po, x, seed, 2)
    got_cb, got_codes, empty = run_twin(driver, tmp_path, v, seed, 2, coarse=coarse, rotation=rot)
    ac.assert_same_floats(got_cb, want_cb)
    assert np.array_equal(got_codes, want_codes) and empty == p16.empty_count(want_cb)


def test_twin_zero_rounds_leave_the_seed_and_write_no_code(driver, tmp_path):
    _, v, seed = make(*SHAPES["2x16-d4"])
    seed[1, 7, 0] = np.nan
    cb, codes, empty = run_twin(driver, tmp_path, v, seed, 0)
    assert np.array_equal(cb.view(np.uint32), seed.view(np.uint32)) and codes.size == 0 and empty == 1


@pytest.mark.parametrize("div_mode", [1, 0])
def test_update_twin_matches_the_compose_update_in_ascending_order_only(driver, tmp_path, div_mode):
    rng = np.random.default_rng(3)
    n, nsq, dim = 3000, 2, 6
    v = rng.normal(size=(n, dim)).astype(np.float32)
    v[rng.random(n) < 0.2] *= np.float32(1e8)                    # mixed magnitude: the order of a sum shows
    codes = rng.choice(np.array([0, 1, 255, 256, 257, 65280, 65535], np.uint16), size=(n, nsq))
    want_cb, want_counts = p16.update(v, codes, div_mode)
    other = p16.update(v, codes, div_mode, descending=True)[0]
    assert not np.array_equal(want_cb.view(np.uint32), other.view(np.uint32))
    cb, counts = run_update(driver, tmp_path, v, codes, div_mode)
    ac.assert_same_floats(cb, want_cb)
    assert np.array_equal(counts, want_counts) and int(counts.sum()) == n * nsq


def _parse(line):
    return None if line == "refused" else dict((k, int(x)) for k, x in (t.split("=") for t in line.split()))


def plans(exe, nsq, dmax):
    out = subprocess.run([exe, "plans", str(nsq), str(dmax)], stdout=subprocess.PIPE, timeout=300).stdout.decode().splitlines()
    assert len(out) == dmax
    return [_parse(l.strip()) for l in out]


def test_update_geometry_fits_for_every_sub_vector_size(driver):
    """every dsub the 16-bit encoder admits: dim <= 4096 on 2, 4 and 8 sub-quantizers"""
    widths = set()
    for nsq, dmax in ((2, 2048), (4, 1024), (8, 512)):
        for ds, p in enumerate(plans(driver, nsq, dmax), 1):
            assert p is not None, (nsq, ds)
            assert p["wg"] == 256 and p["dsub"] == ds and p["width"] == min(ds, 64)
            assert p["wave_groups"] == 64 // p["width"] and p["wave_groups"] * p["width"] <= 64          # whole groups per wave
            assert p["wg_groups"] == 4 * p["wave_groups"] and p["wg_groups"] * p["width"] <= p["wg"]    # the launch bounds hold them
            assert p["width"] * p["dblocks"] >= ds > p["width"] * (p["dblocks"] - 1)
            assert p["units"] == K16 * p["dblocks"]
            assert p["grid"] * p["wg_groups"] >= p["units"] > (p["grid"] - 1) * p["wg_groups"]          # every unit dealt, no idle workgroup
            assert p["owned_min"] == p["owned_max"] == 1 and p["stray"] == 0                             # each component exactly once
            assert p["lds"] == 4 * (256 + 4 * 256) <= 48 * 1024
            widths.add(p["width"])
    assert widths == set(range(1, 65))
    assert plans(driver, 2, 2049)[-1] is None and plans(driver, 3, 1)[0] is None and plans(driver, 16, 1)[0] is None


F32P = C.POINTER(C.c_float)


def _call(fn, vectors=1, n=100, dim=32, nsq=4, K=0, coarse=None, cb=1, iters=1, codes=1, div_mode=1, sum_mode=1):
    """host memory only: the device form is handed a host pointer it must not touch"""
    v = np.zeros((100, 64), np.float32)
    c = np.zeros(65536, np.float32)
    k = np.zeros(1024, np.uint16)
    name = fn.__name__
    vp = (v.ctypes.data_as(C.c_void_p) if name.endswith("device") else v.ctypes.data_as(F32P)) if vectors else None
    cbp = c.ctypes.data_as(F32P) if cb else None
    if "update16" in name:
        return fn(vp, n, dim, nsq, k.ctypes.data_as(C.c_void_p) if codes else None, cbp, None, div_mode, 0)
    return fn(vp, n, dim, nsq, K, coarse, None, cbp, iters, None, None, div_mode, sum_mode, 0)


@pytest.mark.parametrize("entry", ["qadc_pq_train16_host", "qadc_pq_train16_device", "qadc_pq_update16_host"])
def test_argument_refusals_come_before_any_hip_call(pyqadc, entry):
    lib = pyqadc.lib()
    fn = getattr(lib, entry)
    some = np.zeros(64, np.float32).ctypes.data_as(F32P)

    def refused(needle, **kw):
        assert _call(fn, **kw) == pyqadc.QADC_E_ARG, kw
        assert needle in lib.qadc_last_error().decode(), (kw, lib.qadc_last_error())

    for nsq in (0, 1, 3, 16, -2):
        refused("sq_count must be 2, 4 or 8", nsq=nsq, dim=48)
    refused("multiple of sq_count", dim=33)
    refused("multiple of sq_count", dim=0)
    refused("<= 4096", dim=4096 + 4)
    refused("NULL", vectors=0)
    refused("NULL", cb=0)
    refused("0 < n < 2^32", n=0)
    refused("0 < n < 2^32", n=2 ** 32)
    refused("div_mode", div_mode=2)
    refused("div_mode", div_mode=-1)
    if "update16" in entry:
        refused("codes must not be NULL", codes=0)
        return
    refused("iters", iters=-1)
    refused("coarse", K=20, coarse=None)
    refused("K_coarse", K=-1, coarse=some)
    refused("sum_mode", sum_mode=2)
    refused("sum_mode", sum_mode=-1)
    # zero rounds: the seed's bits stay, no code is written, no device is involved
    cb = np.arange(2 * K16 * 2, dtype=np.float32)
    cb[5] = np.nan
    keep = cb.copy()
    v = np.zeros((10, 4), np.float32)
    codes = np.full((10, 2), 0xABCD, np.uint16)
    empty = C.c_uint64(7)
    vp = v.ctypes.data_as(C.c_void_p) if entry.endswith("device") else v.ctypes.data_as(F32P)
    assert fn(vp, 10, 4, 2, 0, None, None, cb.ctypes.data_as(F32P), 0, codes.ctypes.data_as(C.c_void_p), C.byref(empty), 1, 1, 0) == 0
    assert np.array_equal(cb.view(np.uint32), keep.view(np.uint32)) and empty.value == 1 and (codes == 0xABCD).all()


def test_python_front_refuses_bad_shapes(pyqadc):
    v = np.zeros((10, 8), np.float32)
    with pytest.raises(pyqadc.QadcError, match="65536"):
        pyqadc.train_pq16(v, np.zeros((2, 256, 4), np.float32), 1)            # an 8-bit seed
    with pytest.raises(pyqadc.QadcError):
        pyqadc.train_pq16(v, np.zeros((2, K16, 3), np.float32), 1)            # 6 columns for 8
    with pytest.raises(pyqadc.QadcError):
        pyqadc.pq_update16(v, np.zeros((10, 4), np.uint16), 2)                # codes of another shape
    with pytest.raises(pyqadc.QadcError):
        pyqadc.pq_update16(v, np.zeros((10, 3), np.uint16), 3)                # 8 columns on 3 sub-quantizers
    cb, codes, empty = pyqadc.train_pq16(v, np.ones((2, K16, 4), np.float32), 0)
    assert (cb == 1).all() and codes.shape == (10, 2) and codes.dtype == np.uint16 and empty == 0


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(driver, po, tmp_path):
    """both twins and the plans, stand-alone, built with -fsanitize=address,undefined: the same bits, no report"""
    exe = str(tmp_path / "pq_train16_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           SRC, "-o", exe])
    rng, v, seed = make(2, 4, 40, seed=9)
    coarse = v[:5].copy()
    plain = run_twin(driver, tmp_path, v, seed, 1, coarse=coarse, rotation=ac.random_rotation(np.random.default_rng(1), 4))
    asan = run_twin(exe, tmp_path, v, seed, 1, coarse=coarse, rotation=ac.random_rotation(np.random.default_rng(1), 4))
    ac.assert_same_floats(asan[0], plain[0])
    assert np.array_equal(asan[1], plain[1]) and asan[2] == plain[2]
    codes = rng.integers(0, K16, (40, 2)).astype(np.uint16)
    codes[0] = (0, 65535)
    a, b = run_update(exe, tmp_path, v, codes), run_update(driver, tmp_path, v, codes)
    ac.assert_same_floats(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert plans(exe, 2, 130) == plans(driver, 2, 130)
