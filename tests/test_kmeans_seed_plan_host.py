"""CPU: the geometry of the k-means++ seeding kernels (quick-adc_amd/host/kmeans_seed_plan.hpp; driver
tests/cpp/kmeans_seed_plan_host.cpp): every row is owned by one lane of one workgroup, the kernel's walk over the columns closes every
sub-space where it ends for every (sq_count, dim) the call admits, the LDS fits, the tree's node counts are right at its edges — and
every refusal, in the plan and through the C-ABI in a process that never opens a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "kmeans_seed_plan_host")


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "kmeans_seed_plan_host.cpp"), EXE, link=False)
    return EXE


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pyqadc


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, timeout=300)
    assert out.returncode == 0
    return out.stdout.decode().strip()


def plan(exe, n, dim, sq_count, k):
    line = run(exe, "plan", n, dim, sq_count, k)
    return line if line.startswith("refused") else dict((key, int(x)) for key, x in (t.split("=") for t in line.split()))


def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 77, 64 ** 3 + 1])
def test_every_row_has_one_owner(driver, n):
    assert run(driver, "rows", n) == "owned=1"


def test_every_admitted_shape_walks_its_columns_and_fits(driver):
    line = dict((key, int(x)) for key, x in (t.split("=") for t in run(driver, "sweep", 100000).split()))
    assert line["shapes"] == sum(4096 // s for s in range(1, 33))
    assert line["ok"] == 1 and line["max_lds"] == 4 * (4 * 64 * 33 + 4096) <= 64 * 1024


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 64 ** 3 - 1, 64 ** 3, 64 ** 3 + 1, 2 ** 32 - 1])
def test_node_counts(driver, n):
    p = plan(driver, n, 128, 16, 1)
    counts = [ceil_div(n, 64 ** level) for level in range(7)]
    root = max(2, next(level for level in range(7) if counts[level] == 1))
    assert p["root_level"] == root
    assert [p["nodes%d" % level] for level in range(7)] == [c if level <= root else 0 for level, c in enumerate(counts)]
    assert p["nodes%d" % root] == 1
    assert p["update_grid"] == counts[2] and p["pick_grid"] == 16 and p["wg"] == 256 and p["rows_per_wg"] == 4096
    assert p["upper_nodes"] == sum(counts[3:root + 1])
    offset = 0
    for level in range(3, 7):
        assert p["offset%d" % level] == offset
        offset += p["nodes%d" % level]
    assert p["bitmap_words"] == ceil_div(n, 32)
    tree = counts[1] + counts[2] + p["upper_nodes"]
    assert p["scratch_bytes"] == 16 * (4 * n + 8 * tree + 4 * p["bitmap_words"] + 12 + 8 * 4 + 4)      # k = 1, dsub = 8


def test_plan_refusals(driver):
    def why(*a):
        line = plan(driver, *a)
        assert isinstance(line, str), a
        return line
    assert "0 < n < 2^32" in why(0, 8, 1, 1) and "0 < n < 2^32" in why(2 ** 32, 8, 1, 1)
    assert "1 <= k <= n" in why(10, 8, 1, 0) and "1 <= k <= n" in why(10, 8, 1, 11) and "1 <= k <= n" in why(10, 8, 1, -3)
    assert "sq_count must be in [1, 32]" in why(10, 8, 0, 1) and "sq_count must be in [1, 32]" in why(10, 66, 33, 1)
    assert "multiple of sq_count" in why(10, 9, 2, 1) and "multiple of sq_count" in why(10, 0, 1, 1) and "multiple of sq_count" in why(10, -8, 2, 1)
    assert "dim must be <= 4096" in why(10, 4097, 1, 1) and "dim must be <= 4096" in why(10, 4128, 32, 1)
    for a in ((10, 4096, 1, 10), (10, 4096, 32, 1), (2 ** 32 - 1, 1, 1, 2 ** 32 - 1), (1, 32, 32, 1)):
        assert isinstance(plan(driver, *a), dict), a


def test_c_abi_refusals_come_before_any_device(pyqadc):
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    v = np.ones((10, 8), np.float32)
    centres, rows, fb = np.full((2, 3, 4), 7.0, np.float32), np.full((2, 3), 9, np.uint32), C.c_uint64(5)
    vp, cp, rp = v.ctypes.data_as(f32p), centres.ctypes.data_as(f32p), rows.ctypes.data_as(u32p)

    def refused(message, vectors=vp, n=10, dim=8, sq_count=2, k=3, K_coarse=0, coarse=None, out=cp):
        for name in ("qadc_kmeans_seed_host", "qadc_kmeans_seed_device"):
            vec = vectors if name.endswith("host") or vectors is None else C.cast(vectors, C.c_void_p)
            rc = getattr(L, name)(vec, n, dim, sq_count, k, K_coarse, coarse, None, 1, out, rp, C.byref(fb), 0)
            assert rc == E and message in L.qadc_last_error().decode(), (name, message, L.qadc_last_error())

    refused("vectors must not be NULL", vectors=None)
    refused("centres_out must not be NULL", out=None)
    refused("0 < n < 2^32", n=0)
    refused("0 < n < 2^32", n=2 ** 32)
    refused("1 <= k <= n", k=0)
    refused("1 <= k <= n", k=-1)
    refused("1 <= k <= n", k=11)
    refused("sq_count must be in [1, 32]", sq_count=0)
    refused("sq_count must be in [1, 32]", sq_count=33, dim=66)
    refused("multiple of sq_count", dim=9)
    refused("multiple of sq_count", dim=0)
    refused("dim must be <= 4096", dim=4098)
    refused("K_coarse", K_coarse=-1)
    refused("K_coarse", K_coarse=2)
    rc = L.qadc_kmeans_seed_device(C.c_void_p(v.ctypes.data + 2), 10, 8, 2, 3, 0, None, None, 1, cp, rp, C.byref(fb), 0)
    assert rc == E and b"d_vectors must be 4-byte aligned" in L.qadc_last_error()
    assert (centres == 7.0).all() and (rows == 9).all() and fb.value == 5                     # a refused call writes nothing


def test_python_wrappers_refuse_without_a_device(pyqadc):
    v = np.ones((10, 8), np.float32)
    for kw, message in ((dict(k=0), "1 <= k <= n"), (dict(k=11), "1 <= k <= n"), (dict(k=2, sq_count=3), "multiple of sq_count"),
                        (dict(k=2, seed=-1), "seed must be"), (dict(k=2, seed=2 ** 64), "seed must be"),
                        (dict(k=2, rotation=np.eye(4)), "rotation has shape"), (dict(k=2, coarse=np.ones((2, 4))), "coarse has shape")):
        with pytest.raises(pyqadc.QadcError, match=message):
            pyqadc.kmeans_seed(v, **kw)
    with pytest.raises(pyqadc.QadcError, match="expected \\[n\\]\\[dim\\]"):
        pyqadc.kmeans_seed(np.ones(8, np.float32), 1)
    with pytest.raises(pyqadc.QadcError, match="sq_count must be in"):
        pyqadc.kmeans_seed(np.ones((10, 66), np.float32), 2, sq_count=33)
