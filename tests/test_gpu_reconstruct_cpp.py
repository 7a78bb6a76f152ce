"""reconstruct_hip and pq_decode_hip — the C++14 mirrors of qadc_adc_index_reconstruct and qadc_pq_decode_host
(quick-adc_amd/host/db_build.hpp) — through tests/cpp/reconstruct_demo.cpp: the demo holds the mirrors to the
host twin itself, and what it writes out must equal, bit for bit, what pyqadc.AdcIndex.reconstruct returns on the same data."""
import os
import subprocess

import numpy as np
import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "reconstruct_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
def test_the_demo_equals_the_python_call(demo, tmp_path, rotated):
    import pyqadc
    rng = np.random.default_rng(17)
    dim, nsq, K, n = 24, 8, 5, 3000
    cb = rng.normal(size=(nsq, 256, dim // nsq)).astype(np.float32)
    rot = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(dim, dim)))[0], np.float32)
    coarse = rng.normal(size=(K, dim)).astype(np.float32) * 3
    vec = (coarse[rng.integers(0, K, n)] + rng.normal(size=(n, dim))).astype(np.float32)
    labels = rng.integers(0, 2500, n).astype(np.uint32)                     # repeats
    keys = np.concatenate([labels[:400], np.arange(2500, 2520, dtype=np.uint32), labels[:5]]).astype(np.uint32)
    fin, fout = str(tmp_path / "demo.in"), str(tmp_path / "demo.out")
    with open(fin, "wb") as f:
        np.array([dim, nsq, K, rotated, n, len(keys)], np.int32).tofile(f)
        for a in (cb,) + ((rot,) if rotated else ()) + (coarse, vec, labels, keys):
            a.tofile(f)
    out = subprocess.run([demo, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % len(keys)
    with open(fout, "rb") as f:
        got = np.fromfile(f, np.float32, len(keys) * dim).reshape(len(keys), dim)
        where = np.fromfile(f, np.uint64, len(keys))
        err = np.fromfile(f, np.float32, n)
        assert f.read() == b""
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.set_pq(cb)
    if rotated:
        idx.set_rotation(rot)
    idx.set_coarse(coarse)
    idx.add_vectors(vec, labels=labels)
    want, want_where = idx.reconstruct(keys)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(where, want_where)
    assert (where[400:420] == pyqadc.QADC_RECONSTRUCT_MISSING).all() and (where[:400] != pyqadc.QADC_RECONSTRUCT_MISSING).all()
    rows = np.concatenate([idx.reconstruct_rows(p) for p in range(K)])
    want_err, total = pyqadc.quant_error(np.zeros((n, dim), np.float32),
                                         np.concatenate([np.full(idx.partition_size(p), p, np.int32) for p in range(K)]),
                                         np.concatenate([idx.read_partition(p)[0] for p in range(K)]), cb, coarse=coarse,
                                         rotation=rot if rotated else None)
    assert np.array_equal(err.view(np.uint32), want_err.view(np.uint32)) and total > 0 and len(rows) == n
    idx.close()
