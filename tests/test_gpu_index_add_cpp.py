"""db_add into the 4-bit index from C++14 (quick-adc_amd/host/db_build.hpp: db_add_hip(qadc_index*, ...);
tests/cpp/db_add4_demo.cpp): a .fvecs file streamed through io::vectors_reader with a chunk size that does not divide its length
leaves the partitions pyqadc.Index.add_vectors leaves for the same array — codes and labels, compared for equality."""
import os
import subprocess

import numpy as np
import pytest

from helpers import path_independent
from test_gpu_adc_add import assert_partitions, read_all
from test_gpu_index_add import Quantizers4
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "cpp", "db_add4_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(DEMO + ".cpp", DEMO)
    return DEMO


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("M,dim,K,opq", [(16, 32, 8, 1), (32, 64, 0, 0)], ids=["16x4-ivf-opq", "32x4-flat"])
def test_db_add_hip_streams_a_file_into_the_index(demo, tmp_path, M, dim, K, opq):
    n, chunk = 1000, 300                                                         # chunks of 300, 300, 300 and 100
    q = Quantizers4(M, dim, K=K, n=n, seed=10)
    base, quant, out = (str(tmp_path / name) for name in ("base.fvecs", "quantizers.bin", "partitions.bin"))
    rows = np.zeros((n, dim + 1), np.float32)
    rows[:, 0] = np.array([dim], np.int32).view(np.float32)[0]
    rows[:, 1:] = q.vectors
    rows.tofile(base)
    with open(quant, "wb") as f:
        np.array([M, 4, dim, K, opq], np.int32).tofile(f)
        q.codebooks.tofile(f)
        if K:
            q.coarse.tofile(f)
        if opq:
            q.rotation.tofile(f)
    run = subprocess.run([demo, quant, base, str(chunk), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    assert run.stdout.decode().strip() == "ok %d" % n
    got = []
    with open(out, "rb") as f:
        parts, labelled = (int(x) for x in np.fromfile(f, np.int32, 2))
        for _ in range(parts):
            size = int(np.fromfile(f, np.uint32, 1)[0])
            codes = np.fromfile(f, np.uint8, size * M // 2).reshape(size, M // 2)
            got.append((codes, np.fromfile(f, np.uint32, size) if labelled else None))
        assert f.read() == b""
    idx = q.index(opq=bool(opq), coarse=K > 0)
    try:
        idx.add_vectors(q.vectors)
        assert_partitions(got, read_all(idx))
        assert sum(len(c) for c, _ in got) == n and len(got) == max(K, 1)
    finally:
        idx.close()
