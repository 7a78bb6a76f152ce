"""db_add into a float-ADC index from C++14 (quick-adc_amd/host/db_build.hpp: db_add_hip(qadc_adc_index*, ...);
tests/cpp/adc_db_add_demo.cpp): a .fvecs file streamed through io::vectors_reader with a chunk size that does not divide its
length leaves the partitions pyqadc.AdcIndex.add_vectors leaves for the same array — codes and labels, compared for equality."""
import os
import subprocess

import numpy as np
import pytest

from helpers import path_independent
from test_gpu_adc_add import Quantizers, assert_partitions, read_all
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "cpp", "adc_db_add_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(DEMO + ".cpp", DEMO)
    return DEMO


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("nsq,bits,dim,K,opq", [(8, 8, 64, 8, 1), (2, 16, 16, 8, 0), (4, 8, 16, 0, 0)], ids=["8x8-ivf-opq", "2x16-ivf", "4x8-flat"])
def test_db_add_hip_streams_a_file_into_the_index(demo, tmp_path, nsq, bits, dim, K, opq):
    n, chunk = 1000, 300                                                         # chunks of 300, 300, 300 and 100
    q = Quantizers(nsq, bits, dim, K=K, n=n, seed=10)
    base, quant, out = (str(tmp_path / name) for name in ("base.fvecs", "quantizers.bin", "partitions.bin"))
    rows = np.zeros((n, dim + 1), np.float32)
    rows[:, 0] = np.array([dim], np.int32).view(np.float32)[0]
    rows[:, 1:] = q.vectors
    rows.tofile(base)
    with open(quant, "wb") as f:
        np.array([nsq, bits, dim, K, opq], np.int32).tofile(f)
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
            codes = np.fromfile(f, np.uint8, size * nsq * bits // 8)
            codes = codes.reshape(size, nsq) if bits == 8 else codes.view("<u2").astype(np.uint16).reshape(size, nsq)
            got.append((codes, np.fromfile(f, np.uint32, size) if labelled else None))
        assert f.read() == b""
    idx = q.index(opq=bool(opq), coarse=K > 0)
    try:
        idx.add_vectors(q.vectors)
        assert_partitions(got, read_all(idx))
        assert sum(len(c) for c, _ in got) == n and len(got) == max(K, 1)
    finally:
        idx.close()
