"""The C++14 engine quick-adc_amd/host/adc_search_hip.hpp — nns_engine_batch's contract over qadc_adc_search_candidates, query
vectors in — fills every heap exactly as the CPU path it replaces (nns_engine + scanner_simple over pq_bytes, the host twin) on the
same seeded database (tests/cpp/adc_search_hip_demo.cpp): flat and IVF, plain and OPQ, whole and ragged batches."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_search_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(os.path.join(ROOT, "tests", "cpp", "adc_search_hip_demo.cpp"), EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("M,sq_dim,n,K,ma,nq,R,batch,opq", [
    (8, 16, 40000, 0, 1, 8, 100, 8, 0),           # flat, the direct form
    (8, 16, 20000, 0, 3, 7, 10, 4, 1),            # flat probed three times, OPQ, a ragged last batch
    (8, 16, 60000, 32, 8, 33, 100, 16, 0),        # IVF
    (4, 32, 30000, 16, 16, 9, 1000, 32, 1),       # every partition probed, R large, OPQ
    (16, 8, 30000, 64, 24, 16, 50, 5, 0),
    (8, 12, 20000, 16, 1, 6, 20, 1, 1),           # a sub-vector size outside the register paths, one query per call
])
def test_search_engine_fills_heaps_like_the_cpu_engine(demo, M, sq_dim, n, K, ma, nq, R, batch, opq):
    out = subprocess.run([demo] + [str(v) for v in (M, sq_dim, n, K, ma, nq, R, batch, opq, 11)], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=900)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
