"""quick-adc_amd/host/scanner_simple_hip.hpp with set_finish(1), the device finish: under the query engine of
host/query_driver.hpp it fills every heap exactly as the CPU scanner_simple (host/scanner_simple.hpp) does, on the same seeded
database (tests/cpp/scanner_simple_hip_finish_demo.cpp), and leaves no query to the host."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "scanner_simple_hip_finish_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(os.path.join(ROOT, "tests", "cpp", "scanner_simple_hip_finish_demo.cpp"), EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("finish", [1, 0])
@pytest.mark.parametrize("M,n,K,ma,nq,R", [
    (8, 200000, 1, 1, 8, 100),
    (4, 1000, 1, 1, 4, 1500),         # R > n
    (16, 300000, 1, 1, 4, 1000),
    (8, 100000, 64, 24, 16, 100),
    (16, 50000, 32, 8, 8, 10),
    (4, 80000, 16, 4, 8, 1),
])
def test_scanner_simple_hip_fills_heaps_like_scanner_simple_under_either_finish(demo, M, n, K, ma, nq, R, finish):
    out = subprocess.run([demo, str(M), str(n), str(K), str(ma), str(nq), str(R), "5", str(finish)], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq


@pytest.mark.gpu
@path_independent
def test_scanner_simple_hip_refuses_another_finish_mode(demo):
    out = subprocess.run([demo, "8", "100", "1", "1", "1", "10", "5", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=120)
    assert out.returncode == 1
    assert "set_finish" in out.stderr.decode()
