"""The C++14 mirrors on 4-bit codes: quick-adc_amd/host/scanner_simple_hip.hpp and host/adc_search_hip.hpp put a (16,4) or (32,4)
database into a qadc_index and scan it through a float-ADC view (qadc_adc_index_create_view).  Under the query engine of
host/query_driver.hpp they fill every heap exactly as the CPU scanner_simple (scan_4f, host/scanner_simple.hpp) does, on the same
seeded database (tests/cpp/scanner_simple_hip4_demo.cpp, tests/cpp/adc_search_hip4_demo.cpp)."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "tests", "cpp", "scanner_simple_hip4_demo")
SEARCH = os.path.join(ROOT, "tests", "cpp", "adc_search_hip4_demo")


@pytest.fixture(scope="module")
def scan_demo():
    _compile(SCAN + ".cpp", SCAN)
    return SCAN


@pytest.fixture(scope="module")
def search_demo():
    _compile(SEARCH + ".cpp", SEARCH)
    return SEARCH


def run_ok(args, nq):
    out = subprocess.run([str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("finish", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("M,n,K,ma,nq,R", [
    (16, 200000, 1, 1, 8, 100),
    (32, 1000, 1, 1, 4, 1500),        # R > n
    (32, 300000, 1, 1, 4, 1000),
    (16, 100000, 64, 24, 16, 100),
    (32, 50000, 32, 8, 8, 10),
    (16, 80000, 16, 4, 8, 1),
])
def test_scanner_simple_hip_fills_heaps_like_scan_4(scan_demo, M, n, K, ma, nq, R, finish):
    run_ok([scan_demo, M, n, K, ma, nq, R, finish, 5], nq)


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("finish", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("M,ds,n,K,ma,nq,R,batch,opq", [
    (16, 8, 50000, 0, 1, 9, 100, 4, 0),         # flat
    (32, 4, 500, 0, 1, 5, 1000, 2, 1),          # flat, OPQ, R > n
    (16, 8, 60000, 64, 8, 12, 100, 5, 0),       # IVF
    (32, 8, 40000, 32, 24, 7, 10, 3, 1),        # IVF, OPQ
    (16, 4, 30000, 16, 1, 6, 1, 6, 0),          # IVF, one probe: the direct table form
])
def test_adc_search_engine_hip_fills_heaps_like_the_cpu_engine(search_demo, M, ds, n, K, ma, nq, R, batch, opq, finish):
    run_ok([search_demo, M, ds, n, K, ma, nq, R, batch, opq, finish, 7], nq)
