"""The C++14 mirrors on 16-bit codes: quick-adc_amd/host/scanner_simple_hip.hpp and host/adc_search_hip.hpp put a (2,16), (4,16) or
(8,16) database into an index of qadc_adc_index_create16.  Under the query engine of host/query_driver.hpp they fill every heap
exactly as the CPU scanner_simple (scan_standard<uint16_t, NSQ>, host/scanner_simple.hpp) does, on the same seeded database
(tests/cpp/scanner_simple_hip16_demo.cpp, tests/cpp/adc_search_hip16_demo.cpp)."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "tests", "cpp", "scanner_simple_hip16_demo")
SEARCH = os.path.join(ROOT, "tests", "cpp", "adc_search_hip16_demo")


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
    (2, 100000, 1, 1, 4, 100),
    (4, 1000, 1, 1, 3, 1500),         # R > n
    (8, 70001, 1, 1, 3, 1000),
    (2, 60000, 16, 4, 6, 10),
    (4, 50000, 32, 6, 4, 100),
    (8, 30000, 8, 3, 4, 1),
])
def test_scanner_simple_hip_fills_heaps_like_scan_standard_u16(scan_demo, M, n, K, ma, nq, R, finish):
    run_ok([scan_demo, M, n, K, ma, nq, R, finish, 5], nq)


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("finish", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("M,ds,n,K,ma,nq,R,batch,opq", [
    (2, 8, 1500, 0, 1, 5, 100, 2, 0),           # flat
    (8, 2, 300, 0, 1, 3, 500, 3, 1),            # flat, OPQ, R > n
    (4, 4, 600, 8, 3, 5, 10, 2, 0),             # IVF
    (2, 8, 1200, 8, 4, 4, 1, 4, 1),             # IVF, OPQ
])
def test_adc_search_engine_hip_fills_heaps_like_the_cpu_engine(search_demo, M, ds, n, K, ma, nq, R, batch, opq, finish):
    run_ok([search_demo, M, ds, n, K, ma, nq, R, batch, opq, finish, 7], nq)
