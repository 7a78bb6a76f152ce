"""Range search through the C++14 mirrors — scanner_simple_hip::range_scan and adc_search_engine_hip::range_search
(quick-adc_amd/host/scanner_simple_hip.hpp, adc_search_hip.hpp; qadc_adc_range_*) — against the CPU twin
scanner_simple::range_scan on the same seeded database (tests/cpp/adc_range_hip_demo.cpp): keys and value bits of every query, without
filters and under an index-wide EXCLUDE with per-query ALLOWs, with radii from the query's own R-heap, +inf and -inf."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_range_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("M,ds,n,K,ma,nq,R", [
    (8, 4, 12000, 0, 1, 7, 100),            # flat: keys are positions; query 2 keeps all 12000 rows (a re-run, radix passes)
    (8, 4, 12000, 16, 4, 11, 50),           # labelled partitions, two of them empty
    (16, 2, 9000, 8, 2, 6, 10),
])
def test_both_mirrors_return_the_twins_rows(demo, M, ds, n, K, ma, nq, R):
    out = subprocess.run([demo, str(M), str(ds), str(n), str(K), str(ma), str(nq), str(R), "5", "30"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    ok, queries, rows = out.stdout.decode().split()
    assert ok == "ok" and int(queries) == nq and int(rows) > n // 2
