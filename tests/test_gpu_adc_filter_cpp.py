"""scanner_simple_hip::set_filter — the C++14 mirror's key filter (qadc_adc_index_set_filter) — against the
CPU twin, scanner_simple with a key_filter (host/scanner_simple.hpp), heap for heap on the same seeded database
(tests/cpp/scanner_simple_hip_filter_demo.cpp): without a filter, with a seeded share of the keys, with the keys of the unfiltered
heaps, and again after the filter was cleared."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "scanner_simple_hip_filter_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("mode", [0, 1], ids=["exclude", "allow"])
@pytest.mark.parametrize("M,n,K,ma,nq,R,finish", [
    (8, 12000, 1, 1, 4, 100, 0),          # flat: keys are positions
    (8, 30000, 16, 4, 6, 100, 1),         # labelled partitions, duplicate probes, the device finish
    (4, 12000, 8, 3, 4, 1, 0),
    (16, 12000, 8, 2, 4, 10, 1),
])
def test_scanner_simple_hip_with_a_filter_fills_heaps_like_the_twin(demo, M, n, K, ma, nq, R, finish, mode):
    out = subprocess.run([demo, str(M), str(n), str(K), str(ma), str(nq), str(R), "5", str(finish), str(mode), "30"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
