"""adc_search_engine_hip::set_query_filters — the C++14 mirror's one filter per query (qadc_adc_search_filtered,
qadc_adc_search_candidates_filtered) — against the CPU twin, scanner_simple under set_filter and
set_query_filter (host/scanner_simple.hpp), heap for heap on the same seeded database
(tests/cpp/adc_search_hip_qfilter_demo.cpp): without filters, with a different filter for every query (none, EXCLUDE, ALLOW, EXCLUDE
of the query's own winners), the same under an index-wide EXCLUDE, and again after everything was cleared."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_search_hip_qfilter_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("M,ds,n,K,ma,nq,R,batch,finish", [
    (8, 4, 12000, 0, 1, 8, 100, 8, 0),          # flat: keys are positions; one batch
    (8, 4, 12000, 16, 4, 11, 100, 4, 1),        # labelled partitions, batches of 4 (the last one short), the device finish
    (4, 8, 9000, 8, 3, 9, 1, 16, 0),            # R = 1, a batch larger than the query set
    (16, 2, 12000, 8, 2, 8, 10, 3, 1),
])
def test_the_engine_with_one_filter_per_query_fills_heaps_like_the_twin(demo, M, ds, n, K, ma, nq, R, batch, finish):
    out = subprocess.run([demo, str(M), str(ds), str(n), str(K), str(ma), str(nq), str(R), str(batch), "5", str(finish), "30"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
