"""refine_store_hip with SQ8 rows — the C++14 mirror (quick-adc_amd/host/refine_hip.hpp) — beside the host
twin (host/refine.hpp) on seeded vectors (tests/cpp/refine_sq_hip_demo.cpp): the range, a dense and a keyed store, get, the clamp
counter, rerank and knn."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_sq_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


def test_the_mirror_builds_as_cxx14(demo):
    assert os.path.exists(demo)


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("dim,n,nq,R", [(65, 257, 3, 40), (260, 128, 5, 200)])
def test_the_mirror_and_the_twin_agree(demo, dim, n, nq, R):
    out = subprocess.run([demo] + [str(v) for v in (dim, n, nq, R, 41)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
