"""refine_store_hip and search_refined — the C++14 mirror of the refine store (quick-adc_amd/host/refine_hip.hpp; DESIGN.md section
11.11) — beside the host twin (host/refine.hpp) on the same seeded IVF database (tests/cpp/refine_hip_demo.cpp): the engine's heaps
of R_IN entries re-ranked by the store and by the twin, for a float and a half store, with candidates the store does not hold."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("bits,M,ds,n,K,ma,nq,R,r_in", [
    (8, 8, 4, 20000, 16, 4, 6, 100, 400),       # 8x8
    (4, 16, 2, 20000, 16, 4, 6, 100, 1000),     # 16x4: a float-ADC view of a 4-bit index
], ids=["8x8", "16x4"])
def test_the_mirror_and_the_twin_agree(demo, bits, M, ds, n, K, ma, nq, R, r_in):
    out = subprocess.run([demo] + [str(v) for v in (bits, M, ds, n, K, ma, nq, R, r_in, 41)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
