"""The C++14 front end under the caller's labels (tests/cpp/refine_keyed_hip_demo.cpp; DESIGN.md sections 11.5 and 11.14):
qadc_adc_index_add_vectors_labelled beside the host twin's labelled add_vectors, refine_store_hip as a keyed store beside
refine::keyed_store, through a life of put, search_refined, remove and an overwriting put, for a float and a half store."""
import os
import subprocess

import pytest

from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_keyed_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
def test_the_mirror_and_the_twins_agree_through_a_life(demo):
    M, ds, n, K, ma, nq, R, r_in = 8, 4, 20000, 16, 4, 6, 100, 400
    out = subprocess.run([demo] + [str(v) for v in (M, ds, n, K, ma, nq, R, r_in, 43)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
