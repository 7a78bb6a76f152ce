"""refine_store_hip::knn — the C++14 mirror of qadc_refine_knn (quick-adc_amd/host/refine_hip.hpp) — through
tests/cpp/refine_knn_hip_demo.cpp: the demo holds the mirror to the host twin itself, and what it writes out must equal, bit for
bit, what pyqadc.Refine.knn returns on the same data."""
import os
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_knn_cases as kc
from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_knn_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("dtype,keyed,flt", [("f32", False, None), ("f16", False, "exclude"), ("f32", True, "allow"), ("f16", True, None)],
                         ids=["f32-dense", "f16-dense-exclude", "f32-keyed-allow", "f16-keyed"])
def test_the_demo_equals_the_python_call(demo, tmp_path, dtype, keyed, flt):
    import pyqadc
    rng = np.random.default_rng(91)
    dim, n, nq, R = 65, 8000, 9, 100
    labels = rng.permutation(40000)[:n].astype(np.uint32) if keyed else np.arange(500, 500 + n, dtype=np.uint32)
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    fkeys = np.ascontiguousarray(labels[rng.random(n) < 0.5]) if flt else np.zeros(0, np.uint32)
    fin, fout = str(tmp_path / "demo.in"), str(tmp_path / "demo.out")
    with open(fin, "wb") as f:
        np.array([dim, rc.DTYPES[dtype], keyed, n, nq, R, -1 if flt is None else kc.MODES[flt], len(fkeys)], np.int32).tofile(f)
        for a in (labels, vec, q, fkeys):
            a.tofile(f)
    out = subprocess.run([demo, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
    with open(fout, "rb") as f:
        got = dict(keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R), dist=np.fromfile(f, np.float32, nq * R).reshape(nq, R),
                   sizes=np.fromfile(f, np.int32, nq))
        assert f.read() == b""
    st = pyqadc.Refine(dim, dtype, keyed=keyed)
    if keyed:
        st.put(vec, labels)
    else:
        st.add(vec, int(labels[0]))
    pf = pyqadc.AdcFilter(fkeys, flt) if flt else None
    k, d, s = st.knn(q, R, filter=pf)
    assert kc.same(got, dict(keys=k, dist=d, sizes=s)) is None
    assert (s == R).all()
    if pf is not None:
        pf.close()
    st.close()
