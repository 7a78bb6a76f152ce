"""refine_store_hip under the inner-product metric — set_metric of quick-adc_amd/host/refine_hip.hpp —
through tests/cpp/refine_ip_hip_demo.cpp: the demo holds knn, rerank and knn_probed under QADC_REFINE_IP to the host twin itself,
and the arrays it writes out must equal, bit for bit, what pyqadc.Refine(metric="ip") returns on the same data."""
import os
import subprocess

import numpy as np
import pytest

import refine_ip_cases as ic
from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_ip_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_demo_equals_the_python_calls(demo, tmp_path, dtype):
    import pyqadc
    rng = np.random.default_rng(91)
    dim, n, nq, R, r_in, ma = 65, 1500, 9, 100, 300, 2
    sizes = np.array([0, 1, 63, 300, 700, 450], np.uint32)
    K = len(sizes)
    labels = rng.permutation(n + 14).astype(np.uint32)                         # 14 labels the store does not hold
    labels[::40] = labels[1::40]                                               # keys reached through two rows
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    cand = rng.integers(0, n + 20, (nq, r_in)).astype(np.uint32)
    assign = np.stack([rng.permutation(K)[:ma] for _ in range(nq)]).astype(np.int32)
    assign[0] = (4, 5)
    assert sizes.sum() == n + 14
    fin, fout = str(tmp_path / "demo.in"), str(tmp_path / "demo.out")
    with open(fin, "wb") as f:
        np.array([dim, ic.DTYPES[dtype], n, nq, R, r_in, K, ma], np.int32).tofile(f)
        for a in (sizes, labels, vec, q, cand, assign):
            a.tofile(f)
    out = subprocess.run([demo, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
    got = []
    with open(fout, "rb") as f:
        for _ in range(3):
            got.append(dict(keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R), dist=np.fromfile(f, np.float32, nq * R).reshape(nq, R),
                            sizes=np.fromfile(f, np.int32, nq), missing=0))
        got[1]["missing"], got[2]["missing"] = (int(x) for x in np.fromfile(f, np.uint64, 2))
        assert f.read() == b""
    st = pyqadc.Refine.from_vectors(vec, dtype, metric="ip")
    idx = ic.make_index(pyqadc, ic.split(labels, tuple(int(s) for s in sizes)))
    try:
        names = ("keys", "dist", "sizes", "missing")
        assert ic.same(got[0], dict(zip(names, st.knn(q, R) + (0,)))) is None
        assert ic.same(got[1], dict(zip(names, st.rerank(q, cand, R)))) is None
        assert ic.same(got[2], dict(zip(names, st.knn_probed(idx, q, assign, R)))) is None
        assert (got[0]["sizes"] == R).all() and got[1]["missing"] > 0 and got[2]["missing"] > 0
        assert (np.diff(got[0]["dist"], axis=1) <= 0).all()
    finally:
        idx.close()
        st.close()
