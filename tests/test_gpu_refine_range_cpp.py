"""refine_store_hip::range and ::rerank_range — the C++14 mirrors of qadc_refine_range and qadc_refine_rerank_range
(quick-adc_amd/host/refine_hip.hpp) — through tests/cpp/refine_range_hip_demo.cpp: the demo holds the
mirrors to the host twins itself, and what it writes out must equal, bit for bit, what pyqadc.Refine returns on the same data."""
import os
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_range_cases as rr
from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_range_hip_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(EXE + ".cpp", EXE)
    return EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("dtype,keyed,flt", [("f32", False, None), ("f16", False, "exclude"), ("f32", True, "allow"), ("f16", True, None)],
                         ids=["f32-dense", "f16-dense-exclude", "f32-keyed-allow", "f16-keyed"])
def test_the_demo_equals_the_python_calls(demo, tmp_path, dtype, keyed, flt):
    import pyqadc
    rng = np.random.default_rng(92)
    dim, n, nq = 65, 8000, 9
    labels = rng.permutation(40000)[:n].astype(np.uint32) if keyed else np.arange(500, 500 + n, dtype=np.uint32)
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    d = ((vec[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(-1)
    radius = np.quantile(d, 0.02, axis=1).astype(np.float32)
    radius[1], radius[2] = 0.0, np.float32(np.quantile(d[2], 0.0005))          # nothing; a handful: no overflow of a region of 16 words
    fkeys = np.ascontiguousarray(labels[rng.random(n) < 0.5]) if flt else np.zeros(0, np.uint32)
    fin, fout = str(tmp_path / "demo.in"), str(tmp_path / "demo.out")
    with open(fin, "wb") as f:
        np.array([dim, rc.DTYPES[dtype], keyed, n, nq, -1 if flt is None else rr.MODES[flt], len(fkeys)], np.int32).tofile(f)
        for a in (labels, vec, q, radius, fkeys):
            a.tofile(f)
    out = subprocess.run([demo, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    with open(fout, "rb") as f:
        def csr():
            lims = np.fromfile(f, np.uint64, nq + 1)
            return lims, np.fromfile(f, np.uint32, int(lims[-1])), np.fromfile(f, np.float32, int(lims[-1]))
        gl, gk, gd = csr()
        in_lims = np.fromfile(f, np.uint64, nq + 1)
        in_keys = np.fromfile(f, np.uint32, int(in_lims[-1]))
        xl, xk, xd = csr()
        xm = int(np.fromfile(f, np.uint64, 1)[0])
        assert f.read() == b""
    assert out.stdout.decode().strip() == "ok %d %d" % (nq, len(gk))
    st = pyqadc.Refine(dim, dtype, keyed=keyed)
    if keyed:
        st.put(vec, labels)
    else:
        st.add(vec, int(labels[0]))
    pf = pyqadc.AdcFilter(fkeys, flt) if flt else None
    lims, keys, dist = st.range(q, radius, filter=pf)
    assert rr.same(dict(lims=gl, keys=gk, dist=gd, missing=0), dict(lims=lims, keys=keys, dist=dist, missing=0)) is None
    assert len(keys) > 100 and lims[2] == lims[1]
    ol, ok, od, missing = st.rerank_range(q, in_lims, in_keys, radius)
    assert rr.same(dict(lims=xl, keys=xk, dist=xd, missing=xm), dict(lims=ol, keys=ok, dist=od, missing=missing)) is None
    assert missing == 2 * nq and len(ok) >= len(keys)                       # (the candidates were found without the filter)
    if pf is not None:
        pf.close()
    st.close()


SEARCH_EXE = os.path.join(ROOT, "tests", "cpp", "refine_range_search_hip_demo")


@pytest.fixture(scope="module")
def search_demo():
    _compile(SEARCH_EXE + ".cpp", SEARCH_EXE)
    return SEARCH_EXE


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("bits,M,ds,n,K,ma,nq", [
    (8, 8, 4, 20000, 16, 4, 7),       # 8x8
    (4, 16, 2, 20000, 16, 4, 7),      # 16x4: a float-ADC view of a 4-bit index
], ids=["8x8", "16x4"])
def test_range_search_refined_equals_the_twin_on_the_engines_rows(search_demo, bits, M, ds, n, K, ma, nq):
    """range_search_refined(engine, store, ...) of host/refine_hip.hpp: the engine's range search, then the store's rerank_range, held
    by the demo to refine::rerank_range on the same rows, with rows the store does not hold"""
    out = subprocess.run([search_demo] + [str(x) for x in (bits, M, ds, n, K, ma, nq, 5)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    words = out.stdout.decode().split()
    assert words[0] == "ok" and int(words[1]) == nq and int(words[2]) > 0
