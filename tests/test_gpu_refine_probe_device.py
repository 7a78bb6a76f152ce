"""GPU: the probed exact search on torch tensors, and the composition with the coarse step:
Refine.knn_probed_device with and without out=; AdcIndex.assign / assign_device against the probe lists search() reports;
search_exact / search_exact_device against knn_probed on those lists, and at ma = K against Refine.knn; Index.search_exact through a
view; and the C++14 mirrors (quick-adc_amd/host/refine_hip.hpp) through tests/cpp/refine_probe_hip_demo.cpp, which holds them to the
host twin itself and whose output must equal the Python calls bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import refine_knn_cases as kc
import refine_probe_cases as pc
from helpers import path_independent
from test_scanner_hip_cpp import _compile

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_probe_hip_demo")
K = len(pc.SIZES)
N = sum(pc.SIZES)
DIM = 16


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return pc.build_driver()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def host(k, d, s):
    return dict(keys=k.cpu().numpy().view(np.uint32), dist=d.cpu().numpy(), sizes=s.cpu().numpy())


def ivf(pyqadc, rng, dtype="f32"):
    """a store of the keys 0 .. N and an owned index over them with quantizers: random codes, labels that hold every key once"""
    vec = rng.normal(size=(N, DIM)).astype(np.float32)
    st = pyqadc.Refine(DIM, dtype)
    st.add(vec, 0)
    idx = pc.make_index(pyqadc, pc.split_labels(rng.permutation(np.arange(N, dtype=np.uint32))))
    idx.set_pq(rng.normal(size=(8, 256, DIM // 8)).astype(np.float32))
    idx.set_coarse(rng.normal(size=(K, DIM)).astype(np.float32))
    return st, idx


@path_independent
def test_torch_tensors_in_and_out(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(1)
    q = rng.normal(size=(33, 65)).astype(np.float32)
    a = pc.probes(rng, 33, 2, K)
    c = pc.dense_case(rng, 65, "f16", lambda vec, labels: [pc.call(q, a, 40)])
    (want,) = pc.run_twin(twin, tmp_path, [c])
    st, idx = pc.make_store(pyqadc, c), pc.make_index(pyqadc, c["parts"])
    try:
        k, d, s, m = st.knn_probed_device(idx, dev(q), dev(a), 40)
        assert k.dtype == torch.int32 and k.is_cuda and tuple(k.shape) == (33, 40) and tuple(s.shape) == (33,)
        assert pc.same(dict(host(k, d, s), missing=m), want[0]) is None
        out = (torch.full((33, 40), 7, dtype=torch.int32, device="cuda:0"), torch.full((33, 40), 7.0, device="cuda:0"),
               torch.full((33,), 7, dtype=torch.int32, device="cuda:0"))
        k2, d2, s2, m2 = st.knn_probed_device(idx, dev(q), dev(a), 40, out=out)
        assert k2 is out[0] and d2 is out[1] and s2 is out[2] and pc.same(dict(host(*out), missing=m2), want[0]) is None
        with pytest.raises(TypeError):
            st.knn_probed_device(idx, dev(q), dev(a.astype(np.int64)), 40)
        with pytest.raises(pyqadc.QadcError):
            st.knn_probed_device(idx, dev(q), dev(a), 40, out=(out[0][:, :39], out[1], out[2]))
    finally:
        idx.close()
        st.close()


@path_independent
@pytest.mark.parametrize("ma", [1, 3, K])
def test_search_exact_is_assign_then_knn_probed(pyqadc, ma):
    rng = np.random.default_rng(2)
    st, idx = ivf(pyqadc, rng)
    q = rng.normal(size=(33, DIM)).astype(np.float32)
    try:
        assign = idx.search(q, ma, 10)[3]
        assert np.array_equal(idx.assign(q, ma), assign) and np.array_equal(idx.assign_device(dev(q), ma).cpu().numpy(), assign)
        k, d, s, m, a = idx.search_exact(q, ma, 50, st)
        wk, wd, ws, wm = st.knn_probed(idx, q, assign, 50)
        assert np.array_equal(a, assign) and pc.same(dict(keys=k, dist=d, sizes=s, missing=m), dict(keys=wk, dist=wd, sizes=ws, missing=wm)) is None
        dk, dd, ds, dm, da = idx.search_exact_device(dev(q), ma, 50, st)
        assert np.array_equal(da.cpu().numpy(), assign) and pc.same(dict(host(dk, dd, ds), missing=dm), dict(keys=wk, dist=wd, sizes=ws, missing=wm)) is None
        flt = pyqadc.AdcFilter(np.arange(0, N, 2, dtype=np.uint32), "allow")
        fk, fd, fs, fm, _ = idx.search_exact(q, ma, 50, st, filter=flt)
        assert (fk[fk != pc.NO_KEY] % 2 == 0).all() and fm == 0
        if ma == K:                                                          # every partition probed: the exhaustive search
            nk, nd, ns = st.knn(q, 50)
            assert m == 0 and kc.same(dict(keys=k, dist=d, sizes=s), dict(keys=nk, dist=nd, sizes=ns)) is None
            nk, nd, ns = st.knn(q, 50, filter=flt)
            assert kc.same(dict(keys=fk, dist=fd, sizes=fs), dict(keys=nk, dist=nd, sizes=ns)) is None
        flt.close()
    finally:
        idx.close()
        st.close()


@path_independent
def test_a_flat_index_probes_partition_zero(pyqadc):
    rng = np.random.default_rng(3)
    vec = rng.normal(size=(500, DIM)).astype(np.float32)
    st = pyqadc.Refine(DIM, "f32")
    st.add(vec, 0)
    idx = pc.make_index(pyqadc, [pc.part(None, 0, 500)])
    idx.set_pq(rng.normal(size=(8, 256, DIM // 8)).astype(np.float32))
    try:
        q = rng.normal(size=(5, DIM)).astype(np.float32)
        assert (idx.assign(q, 1) == 0).all()
        k, d, s, m, a = idx.search_exact(q, 1, 20, st)
        nk, nd, ns = st.knn(q, 20)
        assert (a == 0).all() and m == 0 and kc.same(dict(keys=k, dist=d, sizes=s), dict(keys=nk, dist=nd, sizes=ns)) is None
    finally:
        idx.close()
        st.close()


@path_independent
def test_a_4_bit_index_searches_exactly_through_a_view(pyqadc):
    rng = np.random.default_rng(4)
    vec = rng.normal(size=(N, DIM)).astype(np.float32)
    st = pyqadc.Refine(DIM, "f32")
    st.add(vec, 0)
    parts = pc.split_labels(rng.permutation(np.arange(N, dtype=np.uint32)))
    src = pyqadc.Index(16)
    src.add_partitions([rng.integers(0, 256, (p[2], 8), dtype=np.uint8) for p in parts], [p[0] for p in parts])
    src.set_pq(rng.normal(size=(16, 16, DIM // 16)).astype(np.float32))
    src.set_coarse(rng.normal(size=(K, DIM)).astype(np.float32))
    src.finalize(0.01)
    q = rng.normal(size=(9, DIM)).astype(np.float32)
    try:
        k, d, s, m, a = src.search_exact(q, K, 30, st)
        nk, nd, ns = st.knn(q, 30)
        assert m == 0 and sorted(a[0].tolist()) == list(range(K)) and kc.same(dict(keys=k, dist=d, sizes=s), dict(keys=nk, dist=nd, sizes=ns)) is None
        k, d, s, m, a = src.search_exact(q, 2, 30, st)
        view = pyqadc.AdcIndex.view_of(src)
        wk, wd, ws, wm = st.knn_probed(view, q, a, 30)
        view.close()
        assert pc.same(dict(keys=k, dist=d, sizes=s, missing=m), dict(keys=wk, dist=wd, sizes=ws, missing=wm)) is None
    finally:
        src.close()
        st.close()


@path_independent
@pytest.mark.parametrize("dtype,keyed", [("f32", False), ("f16", True)], ids=["f32-dense", "f16-keyed"])
def test_the_demo_equals_the_python_calls(pyqadc, tmp_path, dtype, keyed):
    _compile(EXE + ".cpp", EXE)
    rng = np.random.default_rng(91)
    nq, ma, R = 9, 2, 100
    keys = rng.permutation(40000)[:N].astype(np.uint32) if keyed else np.arange(500, 500 + N, dtype=np.uint32)
    vec = rng.normal(size=(N, DIM)).astype(np.float32)
    labels = rng.permutation(keys)
    labels[::9] = labels[1::9][:len(labels[::9])]                            # keys reached through two rows
    labels[5] = 77777                                                        # and one the store does not hold
    cb = rng.normal(size=(8, 256, DIM // 8)).astype(np.float32)
    cent = rng.normal(size=(K, DIM)).astype(np.float32)
    q = rng.normal(size=(nq, DIM)).astype(np.float32)
    assign = pc.probes(rng, nq, ma, K)
    fin, fout = str(tmp_path / "demo.in"), str(tmp_path / "demo.out")
    with open(fin, "wb") as f:
        np.array([DIM, pc.DTYPES[dtype], keyed, N, K, nq, ma, R], np.int32).tofile(f)
        for arr in (keys, vec, np.array(pc.SIZES, np.uint32), labels, cb, cent, q, assign):
            arr.tofile(f)
    out = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    assert out.stdout.decode().strip() == "ok %d" % nq
    with open(fout, "rb") as f:
        def result():
            return dict(keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R), dist=np.fromfile(f, np.float32, nq * R).reshape(nq, R),
                        sizes=np.fromfile(f, np.int32, nq), missing=int(np.fromfile(f, np.uint64, 1)[0]))
        probed, exact = result(), result()
        probes = np.fromfile(f, np.int32, nq * ma).reshape(nq, ma)
        assert f.read() == b""
    st = pyqadc.Refine(DIM, dtype, keyed=keyed)
    if keyed:
        st.put(vec, keys)
    else:
        st.add(vec, int(keys[0]))
    idx = pc.make_index(pyqadc, pc.split_labels(labels))
    idx.set_pq(cb)
    idx.set_coarse(cent)
    try:
        k, d, s, m = st.knn_probed(idx, q, assign, R)
        assert pc.same(probed, dict(keys=k, dist=d, sizes=s, missing=m)) is None
        k, d, s, m, a = idx.search_exact(q, ma, R, st)
        assert np.array_equal(a, probes) and pc.same(exact, dict(keys=k, dist=d, sizes=s, missing=m)) is None
    finally:
        idx.close()
        st.close()
