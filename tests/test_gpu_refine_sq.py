"""GPU: SQ8 refine rows and the read-back (qadc_refine_create_sq8, _sq_range_*, _sq_info, _get*) through
the C-ABI.  Every script of tests/refine_sq_cases.py is replayed on the library, host form and device form, and equals the host
twin (tests/cpp/refine_sq_host.cpp) bit for bit: the rows get() decodes (which pin the stored bytes), the clamp counter, keys, the
distances' bit patterns, sizes and missing counts."""
import ctypes as C

import numpy as np
import pytest

import refine_sq_cases as sq
from helpers import path_independent

pytestmark = pytest.mark.gpu

F32 = np.float32
FORMS = ["host", "device"]
RERANK_DIMS = (1, 63, 64, 65, 96, 128, 255, 256, 257, 260, 4096)
# (dim, nq): every tile of the plan — 4 x J1..J4 and 4 in LDS for calls of up to 4 queries; 32 x J1, 32 x J2, 16 x J3, 16 x J4 and the
# LDS tiles of 32, 16, 8 and 4 queries for larger calls
KNN_SHAPES = ((1, 3), (65, 4), (129, 2), (256, 3), (260, 4), (4096, 2), (63, 6), (96, 5), (192, 7), (255, 5), (260, 6), (1024, 5), (2048, 5),
              (4096, 5))


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return sq.build_driver()


def dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 and dtype == np.uint32 else a


def run_gpu(p, s, form, knn_plan=None):
    """a script on the library -> dict(refused, ops); form "device" takes every call's *_device form"""
    dim, d = s["dim"], form == "device"
    try:
        st = p.Refine(dim, s["dtype"], keyed=s["keyed"], vmin=s["vmin"], step=s["step"])
    except p.QadcError:
        return dict(refused=1, ops=[])
    if knn_plan:
        st.set_knn_plan(*knn_plan)
    out = []
    for op in s["ops"]:
        if op[0] == "add":
            v = sq._vec(op[2], dim)
            try:
                st.add_device(dev(v), int(op[1])) if d else st.add(v, int(op[1]))
                out.append(dict(ok=np.array([1], np.int32)))
            except p.QadcError:
                out.append(dict(ok=np.array([0], np.int32)))
        elif op[0] == "put":
            v, lab = sq._vec(op[2], dim), sq._u32(op[1])
            st.put_device(dev(v), dev(lab)) if d else st.put(v, lab)
            out.append(dict(ok=np.array([1], np.int32)))
        elif op[0] == "remove":
            lab = sq._u32(op[1])
            out.append(dict(removed=np.array([st.remove_device(dev(lab)) if d else st.remove(lab)], np.uint64)))
        elif op[0] == "get":
            k = sq._u32(op[1])
            if d:
                rows, found = st.get_device(dev(k))
                rows, found = host(rows), host(found)
            else:
                rows, found = st.get(k)
            out.append(dict(rows=rows, found=np.asarray(found, np.uint8)))
        elif op[0] == "bytes":
            out.append(dict())                                                        # (the rows of get() pin them)
        elif op[0] == "info":
            out.append(dict(clamped=np.array([st.sq_info()["clamped"]], np.uint64), held=np.array([st.info()["rows"]], np.uint64)))
        elif op[0] == "range":
            v = sq._vec(op[1], dim)
            a, b = p.refine_sq_range_device(dev(v)) if d else p.refine_sq_range(v)
            out.append(dict(vmin=a, step=b))
        elif op[0] == "rerank":
            q = sq._vec(op[1], dim)
            keys = np.ascontiguousarray(op[2], np.uint32).reshape(len(q), -1)
            if d:
                k, dist, sizes, missing = st.rerank_device(dev(q), dev(keys), op[3], counts=None if op[4] is None else dev(np.asarray(op[4], np.int32)),
                                                           values=None if op[5] is None else dev(np.asarray(op[5], F32)))
                k, dist, sizes = host(k, np.uint32), host(dist), host(sizes)
            else:
                k, dist, sizes, missing = st.rerank(q, keys, op[3], counts=op[4], values=op[5])
            out.append(dict(missing=np.array([missing], np.uint64), keys=k, dist=dist, sizes=sizes))
        elif op[0] == "knn":
            q = sq._vec(op[1], dim)
            f = None if op[3] is None else p.AdcFilter(sq._u32(op[4]), mode="allow" if op[3] == 1 else "exclude")
            if d:
                k, dist, sizes = st.knn_device(dev(q), op[2], filter=f)
                k, dist, sizes = host(k, np.uint32), host(dist), host(sizes)
            else:
                k, dist, sizes = st.knn(q, op[2], filter=f)
            if f is not None:
                f.close()
            out.append(dict(keys=k, dist=dist, sizes=sizes))
    st.close()
    return dict(refused=0, ops=out)


def replay(p, twin, tmp_path, scripts, form, knn_plan=None):
    want = sq.run_twin(twin, tmp_path, scripts)
    for s, w in zip(scripts, want):
        g = run_gpu(p, s, form, knn_plan)
        assert sq.same(g, w) is None, "dim %d %s keyed=%s, %s form: %s" % (s["dim"], s["dtype"], s["keyed"], form, sq.same(g, w))
    return want


@path_independent
@pytest.mark.parametrize("form", FORMS)
def test_encoder_bytes_and_clamp_counter(pyqadc, twin, tmp_path, form):
    """add / add_device and put / put_device: the bytes (through get) and the counter after several calls"""
    scripts = [sq.grid_script(dim)[0] for dim in sq.DIMS]
    scripts += [sq.edge_script(dim, keyed) for dim in sq.DIMS for keyed in (False, True)]
    scripts += [sq.keyed_script(dim) for dim in (1, 65, 260)]
    want = replay(pyqadc, twin, tmp_path, scripts, form)
    assert any(int(w["ops"][-1]["clamped"][0]) > 0 for w in want)


@path_independent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_rerank(pyqadc, twin, tmp_path, keyed, form):
    scripts = [sq.rerank_script(dim, keyed, r_in, rows=300 if dim < 4096 else 80) for dim in RERANK_DIMS for r_in in (17, 65)]
    replay(pyqadc, twin, tmp_path, scripts, form)


@path_independent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_knn_over_several_launches(pyqadc, twin, tmp_path, keyed, form):
    """chunk_rows = 64: 300 rows take several launches; pass_nq = 3 cuts the larger calls into passes"""
    scripts = [sq.knn_script(dim, keyed, nq, rows=300 if dim < 1024 else 150) for dim, nq in KNN_SHAPES]
    replay(pyqadc, twin, tmp_path, scripts, form, knn_plan=(64, 3))


@path_independent
def test_knn_of_an_empty_store(pyqadc, twin, tmp_path):
    q = np.ones((2, 65), F32)
    scripts = [sq.script(65, "sq8", [("knn", q, 5, None, []), ("get", [0, 1]), ("info",)], keyed=k, vmin=np.zeros(65), step=np.ones(65))
               for k in (False, True)]
    for form in FORMS:
        replay(pyqadc, twin, tmp_path, scripts, form)


@path_independent
@pytest.mark.parametrize("form", FORMS)
def test_sq_range(pyqadc, twin, tmp_path, form):
    """n = 0, 1, 67 (no multiple of the kernel's tile of 64 rows) and 1000 at dims 1, 65 and 4096; a column with nothing finite"""
    replay(pyqadc, twin, tmp_path, sq.range_scripts(), form)


@path_independent
def test_refusals(pyqadc, twin, tmp_path):
    """the parameters no store takes; qadc_refine_create keeps refusing dtype 2; sq_info belongs to SQ8 stores"""
    scripts = sq.refusal_scripts()
    want = replay(pyqadc, twin, tmp_path, scripts, "host")
    assert all(w["refused"] == 1 for w in want)
    L = pyqadc.lib()
    h = C.c_void_p()
    assert L.qadc_refine_create(C.byref(h), 8, 2, 0) == pyqadc.QADC_E_ARG and not h.value
    assert L.qadc_refine_create_keyed(C.byref(h), 8, 2, 0) == pyqadc.QADC_E_ARG and not h.value
    one = np.ones(8, F32)
    f32p = C.POINTER(C.c_float)
    assert L.qadc_refine_create_sq8(C.byref(h), 8, None, one.ctypes.data_as(f32p), 0, 0) == pyqadc.QADC_E_ARG
    assert L.qadc_refine_create_sq8(C.byref(h), 0, one.ctypes.data_as(f32p), one.ctypes.data_as(f32p), 0, 0) == pyqadc.QADC_E_ARG
    st = pyqadc.Refine(8, "f16")
    assert L.qadc_refine_sq_info(st._h, None, None, None) == pyqadc.QADC_E_STATE
    st.close()
    st = pyqadc.Refine(8, "sq8", vmin=one, step=one)
    assert L.qadc_refine_sq_info(st._h, None, None, None) == 0
    i = st.sq_info()
    assert np.array_equal(i["vmin"], one) and np.array_equal(i["step"], one) and i["clamped"] == 0
    assert L.qadc_refine_get(st._h, None, 0, None, None) == 0
    st.close()


@path_independent
def test_get_of_float_and_half_stores(pyqadc, twin, tmp_path):
    for form in FORMS:
        replay(pyqadc, twin, tmp_path, sq.plain_get_scripts(), form)


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_growth_keeps_every_byte(pyqadc, keyed):
    """rows are dim bytes, no padding: info's bytes = capacity x dim; adds that relocate keep every row"""
    rng = np.random.default_rng(2)
    dim, n = 63, 301
    v, vmin, step = sq.data_params(rng, n, dim)
    lab = np.arange(n, dtype=np.uint32) + 9
    st = pyqadc.Refine(dim, "sq8", keyed=keyed, vmin=vmin, step=step)
    put = (lambda a, b: st.put(v[a:b], lab[a:b])) if keyed else (lambda a, b: st.add(v[a:b], 9 + a))
    fixed = st.keyed_info()["table_slots"] * 12 if keyed else 0
    per_row = dim + (8 if keyed else 0)
    st.reserve(100)
    assert st.info()["bytes"] == 100 * per_row + fixed and st.info()["dtype"] == "sq8"
    put(0, 100)
    before, found = st.get(lab[:100])
    assert found.all() and st.relocations() == 0
    put(100, 101)                                                                     # 1.5 x the allocation
    assert st.relocations() == 1 and st.info()["bytes"] == 150 * per_row + fixed
    put(101, n)
    assert st.relocations() == 2 and st.info()["bytes"] == n * per_row + fixed
    after, found = st.get(lab)
    assert found.all() and np.array_equal(after[:100].view(np.uint32), before.view(np.uint32))
    c, _ = sq.np_encode(v, vmin, step)
    assert np.array_equal(after.view(np.uint32), sq.np_decode(c, vmin, step).view(np.uint32))
    st.close()


@path_independent
def test_search_refined_device_takes_an_sq8_store(pyqadc, twin, tmp_path):
    """AdcIndex.search_refined* on a tiny 8x8 index (K = 4) with an SQ8 store = search_device, then the twin's rerank"""
    import torch
    rng = np.random.default_rng(4)
    dim, n, K, nq, ma, R, r_in = 32, 2000, 4, 6, 2, 10, 40
    coarse = (rng.normal(size=(K, dim)) * 2).astype(F32)
    vec = (coarse[rng.integers(0, K, n)] + rng.normal(size=(n, dim))).astype(F32)
    queries = (vec[rng.integers(0, n, nq)] + 0.3 * rng.normal(size=(nq, dim))).astype(F32)
    resid = (vec - coarse[pyqadc.coarse_assign(vec, coarse, 1)[:, 0]]).astype(F32)
    idx = pyqadc.AdcIndex(8, 8)
    idx.set_pq(pyqadc.pq_seed(resid, 8, 8, rng))
    idx.set_coarse(coarse)
    idx.add_vectors(vec, labels_offset=0)
    st = pyqadc.Refine.from_vectors(vec, dtype="sq8")
    info = st.sq_info()
    # (the set's own maxima may count: (max - min) * inv can round above 255 where inv = 1 / step is rounded up; the byte is 255)
    assert info["clamped"] == int(sq.np_encode(vec, info["vmin"], info["step"])[1].sum()) <= dim
    assert st.info()["rows"] == n and st.info()["bytes"] == n * dim
    dq = torch.from_numpy(queries).cuda()
    keys, vals, _ = idx.search_device(dq, ma, r_in)
    gk, gd, gs, gm = idx.search_refined_device(dq, ma, R, r_in, st)
    hk, hd, hs, hm = idx.search_refined(queries, ma, R, r_in, st)
    s = sq.script(dim, "sq8", [("add", 0, vec), ("rerank", queries, host(keys, np.uint32), R, None, host(vals))], vmin=info["vmin"],
                  step=info["step"])
    want = sq.run_twin(twin, tmp_path, [s])[0]["ops"][1]
    for k, d, z, m in ((host(gk, np.uint32), host(gd), host(gs), gm), (hk, hd, hs, hm)):
        assert np.array_equal(k, want["keys"]) and np.array_equal(d.view(np.uint32), want["dist"].view(np.uint32))
        assert np.array_equal(z, want["sizes"]) and m == int(want["missing"][0])
    idx.close()
    st.close()
