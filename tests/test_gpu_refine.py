"""GPU: the refine store (pyqadc.Refine over qadc_refine_*) against its host twin
(quick-adc_amd/host/refine.hpp through tests/cpp/refine_host.cpp): keys, the distances' bit patterns, sizes and the missing count,
for equality — there is no tolerance anywhere.  The shapes sit on the edges of the kernels: the strips of 64 components a lane
walks, the candidates a wave and a workgroup take, the three sort instantiations (512, 2048, 8192) and one workgroup per query."""
import ctypes as C

import numpy as np
import pytest

import refine_cases as rc
from helpers import path_independent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return rc.build_driver()


def store_of(pyqadc, c):
    st = pyqadc.Refine(c["dim"], c["dtype"])
    for first, vec in c["adds"]:
        st.add(vec, first)
    return st


def rerank(st, c, R=None):
    k, d, s, m = st.rerank(c["queries"], c["keys"], c["R"] if R is None else R, counts=c["counts"], values=c["values"])
    return dict(keys=k, dist=d, sizes=s, missing=m)


def check(pyqadc, twin, tmp_path, cases, names=None):
    wants = rc.run_twin(twin, tmp_path, cases)
    for i, (c, want) in enumerate(zip(cases, wants)):
        st = store_of(pyqadc, c)
        diff = rc.same(rerank(st, c), want)
        st.close()
        assert diff is None, "%s: %s differs from the twin" % (names[i] if names else i, diff)
    return wants


def candidate_keys(rng, nq, r_in, rows, lo=0):
    """even queries: distinct keys where the store has enough rows; odd ones: drawn with replacement (duplicates)"""
    keys = rng.integers(0, rows, (nq, r_in))
    if rows >= r_in:
        keys[0::2] = rng.random((len(keys[0::2]), rows)).argsort(1)[:, :r_in]
    return (keys + lo).astype(np.uint32)


# (r_in, nq, dim, rows): every r_in at an edge of the sort sizes and of the wave / workgroup tiling, every nq and every dim of the list
EDGES = [(1, 257, 128, 300), (63, 3, 65, 200), (64, 1, 64, 64), (65, 257, 63, 1000), (512, 3, 96, 2000), (513, 257, 1, 700),
         (2048, 1, 4096, 600), (2049, 3, 128, 5000), (8192, 257, 64, 10000), (8192, 1, 4096, 1024), (8192, 3, 65, 20000)]


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("r_in,nq,dim,rows", EDGES, ids=["rin%d-nq%d-dim%d" % e[:3] for e in EDGES])
def test_kernel_edges(pyqadc, twin, tmp_path, r_in, nq, dim, rows, dtype):
    rng = np.random.default_rng(r_in * 1000 + nq + dim)
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    keys = candidate_keys(rng, nq, r_in, rows)
    cases = [rc.case(dim, dtype, [(0, vec)], q, keys, R) for R in (1, r_in, r_in + 5)]
    wants = rc.run_twin(twin, tmp_path, cases)
    st = store_of(pyqadc, cases[0])
    for c, want in zip(cases, wants):
        diff = rc.same(rerank(st, c), want)
        assert diff is None, "R %d: %s differs from the twin" % (c["R"], diff)
    st.close()
    if rows >= r_in:
        assert wants[1]["sizes"][0] == r_in                               # a full list of distinct keys reaches the sort


@path_independent
def test_a_call_of_more_than_one_pass(pyqadc, twin, tmp_path):
    """2049 queries of 8192 candidates are more than the 2^24 candidates of a pass (host/refine_plan.hpp): the second pass serves the
    last query from the start of the scratch"""
    rng = np.random.default_rng(28)
    nq, r_in, rows = 2049, 8192, 500
    assert nq * r_in > 1 << 24 >= (nq - 1) * r_in
    vec = rng.normal(size=(rows, 1)).astype(np.float32)
    q = rng.normal(size=(nq, 1)).astype(np.float32)
    keys = rng.integers(0, rows + 10, (nq, r_in)).astype(np.uint32)                 # ten keys of every 510 are missing
    check(pyqadc, twin, tmp_path, [rc.case(1, "f32", [(0, vec)], q, keys, 3)])


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ties_duplicates_skipped_missing_and_non_finite(pyqadc, twin, tmp_path, dtype):
    rng = np.random.default_rng(21)
    cases, names = [], []
    for dim in rc.DIMS:
        cases += [rc.edge_case(rng, dim, dtype), rc.nonfinite_case(rng, dim, dtype)]
        names += ["edges dim %d" % dim, "non-finite dim %d" % dim]
        if dtype == "f16":
            cases.append(rc.half_range_case(rng, dim))
            names.append("half range dim %d" % dim)
    wants = check(pyqadc, twin, tmp_path, cases, names)
    assert wants[0]["missing"] == 4 and wants[0]["sizes"].tolist() == [6, 1, 6, 0, 0]
    img = wants[1]["dist"].view(np.uint32)
    assert (img[1, :30] == rc.NAN_IMAGE).all() and img[0, 29] == rc.NAN_IMAGE and np.isposinf(wants[1]["dist"][0, 27:29]).all()


@path_independent
def test_a_tie_of_identical_rows_straddles_every_place(pyqadc, twin, tmp_path):
    """600 identical rows under different keys plus 100 others, listed in a random order: the tie covers the R-th place at every R"""
    rng = np.random.default_rng(22)
    dim, rows = 96, 700
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[50:650] = vec[50]
    q = np.stack([vec[50], vec[50] + np.float32(0.5), vec[3]]).astype(np.float32)
    keys = np.stack([rng.permutation(rows) for _ in range(3)]).astype(np.uint32) + np.uint32(50)
    cases = [rc.case(dim, "f32", [(50, vec)], q, keys, R) for R in (1, 7, 599, 600, 601, 700)]
    wants = check(pyqadc, twin, tmp_path, cases)
    assert wants[1]["keys"][0].tolist() == list(range(100, 107)) and wants[3]["keys"][1].tolist() == list(range(100, 700))


@path_independent
def test_the_device_conversion_to_half_equals_numpy(pyqadc, twin, tmp_path):
    """every finite half, the float midway to its successor and that float's neighbours, both signs, as one-dimensional rows under
    the query 0: the distance is the stored value squared, so one wrong rounding on the device shows.  Through add and add_device."""
    import torch
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    nxt = np.arange(1, 0x7C01, dtype=np.uint16).view(np.float16).astype(np.float64)
    mid = ((h.astype(np.float64) + np.where(np.isinf(nxt), 65536.0, nxt)) / 2).astype(np.float32)
    vals = np.concatenate([h, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))]).astype(np.float32)
    vals = np.concatenate([vals, -vals, np.array([1e-10, -1e-10, 1e38, -1e38, np.inf, -np.inf], np.float32)]).reshape(-1, 1)
    with np.errstate(over="ignore"):
        stored = vals.astype(np.float16).astype(np.float32)
    assert np.isinf(stored).sum() > 6 and ((stored != 0) & (np.abs(stored) < 6.1e-5)).sum() > 4000          # overflow and subnormals
    st, st_dev = pyqadc.Refine(1, "f16"), pyqadc.Refine(1, "f16")
    st.add(vals)
    st_dev.add_device(torch.from_numpy(vals).cuda())
    q = np.zeros((1, 1), np.float32)
    with np.errstate(over="ignore"):
        want_d = (stored[:, 0] * stored[:, 0]).astype(np.float32)
    for first in range(0, len(vals), 8192):
        keys = np.arange(first, min(first + 8192, len(vals)), dtype=np.uint32)
        order = np.lexsort((keys, want_d[keys].view(np.uint32)))
        for s in (st, st_dev):
            k, d, sizes, missing = s.rerank(q, keys[None, :], len(keys))
            assert sizes[0] == len(keys) and missing == 0
            assert np.array_equal(k[0], keys[order]) and np.array_equal(d[0].view(np.uint32), want_d[keys][order].view(np.uint32))
    st.close()
    st_dev.close()


@path_independent
def test_missing_keys_and_the_ends_of_the_key_space(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(23)
    dim = 65
    vec = rng.normal(size=(300, dim)).astype(np.float32)
    q = rng.normal(size=(3, dim)).astype(np.float32)
    # a store at lo = 50: keys below lo, at lo + rows and far away are missing
    keys = (rng.integers(0, 400, (3, 100))).astype(np.uint32)
    keys[0, :4] = (49, 50, 349, 350)
    low = rc.case(dim, "f32", [(50, vec)], q, keys, 100)
    # the last 300 keys of the key space: 0xFFFFFFFF is held, 0 is not
    hi = 2 ** 32 - 300
    keys = (rng.integers(hi - 20, 2 ** 32, (3, 100))).astype(np.uint32)
    keys[0, :3] = (0xFFFFFFFF, 0, hi)
    keys[1, :] = 0
    top = rc.case(dim, "f16", [(hi, vec)], q, keys, 100)
    empty = rc.case(dim, "f32", [], q, keys, 5)                              # nothing added: everything is missing
    wants = check(pyqadc, twin, tmp_path, [low, top, empty], ["lo 50", "top of the key space", "empty store"])
    assert wants[0]["missing"] > 10 and 50 in wants[0]["keys"][0] and 349 in wants[0]["keys"][0]
    assert 49 not in wants[0]["keys"][0] and 350 not in wants[0]["keys"][0]
    assert 0xFFFFFFFF in wants[1]["keys"][0][:wants[1]["sizes"][0]] and wants[1]["sizes"][1] == 0 and wants[1]["missing"] >= 101
    assert wants[2]["missing"] == 300 and not wants[2]["sizes"].any()


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_growth_reserve_and_info(pyqadc, twin, tmp_path, dtype):
    rng = np.random.default_rng(24)
    dim, lo = 63, 1000
    sizes = [100, 1, 400, 37, 900]                                           # 1.5 x growth: 100 -> 150 -> 501 -> 751 -> 1438
    vec = rng.normal(size=(sum(sizes), dim)).astype(np.float32)
    q = rng.normal(size=(2, dim)).astype(np.float32)
    keys = (rng.integers(0, sum(sizes), (2, 200)) + lo - 20).astype(np.uint32)
    esz = 2 if dtype == "f16" else 4
    st, whole, roomy = pyqadc.Refine(dim, dtype), pyqadc.Refine(dim, dtype), pyqadc.Refine(dim, dtype)
    assert st.info() == dict(dim=dim, dtype=dtype, lo=0, rows=0, bytes=0)
    st.reserve(1)
    assert st.info()["bytes"] == dim * esz and st.relocations() == 0
    roomy.reserve(sum(sizes))
    room = roomy.info()["bytes"]
    assert room == sum(sizes) * dim * esz
    done, cases = 0, []
    for n in sizes:
        st.add(vec[done:done + n], lo if done == 0 else None)
        roomy.add(vec[done:done + n], lo + done)
        done += n
        info = st.info()
        assert (info["lo"], info["rows"]) == (lo, done) and info["bytes"] >= done * dim * esz
        assert roomy.info()["bytes"] == room and roomy.relocations() == 0
        c = rc.case(dim, dtype, [(lo, vec[:done])], q, keys, 50)
        cases.append(c)
        got, other = rerank(st, c), rerank(roomy, c)
        assert rc.same(got, other) is None
        cases[-1]["got"] = got
    assert st.relocations() >= 2
    st.reserve(1)                                                            # less than it holds: a no-op
    assert st.info()["rows"] == done
    whole.add(vec, lo)
    assert rc.same(rerank(whole, cases[-1]), cases[-1]["got"]) is None
    for c, want in zip(cases, rc.run_twin(twin, tmp_path, cases)):
        assert rc.same(c["got"], want) is None
    for s in (st, whole, roomy):
        s.close()


@path_independent
def test_device_io_equals_host_io(pyqadc, twin, tmp_path):
    import torch
    rng = np.random.default_rng(25)
    c = rc.edge_case(rng, 96, "f16")
    big = rc.random_case(rng, 128, "f32", 3000, 5, 600, 100, lo=7)
    big["keys"][2, :50] = 3                                                  # missing
    for case in (c, big):
        host = store_of(pyqadc, case)
        dev = pyqadc.Refine(case["dim"], case["dtype"])
        for first, vec in case["adds"]:
            dev.add_device(torch.from_numpy(vec).cuda(), first)
        assert dev.info() == host.info()
        want = rerank(host, case)
        assert rc.same(rerank(dev, case), want) is None                     # add_device == add
        t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
        k, d, s, m = host.rerank_device(t(case["queries"], np.float32), t(case["keys"], np.int32), case["R"], counts=t(case["counts"], np.int32),
                                        values=t(case["values"], np.float32))
        assert k.dtype == torch.int32 and k.is_cuda and d.is_cuda and s.is_cuda
        got = dict(keys=k.cpu().numpy().view(np.uint32), dist=d.cpu().numpy(), sizes=s.cpu().numpy(), missing=m)
        assert rc.same(got, want) is None                                    # rerank_device == rerank
        host.close()
        dev.close()
    # the device form clamps counts to [0, r_in]; the host form refuses them
    st = store_of(pyqadc, big)
    counts = np.array([-3, 600 + 7, 10, 0, 600], np.int32)
    k, d, s, m = st.rerank_device(t(big["queries"], np.float32), t(big["keys"], np.int32), 100, counts=t(counts, np.int32))
    want = st.rerank(big["queries"], big["keys"], 100, counts=np.clip(counts, 0, 600))
    assert np.array_equal(k.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(d.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(s.cpu().numpy(), want[2]) and m == want[3] and want[2][0] == 0 and want[2][3] == 0
    with pytest.raises(pyqadc.QadcError):
        st.rerank(big["queries"], big["keys"], 100, counts=counts)
    st.close()


@path_independent
def test_the_result_depends_on_the_set_of_candidates_only(pyqadc):
    rng = np.random.default_rng(26)
    c = rc.random_case(rng, 64, "f32", 5000, 4, 2049, 300)
    st = store_of(pyqadc, c)
    a = rerank(st, c)
    c["keys"] = np.stack([rng.permutation(row) for row in c["keys"]])
    assert rc.same(rerank(st, c), a) is None
    st.close()


@path_independent
def test_refusals_leave_the_store_usable(pyqadc):
    L = pyqadc.lib()
    E = pyqadc.QADC_E_ARG
    h = C.c_void_p()
    assert L.qadc_refine_create(None, 8, 0, 0) == E
    for dim, dtype in ((0, 0), (-1, 0), (4097, 0), (8, 2), (8, -1)):
        assert L.qadc_refine_create(C.byref(h), dim, dtype, 0) == E and not h.value, (dim, dtype)
    assert b"dtype" in L.qadc_last_error()

    rng = np.random.default_rng(27)
    c = rc.random_case(rng, 8, "f32", 100, 2, 20, 5, lo=10)
    st = store_of(pyqadc, c)
    before, info = rerank(st, c), st.info()
    v = c["adds"][0][1]

    def refused(call):
        with pytest.raises(pyqadc.QadcError, match="qadc error -1"):
            call()
        assert st.info() == info and rc.same(rerank(st, c), before) is None

    refused(lambda: st.add_raw(None, 5, 110))                                # vectors NULL
    refused(lambda: st.add(v[:5], 111))                                      # a gap
    refused(lambda: st.add(v[:5], 109))                                      # an overlap
    refused(lambda: st.add(v[:5], 10))
    refused(lambda: st.reserve(2 ** 32 + 1))
    assert L.qadc_refine_add(None, None, 0, 0) == E and L.qadc_refine_reserve(None, 1) == E and L.qadc_refine_info(None, None, None, None, None, None) == E
    top = pyqadc.Refine(8, "f32")
    top.add(v[:10], 2 ** 32 - 20)
    with pytest.raises(pyqadc.QadcError, match="qadc error -1"):
        top.add(v[:11])                                                      # would pass 2^32
    top.add(v[:10])                                                          # ... and exactly reaches it
    assert top.info()["rows"] == 20 and top.info()["lo"] == 2 ** 32 - 20
    top.close()

    q, k = c["queries"], c["keys"]
    refused(lambda: st.rerank_raw(2, q, 0, k, None, None, 5))                # r_in
    big = np.zeros((2, 8193), np.uint32)
    refused(lambda: st.rerank_raw(2, q, 8193, big, None, None, 5))
    refused(lambda: st.rerank_raw(2, q, 20, k, None, None, 0))               # R
    refused(lambda: st.rerank_raw(2, q, 20, k, None, None, -1))
    refused(lambda: st.rerank_raw(-1, q, 20, k, None, None, 5))
    refused(lambda: st.rerank_raw(2, None, 20, k, None, None, 5))            # NULL where required
    refused(lambda: st.rerank_raw(2, q, 20, None, None, None, 5))
    refused(lambda: st.rerank_raw(2, q, 20, k, None, None, 5, outputs=False))
    refused(lambda: st.rerank_raw(2, q, 20, k, np.array([0, 21], np.int32), None, 5))     # counts outside [0, r_in]
    refused(lambda: st.rerank_raw(2, q, 20, k, np.array([-1, 3], np.int32), None, 5))
    m = C.c_uint64(0)
    assert L.qadc_refine_rerank(None, 2, None, 20, None, None, None, 5, None, None, None, C.byref(m)) == E
    assert L.qadc_refine_rerank_device(None, 2, None, 20, None, None, None, 5, None, None, None, C.byref(m)) == E
    assert L.qadc_refine_rerank_device(st._h, 2, None, 20, None, None, None, 5, None, None, None, C.byref(m)) == E
    assert L.qadc_refine_rerank_device(st._h, 2, 8, 0, 8, None, None, 5, 8, 8, 8, C.byref(m)) == E       # (refused before any pointer is read)
    assert L.qadc_refine_rerank_device(st._h, 2, 8, 20, 8, None, None, 0, 8, 8, 8, C.byref(m)) == E
    assert rc.same(rerank(st, c), before) is None
    k2, d2, s2, m2 = st.rerank_raw(0, q, 20, k, None, None, 5)               # no query: a no-op
    assert m2 == 0
    st.close()
    assert L.qadc_refine_destroy(None) == 0
