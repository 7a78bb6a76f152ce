"""GPU: the probed exact search by inner product (pyqadc.Refine(metric="ip").knn_probed and .knn_probed_device over
qadc_refine_knn_probed*) against the host twin (refine::knn_probed of quick-adc_amd/host/refine.hpp with metric
kIP through tests/cpp/refine_ip_host.cpp), and its compositions AdcIndex.search_exact, .search_exact_device and Index.search_exact:
an owned 8-bit index, an owned 16-bit index and a view of a 4-bit one; labels that repeat within a partition, across groups and
across launches, with R small enough that the copies alone would fill it; labels the store does not hold; ma = K against knn; both
filters.  The coarse step stays L2: search_exact under "ip" is assign, then knn_probed under "ip"."""
import numpy as np
import pytest

import refine_ip_cases as ic
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = (0, 1, 63, 300, 700, 200)
K = len(SIZES)
N = 1100                       # the keys the store holds; the partitions have sum(SIZES) = 1264 rows
DIM = 16


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return ic.build_driver()


def index8(pyqadc, parts):
    return ic.make_index(pyqadc, parts)


def index16(pyqadc, parts):
    rng = np.random.default_rng(1)
    idx = pyqadc.AdcIndex.create16(2)
    idx.add_partitions([rng.integers(0, 65536, (len(p), 2)).astype(np.uint16) for p in parts], list(parts))
    return idx


class View4:
    """a view of a finalized 4-bit index, closed with its source"""

    def __init__(self, pyqadc, parts, quantizers=None):
        rng = np.random.default_rng(2)
        self.src = pyqadc.Index(16)
        self.src.add_partitions([rng.integers(0, 256, (len(p), 8), dtype=np.uint8) for p in parts], list(parts))
        if quantizers is not None:
            self.src.set_pq(quantizers[0])
            self.src.set_coarse(quantizers[1])
        self.src.finalize(0.01)
        self.view = pyqadc.AdcIndex.view_of(self.src)
        self._h = self.view._h

    def close(self):
        self.view.close()
        self.src.close()


INDEXES = {"8-bit": index8, "16-bit": index16, "view-of-4-bit": View4}


def labels_with_repeats(rng, best):
    """sum(SIZES) labels: every key 0 .. N once, 60 keys above N (not held), 90 more rows of random held keys, and the key `best` in
    14 more rows — four in partition 4 (rows 0, 100, 400, 650: different launches under chunks of 64 rows), the rest in partitions 2,
    3 and 5 (other groups)"""
    n = sum(SIZES)
    plain = rng.permutation(np.concatenate([rng.permutation(N), N + 5 + np.arange(60), rng.integers(0, N, n - 14 - N - 60)]))
    parts = [p.copy() for p in ic.split(np.concatenate([plain, np.full(14, best)]).astype(np.uint32), SIZES)]
    assert (parts[5][-14:] == best).all()                                      # the copies: swapped to where they belong
    spots = [(4, 0), (4, 100), (4, 400), (4, 650), (2, 5), (2, 6), (2, 60), (3, 0), (3, 150), (3, 299), (5, 1), (5, 2), (5, 100), (5, 150)]
    for i, (p, r) in enumerate(spots):
        parts[5][-14 + i], parts[p][r] = parts[p][r], best
    return parts


def probed_case(rng, dtype, keyed, Rs=(5, 60), nq=9, filters=(None,)):
    vec = (rng.normal(size=(N, DIM))).astype(np.float32)
    q = rng.normal(size=(nq, DIM)).astype(np.float32)
    best = 777
    vec[best] = q[0] * np.float32(3.0)                                         # the largest score of query 0 by far
    parts = labels_with_repeats(rng, best)
    every = np.tile(np.arange(K, dtype=np.int32), (nq, 1))
    few = np.stack([rng.permutation(K)[:3] for _ in range(nq)]).astype(np.int32)
    few[0] = (4, 2, 4)                                                         # a repeated probe counts once
    ops = [ic.probed("ip", parts, a, q, R, f) for a in (every, few) for R in Rs for f in filters]
    labels = np.arange(N, dtype=np.uint32) if keyed else None
    return ic.case(DIM, dtype, vec, ops, labels=labels)


# every index kind over a dense store of every row type; the keyed store's lookup once per row type, on the owned 8-bit index
STORES = [(dtype, False, kind) for dtype in ("f32", "f16", "sq8") for kind in INDEXES] + [(dtype, True, "8-bit") for dtype in ("f32", "f16", "sq8")]


@path_independent
@pytest.mark.parametrize("dtype,keyed,kind", STORES, ids=["%s-%s-%s" % (t, "keyed" if k else "dense", i) for t, k, i in STORES])
def test_repeated_and_missing_labels_on_every_index_kind(pyqadc, twin, tmp_path, dtype, keyed, kind):
    rng = np.random.default_rng(4 + ic.DTYPES[dtype])
    c = probed_case(rng, dtype, keyed)
    (want,) = ic.run_twin(twin, tmp_path, [c])
    ic.assert_same(ic.run_store(pyqadc, c, plan=(64, 0), index_of=INDEXES[kind]), want, kind + ", chunks of 64 rows, host form")
    ic.assert_same(ic.run_store(pyqadc, c, device=True, plan=(64, 0), index_of=INDEXES[kind]), want, kind + ", chunks of 64 rows, device form")
    ic.assert_same(ic.run_store(pyqadc, c, device=True, index_of=INDEXES[kind]), want, kind + ", the default plan, device form")
    small = want[0]                                                            # ma = K, R = 5: the 15 rows of key 777 count once
    assert small["keys"][0, 0] == 777 and len(set(small["keys"][0].tolist())) == 5 and small["sizes"][0] == 5
    assert small["missing"] == 60 * 9                                          # per entry and query
    assert (np.diff(want[1]["dist"][0]) <= 0).all()


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "sq8"])
def test_every_partition_probed_is_knn_and_both_filters(pyqadc, twin, tmp_path, dtype):
    rng = np.random.default_rng(6)
    allow = ("allow", np.concatenate([rng.choice(N, 400, replace=False), [777, N + 7]]))
    exclude = ("exclude", np.concatenate([rng.choice(N, 400, replace=False), [777]]))
    c = probed_case(rng, dtype, False, Rs=(40,), filters=(None, allow, exclude, ("allow", [])))
    (want,) = ic.run_twin(twin, tmp_path, [c])
    ic.assert_same(ic.run_store(pyqadc, c, plan=(64, 0)), want, "chunks of 64 rows")
    ic.assert_same(ic.run_store(pyqadc, c, device=True), want, "the default plan, device form")
    q = c["ops"][0][4]
    knn = dict(c, ops=[ic.knn("ip", q, 40, f) for f in (None, allow, exclude, ("allow", []))])
    for i, (p, k) in enumerate(zip(want[:4], ic.run_store(pyqadc, knn))):       # ma = K: the exhaustive search under the same filter
        assert ic.same(dict(p, missing=0), k) is None, i
    assert np.isin(want[1]["keys"], allow[1]).all() and want[1]["missing"] == 9            # N + 7 is allowed and not held
    assert not np.isin(want[2]["keys"], exclude[1]).any() and want[2]["keys"][0, 0] != 777
    assert want[3]["sizes"].max() == 0 and want[3]["missing"] == 0


@path_independent
@pytest.mark.parametrize("ma", [1, 3, K])
def test_search_exact_under_ip_is_assign_then_knn_probed_under_ip(pyqadc, ma):
    rng = np.random.default_rng(7)
    c = probed_case(rng, "f32", False)
    parts = c["ops"][0][2]
    q = c["ops"][0][4]
    st = ic.make_store(pyqadc, c, metric="ip")
    idx = index8(pyqadc, parts)
    idx.set_pq(rng.normal(size=(8, 256, DIM // 8)).astype(np.float32))
    idx.set_coarse(rng.normal(size=(K, DIM)).astype(np.float32))

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    try:
        assign = idx.assign(q, ma)
        k, d, s, m, a = idx.search_exact(q, ma, 50, st)
        wk, wd, ws, wm = st.knn_probed(idx, q, assign, 50)
        want = dict(keys=wk, dist=wd, sizes=ws, missing=wm)
        assert np.array_equal(a, assign) and ic.same(dict(keys=k, dist=d, sizes=s, missing=m), want) is None
        dk, dd, ds, dm, da = idx.search_exact_device(dev(q), ma, 50, st)
        got = dict(keys=dk.cpu().numpy().view(np.uint32), dist=dd.cpu().numpy(), sizes=ds.cpu().numpy(), missing=dm)
        assert np.array_equal(da.cpu().numpy(), assign) and ic.same(got, want) is None
        assert (np.diff(wd[0, :ws[0]]) <= 0).all()                                     # scores, descending
        st.set_metric("l2")                                                            # the probes are the same under both metrics
        lk, ld, ls, lm, la = idx.search_exact(q, ma, 50, st)
        assert np.array_equal(la, assign) and (np.diff(ld[0, :ls[0]]) >= 0).all()
        if ma == K:
            assert not np.array_equal(lk, k)
            st.set_metric("ip")
            nk, nd, ns = st.knn(q, 50)
            assert ic.same(dict(keys=k, dist=d, sizes=s, missing=0), dict(keys=nk, dist=nd, sizes=ns, missing=0)) is None
    finally:
        idx.close()
        st.close()


@path_independent
def test_a_4_bit_index_searches_exactly_under_ip(pyqadc):
    rng = np.random.default_rng(8)
    c = probed_case(rng, "f16", False)
    parts = c["ops"][0][2]
    q = c["ops"][0][4]
    st = ic.make_store(pyqadc, c, metric="ip")
    v = View4(pyqadc, parts, (rng.normal(size=(16, 16, DIM // 16)).astype(np.float32), rng.normal(size=(K, DIM)).astype(np.float32)))
    try:
        k, d, s, m, a = v.src.search_exact(q, 2, 30, st)
        wk, wd, ws, wm = st.knn_probed(v.view, q, a, 30)
        assert ic.same(dict(keys=k, dist=d, sizes=s, missing=m), dict(keys=wk, dist=wd, sizes=ws, missing=wm)) is None
        k, d, s, m, a = v.src.search_exact(q, K, 30, st)
        nk, nd, ns = st.knn(q, 30)
        assert m == 60 * 9 and ic.same(dict(keys=k, dist=d, sizes=s, missing=0), dict(keys=nk, dist=nd, sizes=ns, missing=0)) is None
    finally:
        v.close()
        st.close()
