"""GPU: search, then exact re-ranking (AdcIndex.search_refined, .search_refined_device, Index.search_refined; DESIGN.md section
11.11) on a clustered 32-d set of 20 000 vectors: an 8x8 IVF index (K = 16, codebooks from train_pq), a float-ADC view of a 16x4
Index, a 4x16 index, and the 4-bit engine itself.  Every comparison is an equality with the host twin (tests/cpp/refine_host.cpp)."""
import numpy as np
import pytest

import refine_cases as rc
from helpers import path_independent

pytestmark = pytest.mark.gpu

DIM, N, K, NQ = 32, 20000, 16, 12


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return rc.build_driver()


class World:
    """the vectors, their quantizers and one store per element type"""

    def __init__(self, pyqadc):
        rng = np.random.default_rng(31)
        self.coarse = (rng.normal(size=(K, DIM)) * 2).astype(np.float32)
        self.vectors = (self.coarse[rng.integers(0, K, N)] + rng.normal(size=(N, DIM))).astype(np.float32)
        self.queries = (self.vectors[rng.integers(0, N, NQ)] + 0.3 * rng.normal(size=(NQ, DIM))).astype(np.float32)
        assign = pyqadc.coarse_assign(self.vectors, self.coarse, 1)[:, 0]
        resid = (self.vectors - self.coarse[assign]).astype(np.float32)
        self.cb8, _, empty8 = pyqadc.train_pq(self.vectors, pyqadc.pq_seed(resid, 8, 8, rng), 4, coarse=self.coarse)
        self.cb4, _, empty4 = pyqadc.train_pq(self.vectors, pyqadc.pq_seed(resid, 16, 4, rng), 4, coarse=self.coarse)
        assert empty8 == 0 and empty4 == 0
        # 65536 centroids per sub-quantizer have no learning set of 20 000 vectors: residual sub-vectors, jittered
        rows = resid[rng.integers(0, N, 65536)].reshape(65536, 4, 8).transpose(1, 0, 2)
        self.cb16 = np.ascontiguousarray(rows + 0.05 * rng.normal(size=rows.shape), np.float32)
        self.stores = {}
        for dtype in ("f32", "f16"):
            self.stores[dtype] = pyqadc.Refine(DIM, dtype)
            self.stores[dtype].add(self.vectors)
        self.pyqadc = pyqadc
        self.made, self.cache = [], {}

    def adc(self, shape):
        """an IVF float-ADC index over all vectors, keys = positions in self.vectors"""
        if shape not in self.cache:
            self.cache[shape] = self._adc(shape)
        return self.cache[shape]

    def _adc(self, shape):
        p = self.pyqadc
        if shape == "8x8":
            idx = p.AdcIndex(8, 8)
            idx.set_pq(self.cb8)
        elif shape == "4x16":
            idx = p.AdcIndex.create16(4)
            idx.set_pq(self.cb16)
        else:
            src = self.index4()
            src.finalize(0.01)
            idx = p.AdcIndex.view_of(src)
            self.made += [idx, src]
            return idx
        idx.set_coarse(self.coarse)
        idx.add_vectors(self.vectors, labels_offset=0)
        self.made.append(idx)
        return idx

    def index4(self, vectors=None):
        idx = self.pyqadc.Index(16)
        idx.set_pq(self.cb4)
        idx.set_coarse(self.coarse)
        idx.add_vectors(self.vectors if vectors is None else vectors, labels_offset=0)
        return idx

    def case(self, dtype, keys, R, counts=None, values=None, queries=None):
        return rc.case(DIM, dtype, [(0, self.vectors)], self.queries if queries is None else queries, keys, R, counts=counts, values=values)

    def close(self):
        for x in self.made + list(self.stores.values()):
            x.close()


@pytest.fixture(scope="module")
def world(pyqadc):
    w = World(pyqadc)
    yield w
    w.close()


def as_result(k, d, s, m):
    import torch
    if isinstance(k, torch.Tensor):
        k, d, s = k.cpu().numpy().view(np.uint32), d.cpu().numpy(), s.cpu().numpy()
    return dict(keys=k, dist=d, sizes=s, missing=m)


@path_independent
@pytest.mark.parametrize("shape", ["8x8", "16x4 view", "4x16"])
def test_search_refined_equals_the_twin_on_the_search_output(world, twin, tmp_path, shape):
    import torch
    idx = world.adc(shape)
    ma, R, r_in = 4, 100, 400
    keys, vals, sizes, _ = idx.search(world.queries, ma, r_in)
    assert (vals < rc.FLT_MAX).all(), "every heap is full: the case holds no sentinel"
    cases, gots = [], []
    for dtype in ("f32", "f16"):
        cases.append(world.case(dtype, keys, R, values=vals))
        gots.append(as_result(*idx.search_refined(world.queries, ma, R, r_in, world.stores[dtype])))
        dev = as_result(*idx.search_refined_device(torch.from_numpy(world.queries).cuda(), ma, R, r_in, world.stores[dtype]))
        assert rc.same(dev, gots[-1]) is None, "search_refined_device differs from search_refined (%s)" % dtype
    # one probe of a short list: the heaps keep FLT_MAX sentinels, which are no candidates
    k1, v1, _, _ = idx.search(world.queries, 1, 2000)
    assert (v1 == rc.FLT_MAX).any()
    cases.append(world.case("f32", k1, 2000, values=v1))
    gots.append(as_result(*idx.search_refined(world.queries, 1, 2000, 2000, world.stores["f32"])))
    for c, got, want in zip(cases, gots, rc.run_twin(twin, tmp_path, cases)):
        assert rc.same(got, want) is None
        assert want["missing"] == 0
    held = (v1 < rc.FLT_MAX).sum(1)
    assert np.array_equal(gots[-1]["sizes"], held) and (held < 2000).any()


@path_independent
def test_a_flat_index_refined_over_all_its_rows_is_brute_force(world, twin, tmp_path, pyqadc):
    n, R = 5000, 50
    idx = pyqadc.AdcIndex(8, 8)
    idx.set_pq(world.cb8)
    idx.add_vectors(world.vectors[:n], labels_offset=0)
    st = pyqadc.Refine(DIM, "f32")
    st.add(world.vectors[:n])
    got = as_result(*idx.search_refined(world.queries, 1, R, n, st))
    st.close()
    idx.close()
    everything = np.tile(np.arange(n, dtype=np.uint32), (NQ, 1))
    (want,) = rc.run_twin(twin, tmp_path, [rc.case(DIM, "f32", [(0, world.vectors[:n])], world.queries, everything, R)])
    assert rc.same(got, want) is None
    exact = ((world.queries[:, None, :].astype(np.float64) - world.vectors[None, :n].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(got["keys"][:, 0], exact.argmin(1))


@path_independent
@pytest.mark.parametrize("shape", ["8x8", "16x4 view", "4x16"])
def test_refining_never_lowers_the_recall(world, twin, tmp_path, shape):
    """ground truth: the whole database by (twin distance, key).  The unrefined list — the R entries of the r_in heap with the
    smallest ADC values, ties by key — is a subset of the candidates, and the refined list is the best R of them: it hits the truth
    at least as often, for every query"""
    idx = world.adc(shape)
    ma, R, r_in = 4, 100, 1000
    everything = np.tile(np.arange(N, dtype=np.uint32), (NQ, 1))
    (truth,) = rc.run_twin(twin, tmp_path, [world.case("f32", everything, R)])
    keys, vals, _, _ = idx.search(world.queries, ma, r_in)
    refined = as_result(*idx.search_refined(world.queries, ma, R, r_in, world.stores["f32"]))
    gains = []
    for q in range(NQ):
        live = vals[q] < rc.FLT_MAX
        k, v = keys[q][live], vals[q][live]
        plain = k[np.lexsort((k, v))][:R]
        want = set(truth["keys"][q].tolist())
        hit_plain, hit_refined = len(want & set(plain.tolist())), len(want & set(refined["keys"][q][:refined["sizes"][q]].tolist()))
        assert hit_refined >= hit_plain, (q, hit_plain, hit_refined)
        # the refined list is the truth restricted to the candidates
        cand = set(k.tolist())
        assert [x for x in truth["keys"][q].tolist() if x in cand] == [x for x in refined["keys"][q].tolist() if x in want]
        gains.append(hit_refined - hit_plain)
    assert sum(gains) > 0, "re-ranking changed nothing: the case is vacuous"


def test_the_4bit_engine_refined_keeps_key_0_once(world, twin, tmp_path, scan_path):
    """Index.search_refined: counts = sizes and no values.  A (0, 127) sentinel left in a heap is row 0 judged by its true distance;
    row 0's own hit and the sentinel are one key.

    Measured on this engine: qadc_search skips a query whose pre-scan holds fewer than r_in codes (status 1, sizes 0: the reference's
    "Max quantization bound too high"), so one probe of a list shorter than r_in refines to nothing, and with a pre-scan of at least
    r_in codes the R-th smallest of it bounds the quantizer, at least r_in codes are pushed and the sentinel is evicted.  The heaps
    that do keep it are those of the int8 scan with R above the list's length (scan_i8): their arrays go through rerank the way
    search_refined hands them over."""
    from helpers import rand_qtables
    idx = world.index4()
    idx.finalize(1.0)
    R = 100
    q = np.concatenate([world.queries[:3], world.vectors[:1]])               # the last query is row 0 itself: a real hit of key 0
    cases, gots = [], []
    for ma, r_in in ((1, 2000), (1, 1000), (4, 2000)):                       # (1, 2000): the probe list is shorter than r_in
        found = idx.search(q, ma, r_in)
        assert (found["sizes"] == (0 if (ma, r_in) == (1, 2000) else r_in)).all() and ((found["status"] == 0) == (found["sizes"] > 0)).all()
        for dtype in ("f32", "f16"):
            cases.append(world.case(dtype, found["keys"], R, counts=found["sizes"], queries=q))
            gots.append(as_result(*idx.search_refined(q, ma, R, r_in, world.stores[dtype])))
    assert not gots[0]["sizes"].any() and (gots[0]["keys"] == rc.NO_KEY).all()
    assert gots[2]["keys"][3, 0] == 0 and gots[2]["dist"][3, 0] == 0         # row 0 is its own nearest neighbour
    # heaps that keep the sentinel: the int8 scan of each query's nearest partition with R above its length
    probed = idx.search(q, 1, 10)["assign"][:, :1]
    r_in = 2000
    heaps = idx.scan_i8(probed, rand_qtables(np.random.default_rng(33), (len(q), 1), 16, 7), r_in)
    keys, sizes = np.zeros((len(q), r_in), np.uint32), np.zeros(len(q), np.int32)
    for i, (k, v) in enumerate(heaps):
        assert ((k == 0) & (v == 127)).sum() == 1 and idx.partition_size(int(probed[i, 0])) < len(k) < r_in   # (the scan's padding lanes repeat keys)
        keys[i, :len(k)], sizes[i] = k, len(k)
    assert (keys[3, :sizes[3]] == 0).sum() >= 2                              # the sentinel and row 0's own entry
    for dtype in ("f32", "f16"):
        cases.append(world.case(dtype, keys, R, counts=sizes, queries=q))
        gots.append(as_result(*world.stores[dtype].rerank(q, keys, R, counts=sizes)))
    idx.close()
    for got, want in zip(gots, rc.run_twin(twin, tmp_path, cases)):
        assert rc.same(got, want) is None and want["missing"] == 0
        for i in range(len(q)):
            assert (got["keys"][i, :got["sizes"][i]] == 0).sum() <= 1
    assert gots[-2]["keys"][3, 0] == 0 and (gots[-2]["sizes"] == R).all()


@path_independent
def test_a_filter_on_the_index_holds_for_the_refined_keys(world, twin, tmp_path, pyqadc):
    import torch
    idx = world.adc("8x8")
    rng = np.random.default_rng(32)
    allowed = np.sort(rng.permutation(N)[:N // 3]).astype(np.uint32)
    f = pyqadc.AdcFilter(allowed, "allow")
    idx.set_filter(f)
    try:
        keys, vals, _, _ = idx.search(world.queries, 4, 400)
        got = as_result(*idx.search_refined(world.queries, 4, 100, 400, world.stores["f32"]))
        dev = as_result(*idx.search_refined_device(torch.from_numpy(world.queries).cuda(), 4, 100, 400, world.stores["f32"]))
    finally:
        idx.set_filter(None)
        f.close()
    (want,) = rc.run_twin(twin, tmp_path, [world.case("f32", keys, 100, values=vals)])
    assert rc.same(got, want) is None and rc.same(dev, want) is None
    assert (got["sizes"] == 100).all() and np.isin(got["keys"], allowed).all()
    plain = as_result(*idx.search_refined(world.queries, 4, 100, 400, world.stores["f32"]))
    assert not np.isin(plain["keys"], allowed).all(), "the filter changed nothing: the case is vacuous"
