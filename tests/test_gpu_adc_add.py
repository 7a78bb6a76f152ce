"""db_add on the GPU (qadc_adc_index_add_vectors, pyqadc.AdcIndex.add_vectors): vectors are encoded and
appended to the partitions of an owned float-ADC index in device memory, and the index grows.

Two models, both compared for equality — the calls do no float arithmetic of their own:
  * the stable grouping by `assign` of what pyqadc.adc_encode / adc_encode16 return (the stateless encoders, pinned to the
    reference elsewhere): partition p = the codes of the vectors assigned to p in input order, labels = labels_offset + i;
  * for the 8-bit shapes also the oracle composition tests/adc_compose.py::encode.
Partitions are looked at through read_partition.  kAddTile (csrc/qadc_adc_kernels.h) is the number of vectors one workgroup of
the dispatch ranks; the shapes sit on its edges and on the 256-partition edge of the radix digit."""
import os
import re

import numpy as np
import pytest

import adc_compose as ac
import pyqadc
from helpers import path_independent
from test_gpu_adc import assert_heap, expected

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"constexpr int kAddTile = (\d+);", open(os.path.join(ROOT, "quick-adc_amd", "csrc", "qadc_adc_kernels.h")).read()).group(1))
CHUNK = pyqadc.QADC_ADC_ADD_CHUNK
# (nsq, bits, dim): rows of 4, 8 and 16 bytes of both encoders
SHAPES = [(4, 8, 16), (8, 8, 64), (16, 8, 32), (2, 16, 16), (4, 16, 64), (8, 16, 16)]


def shape_id(s):
    return "%dx%d-d%d" % s


class Quantizers:
    """One shape's codebooks, K coarse centroids, a rotation and clustered vectors; the stateless encoders' answers are computed
    once per (n, opq, sum_mode) and shared"""

    def __init__(self, nsq, bits, dim, K=8, n=TILE + 1, seed=0):
        rng = np.random.default_rng(5000 + 100 * nsq + bits + dim + 7 * K + seed)
        self.nsq, self.bits, self.dim, self.K = nsq, bits, dim, K
        self.codebooks = rng.standard_normal((nsq, 1 << bits, dim // nsq), dtype=np.float32)
        self.coarse = (rng.normal(size=(K, dim)) * 2).astype(np.float32) if K else None
        self.rotation = ac.random_rotation(rng, dim)
        self.vectors = rng.normal(size=(n, dim)).astype(np.float32)
        if K:
            self.vectors += self.coarse[rng.integers(0, K, n)]
        self.cache = {}

    def index(self, opq=False, coarse=True):
        idx = pyqadc.AdcIndex(self.nsq, 8) if self.bits == 8 else pyqadc.AdcIndex.create16(self.nsq)
        idx.set_pq(self.codebooks)
        idx.set_rotation(self.rotation if opq else None)
        idx.set_coarse(self.coarse if coarse else None)
        return idx

    def encode(self, vectors, opq=False, sum_mode=1, coarse=True):
        f = pyqadc.adc_encode if self.bits == 8 else pyqadc.adc_encode16
        return f(self.codebooks, vectors, self.coarse if coarse else None, self.rotation if opq else None, sum_mode=sum_mode)

    def encoded(self, opq=False, sum_mode=1):
        """(assign, codes) of all of self.vectors: every vector is encoded on its own, so a shorter call returns a prefix"""
        key = (opq, sum_mode)
        if key not in self.cache:
            self.cache[key] = self.encode(self.vectors, opq, sum_mode)
        return self.cache[key]


_quantizers = {}


def quantizers(shape):
    if shape not in _quantizers:
        _quantizers[shape] = Quantizers(*shape)
    return _quantizers[shape]


def group(assign, codes, K, labels_offset=0):
    """the model: [(codes of partition p in input order, their labels)]"""
    order = np.argsort(assign, kind="stable")
    bounds = np.searchsorted(assign[order], np.arange(K + 1))
    return [(codes[order[bounds[k]:bounds[k + 1]]], (order[bounds[k]:bounds[k + 1]] + labels_offset).astype(np.uint32)) for k in range(K)]


def append(model, more):
    return [(np.concatenate([c0, c1]), np.concatenate([l0, l1])) for (c0, l0), (c1, l1) in zip(model, more)]


def read_all(idx):
    return [idx.read_partition(p) for p in range(idx.partition_count())]


def assert_partitions(got, want, what=""):
    assert len(got) == len(want), "%s: %d partitions, expected %d" % (what, len(got), len(want))
    for p, ((gc, gl), (wc, wl)) in enumerate(zip(got, want)):
        assert gc.shape == wc.shape and gc.dtype == wc.dtype, "%s: partition %d holds %s %s, expected %s %s" % (what, p, gc.shape, gc.dtype, wc.shape, wc.dtype)
        assert np.array_equal(gc, wc), "%s: the codes of partition %d differ (first row %d)" % (what, p, np.argwhere((gc != wc).any(axis=1))[0, 0])
        if wl is None:
            assert gl is None, "%s: partition %d has labels" % (what, p)
        else:
            assert gl is not None and np.array_equal(gl, wl), "%s: the labels of partition %d differ" % (what, p)


def raw_add(idx, vectors, count, labels_offset, sum_mode):
    v = None if vectors is None else np.ascontiguousarray(vectors, np.float32)
    idx.add_vectors_raw(v, count, labels_offset, sum_mode)


# ---- 1. parity, IVF ----------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_partitions_equal_the_grouped_encoding(po, shape):
    q = quantizers(shape)
    # OPQ and the source-order sums on one 8-bit and one 16-bit shape each
    variants = [(False, 1)] + {(8, 8, 64): [(True, 1)], (2, 16, 16): [(True, 1)], (4, 8, 16): [(False, 0)], (4, 16, 64): [(False, 0)]}.get(shape, [])
    for opq, sum_mode in variants:
        a, codes = q.encoded(opq, sum_mode)
        if q.bits == 8:                                                          # the model itself against the oracle
            want_a, want_c = ac.encode(po, q.codebooks, q.vectors, q.coarse, q.rotation if opq else None, sum_mode)
            assert np.array_equal(a, want_a.reshape(-1)) and np.array_equal(codes, want_c)
        assert len(np.unique(a)) == q.K, "a partition stays empty at n = kAddTile + 1"
        for n in (1, TILE - 1, TILE, TILE + 1, 1000):
            idx = q.index(opq)
            try:
                idx.add_vectors(q.vectors[:n], labels_offset=7, sum_mode=sum_mode)
                assert idx.partition_count() == q.K
                assert_partitions(read_all(idx), group(a[:n], codes[:n], q.K, 7), "n %d opq %d sum_mode %d" % (n, opq, sum_mode))
                assert [idx.partition_size(p) for p in range(q.K)] == np.bincount(a[:n], minlength=q.K).tolist()
            finally:
                idx.close()


# ---- 2. partition edges ------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("K,n", [(1, TILE + 1), (300, 1000), (257, TILE + 1)], ids=["K1", "K300", "K257"])
def test_partition_counts_around_the_digit_edge(K, n):
    """K = 300 passes the 256-partition edge of one radix digit and leaves most partitions empty; K = 257 has one partition in
    the second digit"""
    q = Quantizers(4, 8, 16, K=K, n=n)
    a, codes = q.encoded()
    assert K == 1 or a.max() >= 256, "no vector beyond partition 255"
    idx = q.index()
    try:
        idx.add_vectors(q.vectors)
        assert_partitions(read_all(idx), group(a, codes, K))
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("shape", [(4, 8, 16), (8, 16, 16)], ids=shape_id)
@pytest.mark.parametrize("target", ["first", "last"])
def test_every_vector_in_one_partition(shape, target):
    """kAddTile + 1 vectors with one assignment: every rank of a tile, and the carry into the next"""
    q = quantizers(shape)
    p = 0 if target == "first" else q.K - 1
    rng = np.random.default_rng(77 + p)
    vectors = (q.coarse[p] + np.float32(0.01) * rng.normal(size=(TILE + 1, q.dim))).astype(np.float32)
    a, codes = q.encode(vectors)
    assert (a == p).all()
    idx = q.index()
    try:
        idx.add_vectors(vectors, labels_offset=3)
        assert_partitions(read_all(idx), group(a, codes, q.K, 3))
        assert np.array_equal(idx.read_partition(p)[1], np.arange(3, TILE + 4, dtype=np.uint32))
    finally:
        idx.close()


# ---- 3. growth ---------------------------------------------------------------------------------------------------------------

GROWTH = [1, 2, 5, 300, 5000]


@pytest.fixture(scope="module")
def growth_case():
    q = Quantizers(8, 8, 64, n=sum(GROWTH), seed=3)
    a, codes = q.encoded()
    return q, a, codes, group(a, codes, q.K)


def add_in_turn(idx, vectors):
    at = 0
    for n in GROWTH:
        idx.add_vectors(vectors[at:at + n], labels_offset=at)
        at += n


@path_independent
def test_appends_in_turn_equal_one_call(growth_case):
    q, a, codes, model = growth_case
    grown, once, built = q.index(), q.index(), q.index()
    try:
        add_in_turn(grown, q.vectors)
        once.add_vectors(q.vectors)
        built.add_partitions([c for c, _ in model], [l for _, l in model])
        assert grown.relocations() > 0
        assert_partitions(read_all(grown), model, "appended in turn")
        assert_partitions(read_all(once), model, "one call")
        assert_partitions(read_all(built), model, "add_partitions, read back")
    finally:
        for idx in (grown, once, built):
            idx.close()


@path_independent
def test_a_reserved_index_never_relocates(growth_case):
    q, a, codes, model = growth_case
    idx = q.index()
    try:
        idx.reserve(np.bincount(a, minlength=q.K))
        assert idx.partition_count() == q.K and idx.partition_size(0) == 0
        add_in_turn(idx, q.vectors)
        assert idx.relocations() == 0
        assert_partitions(read_all(idx), model)
        idx.reserve([1] * q.K)                                                   # a smaller request shrinks nothing
        idx.add_vectors(q.vectors[:1], labels_offset=9000)
        assert idx.relocations() <= 1                                            # (full, but for the rows a 16-byte region rounds up to)
        assert_partitions(read_all(idx), append(model, group(a[:1], codes[:1], q.K, 9000)))
    finally:
        idx.close()


@path_independent
def test_add_vectors_on_top_of_add_partitions(growth_case):
    q, a, codes, model = growth_case
    half = 2000
    first = group(a[:half], codes[:half], q.K)
    idx = q.index()
    try:
        idx.add_partitions([c for c, _ in first], [l for _, l in first])
        idx.add_vectors(q.vectors[half:], labels_offset=half)
        assert_partitions(read_all(idx), model)
        assert idx.relocations() == 1
    finally:
        idx.close()


# ---- 4. queries see the new rows ---------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(8, 8, 64), (2, 16, 16)], ids=shape_id)
def test_search_sees_what_add_vectors_appended(po, shape):
    nsq, bits, dim = shape
    n, ma, R, nq = 5000, 3, 100, 5
    q = Quantizers(nsq, bits, dim, n=n, seed=4)
    a, codes = q.encoded()
    rng = np.random.default_rng(44)
    queries = (q.coarse[rng.integers(0, q.K, nq)] + rng.normal(size=(nq, dim))).astype(np.float32)
    first = 3000                                                                 # checked once before and once after a relocation
    got, ref = q.index(), None
    try:
        for upto in (first, n):
            got.add_vectors(q.vectors[0 if upto == first else first:upto], labels_offset=0 if upto == first else first)
            model = group(a[:upto], codes[:upto], q.K)
            ref = q.index()
            ref.add_partitions([c for c, _ in model], [l for _, l in model])
            for finish in (0, 1):
                got.set_finish(finish)
                ref.set_finish(finish)
                res, want = got.search(queries, ma, R), ref.search(queries, ma, R)
                for x, y in zip(res, want):
                    assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), \
                        "search differs after %d vectors, finish %d" % (upto, finish)
            import torch
            tq = torch.from_numpy(queries).to("cuda:0")
            dres, dwant = got.search_device(tq, ma, R), ref.search_device(tq, ma, R)
            for x, y in zip(dres, dwant):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "search_device differs after %d vectors" % upto
            if bits == 8:                                                        # and the oracle's heap, composed as test_gpu_adc_search.py does
                keys, vals, sizes, got_a = res
                want_a = ac.assign(po, queries, q.coarse, ma)
                assert np.array_equal(got_a, want_a)
                tables = ac.tables(po, q.codebooks, ac.residuals(queries, q.coarse, want_a), 2)
                for i in range(nq):
                    want_heap = expected(po, nsq, [model[k][0] for k in want_a[i]], [model[k][1] for k in want_a[i]], tables[i], R)
                    assert_heap((keys, vals, sizes), want_heap, i, "after %d vectors" % upto)
            ref.close()
            ref = None
        assert got.relocations() == 2
    finally:
        got.close()
        if ref is not None:
            ref.close()


# ---- 5. flat -----------------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(8, 8, 64), (4, 16, 64)], ids=shape_id)
def test_flat_add_vectors_writes_rows_at_the_offset(shape):
    """flat_db::add_vectors (databases.hpp:136-156) on a numpy model: resize to max(size, offset + count), rows at offset + i"""
    q = quantizers(shape)
    _, codes = q.encode(q.vectors[:200], coarse=False)
    idx = q.index(coarse=False)
    model = np.zeros((0, q.nsq), codes.dtype)

    def step(vectors, at, enc):
        nonlocal model
        if vectors is None:
            raw_add(idx, None, 0, at, 1)
        else:
            idx.add_vectors(vectors, labels_offset=at)
        grown = np.zeros((max(len(model), at + len(enc)), q.nsq), codes.dtype)
        grown[:len(model)] = model
        grown[at:at + len(enc)] = enc
        model = grown
        got, labels = idx.read_partition(0)
        assert labels is None and idx.partition_count() == 1
        assert_partitions([(got, None)], [(model, None)], "after the rows at %d" % at)

    try:
        step(q.vectors[:100], 0, codes[:100])
        step(q.vectors[100:150], 200, codes[100:150])
        assert not model[100:200].any() and model[200:250].any()
        step(q.vectors[150:180], 90, codes[150:180])
        step(None, 400, codes[:0])
        assert idx.partition_size(0) == 400
        # keys are positions
        table = np.zeros((1, 1, idx.table_dim), np.float32)
        table[0, 0, :] = 1.0
        for m in range(q.nsq):
            table[0, 0, m * idx.centroids + int(model[230, m])] = 0.0
        keys, vals, sizes = idx.query_scan(np.zeros((1, 1), np.int32), table, 1)
        assert sizes[0] == 1 and vals[0, 0] == 0.0 and (model[keys[0, 0]] == model[230]).all()
        assert keys[0, 0] == np.flatnonzero((model == model[230]).all(axis=1))[0]
    finally:
        idx.close()


# ---- 6. the pass size shows in no result -------------------------------------------------------------------------------------

@path_independent
def test_pass_size_independence():
    n = CHUNK + 3
    q = Quantizers(4, 8, 8, n=n, seed=6)
    a, codes = q.encoded()
    whole, part = q.index(), q.index()
    try:
        whole.add_vectors(q.vectors, labels_offset=11)
        model = group(a, codes, q.K, 11)
        assert_partitions(read_all(whole), model)
        for p in range(q.K):                                                     # rows past the pass edge exist in every partition
            assert (model[p][1] >= 11 + CHUNK).any() or p not in a[CHUNK:]
        # the first 1000 rows of every partition's new part = those of an index given only the vectors that feed them
        feed = max(int(model[p][1][:1000].max()) - 11 + 1 for p in range(q.K))
        part.add_vectors(q.vectors[:feed], labels_offset=11)
        for p in range(q.K):
            gc, gl = part.read_partition(p, 0, min(1000, part.partition_size(p)))
            assert np.array_equal(gc, model[p][0][:1000]) and np.array_equal(gl, model[p][1][:1000])
    finally:
        whole.close()
        part.close()


# ---- 7. device input ---------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(16, 8, 32), (2, 16, 16)], ids=shape_id)
@pytest.mark.parametrize("kind", ["ivf-opq", "flat"])
def test_add_vectors_device_equals_add_vectors(shape, kind):
    import torch
    q = quantizers(shape)
    host, dev = (q.index(opq=kind == "ivf-opq", coarse=kind != "flat") for _ in range(2))
    try:
        t = torch.from_numpy(q.vectors).to("cuda:0")
        for lo, hi, at in ((0, 10, 0), (10, TILE + 1, 10)):
            host.add_vectors(q.vectors[lo:hi], labels_offset=at)
            dev.add_vectors_device(t[lo:hi], labels_offset=at)
        want = read_all(host)
        assert sum(len(c) for c, _ in want) == TILE + 1
        assert_partitions(read_all(dev), want)
        with pytest.raises(TypeError):
            dev.add_vectors_device(q.vectors[:4])
    finally:
        host.close()
        dev.close()


# ---- 8. NaN and infinite vectors ---------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(8, 8, 64), (2, 16, 16), (8, 16, 16)], ids=shape_id)
def test_nan_and_infinite_vectors(po, shape):
    nsq, bits, dim = shape
    q = quantizers(shape)
    v = q.vectors[:7].copy()
    v[0, 3] = np.nan
    v[1, dim - 1] = np.inf
    v[2, :] = -np.inf
    v[3, 0] = np.inf
    v[3, dim // nsq] = -np.inf
    v[4, :] = np.nan
    a, codes = q.encode(v)
    if bits == 8:
        want_a, want_c = ac.encode(po, q.codebooks, v, q.coarse)
        assert np.array_equal(a, want_a.reshape(-1)) and np.array_equal(codes, want_c)
    idx = q.index()
    try:
        idx.add_vectors(v, labels_offset=100)
        assert_partitions(read_all(idx), group(a, codes, q.K, 100))
        assert sum(idx.partition_size(p) for p in range(q.K)) == 7
    finally:
        idx.close()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------

@path_independent
def test_refusals_leave_the_index_as_it_was(po):
    q = quantizers((8, 8, 64))
    a, codes = q.encoded()
    v = q.vectors

    def refused(idx, match, f, *args):
        before = read_all(idx)
        with pytest.raises(pyqadc.QadcError, match=match):
            f(*args)
        assert_partitions(read_all(idx), before, "after the refused call")

    ivf = q.index()
    try:
        ivf.add_vectors(v[:50])
        refused(ivf, "sum_mode", raw_add, ivf, v[50:60], 10, 50, 2)
        refused(ivf, "2\\^32 - 1", raw_add, ivf, v[50:53], 3, 2 ** 32 - 2, 1)
        refused(ivf, "vectors is null", raw_add, ivf, None, 3, 50, 1)
        refused(ivf, "outside partition", ivf.read_partition, 0, ivf.partition_size(0), 1)
        refused(ivf, "does not exist", ivf.read_partition, q.K, 0, 0)
        ivf.set_coarse(q.coarse[:5])                                             # partition count != K
        refused(ivf, "5 centroids and the index 8 partitions", ivf.add_vectors, v[50:60], 50)
        ivf.set_coarse(None)                                                     # a labelled index without a coarse quantizer
        refused(ivf, "more than|one partition", ivf.add_vectors, v[50:60], 50)
        ivf.set_coarse(q.coarse)
        ivf.add_vectors(v[50:100], labels_offset=50)                             # the good call
        assert_partitions(read_all(ivf), group(a[:100], codes[:100], q.K))
    finally:
        ivf.close()

    one = q.index(coarse=False)                                                  # one labelled partition, no coarse quantizer
    try:
        one.add_partitions([codes[:20]], [np.arange(20, dtype=np.uint32)])
        refused(one, "labelled", one.add_vectors, v[:10])
        assert one.partition_size(0) == 20
    finally:
        one.close()

    unl = q.index()                                                              # unlabelled non-empty partitions, a coarse quantizer
    try:
        unl.add_partitions([codes[k:k + 3] for k in range(q.K)])
        refused(unl, "unlabelled", unl.add_vectors, v[:10])
    finally:
        unl.close()

    bare = pyqadc.AdcIndex(8, 8)                                                 # no set_pq
    try:
        with pytest.raises(pyqadc.QadcError, match="set_pq"):
            raw_add(bare, v[:4], 4, 0, 1)
        assert bare.partition_count() == 0
        bare.set_pq(q.codebooks)
        bare.set_coarse(q.coarse)
        bare.add_vectors(v[:100])
        assert_partitions(read_all(bare), group(a[:100], codes[:100], q.K))
    finally:
        bare.close()

    src = pyqadc.Index(16, 0)                                                    # a view
    try:
        src.add_partitions([np.zeros((64, 8), np.uint8)])
        src.finalize(0.01)
        view = pyqadc.AdcIndex.view_of(src)
        try:
            for f, args in ((view.add_vectors_raw, (np.zeros((1, 16), np.float32), 1, 0, 1)), (view.reserve, ([4],)),
                            (view.read_partition, (0, 0, 1))):
                with pytest.raises(pyqadc.QadcError, match="view"):
                    f(*args)
            assert view.partition_size(0) == 64
        finally:
            view.close()
    finally:
        src.close()
