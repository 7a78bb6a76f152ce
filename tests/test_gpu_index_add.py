"""db_add on the 4-bit index (qadc_index_add_vectors, pyqadc.Index.add_vectors): vectors are encoded with
the quantizers the index holds and appended to its partitions in device memory, and the index grows.

Every comparison is for equality — the calls do no float arithmetic of their own.  The model is the stable grouping by `assign`
of what pyqadc.ivf_encode returns (the stateless encoder, pinned to the reference elsewhere): partition p = the codes of the
vectors assigned to p in input order, labels = labels_offset + i.  Partitions are looked at through read_partition.  kAddTile
(csrc/qadc_adc_kernels.h) is the number of vectors one workgroup of the dispatch ranks; the shapes sit on its edges, on the
256-partition edge of the radix digit and on the pass edge QADC_INDEX_ADD_CHUNK."""
import os
import re

import numpy as np
import pytest

import pyqadc
from helpers import float_tables, heaps_equal, path_independent
from test_gpu_adc_add import TILE, Quantizers, append, assert_partitions, group, raw_add, read_all

pytestmark = pytest.mark.gpu

CHUNK = pyqadc.QADC_INDEX_ADD_CHUNK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_TILE = int(re.search(r"constexpr uint32_t kSplitTile = (\d+);", open(os.path.join(ROOT, "quick-adc_amd", "host", "level_plan.hpp")).read()).group(1))
SHAPES = [(16, 32), (32, 64)]                                                    # (M, dim): rows of 8 and 16 bytes
SIZES = (1, TILE - 1, TILE, TILE + 1, 1000)


class Quantizers4(Quantizers):
    """test_gpu_adc_add.Quantizers (codebooks, K coarse centroids, a rotation, clustered vectors) for 4-bit sub-quantizers"""

    def __init__(self, M, dim, K=8, n=TILE + 1, seed=0):
        super().__init__(M, 4, dim, K=K, n=n, seed=seed)

    def index(self, opq=False, coarse=True):
        idx = pyqadc.Index(self.nsq)
        idx.set_pq(self.codebooks)
        if opq:
            idx.set_rotation(self.rotation)
        if coarse:
            idx.set_coarse(self.coarse)
        return idx

    def encode(self, vectors, opq=False, sum_mode=1, coarse=True):
        return pyqadc.ivf_encode(self.codebooks, vectors, self.coarse if coarse else None, self.rotation if opq else None, sum_mode=sum_mode)


_quantizers = {}


def quantizers(shape):
    if shape not in _quantizers:
        _quantizers[shape] = Quantizers4(*shape)
    return _quantizers[shape]


def build_from_model(q, model, opq=False):
    """the route without add_vectors: the grouped codes and labels through add_partitions"""
    idx = q.index(opq)
    idx.add_partitions([c for c, _ in model], [l for _, l in model])
    return idx


# ---- 1. parity, IVF ----------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=["16x4", "32x4"])
def test_partitions_equal_the_grouped_encoding(po, shape):
    q = quantizers(shape)
    opq, sum_mode = (True, 1) if shape[0] == 16 else (False, 0)                  # OPQ on one shape, the source-order sums on the other
    a, codes = q.encoded(opq, sum_mode)
    if shape[0] == 16:                                                           # the model itself against the oracle's encoder
        resid = (q.vectors - q.coarse[a]).astype(np.float32)
        assert np.array_equal(codes, po.pq_encode(q.codebooks, resid, q.rotation, form=1, sum_mode=sum_mode))
    assert len(np.unique(a)) == q.K, "a partition stays empty at n = kAddTile + 1"
    for n in SIZES:
        idx = q.index(opq)
        try:
            idx.add_vectors(q.vectors[:n], labels_offset=7, sum_mode=sum_mode)
            assert idx.partition_count() == q.K
            assert_partitions(read_all(idx), group(a[:n], codes[:n], q.K, 7), "n %d" % n)
            assert [idx.partition_size(p) for p in range(q.K)] == np.bincount(a[:n], minlength=q.K).tolist()
        finally:
            idx.close()


# ---- 2. partition edges ------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("K,n", [(1, TILE + 1), (257, TILE + 1), (300, 1000)], ids=["K1", "K257", "K300"])
def test_partition_counts_around_the_digit_edge(K, n):
    """K = 300 passes the 256-partition edge of one radix digit and leaves most partitions empty; K = 257 has one partition in
    the second digit"""
    q = Quantizers4(16, 16, K=K, n=n)
    a, codes = q.encoded()
    assert K == 1 or a.max() >= 256, "no vector beyond partition 255"
    idx = q.index()
    try:
        idx.add_vectors(q.vectors)
        assert_partitions(read_all(idx), group(a, codes, K))
    finally:
        idx.close()


# ---- 3. the pass edge --------------------------------------------------------------------------------------------------------

@path_independent
def test_one_vector_past_a_pass():
    q = Quantizers4(16, 16, n=CHUNK + 1, seed=6)
    a, codes = q.encoded()                                                       # one ivf_encode of the whole array
    idx = q.index()
    try:
        idx.add_vectors(q.vectors, labels_offset=11)
        model = group(a, codes, q.K, 11)
        assert_partitions(read_all(idx), model)
        assert model[a[CHUNK]][1][-1] == 11 + CHUNK                              # the second pass's one row stands last in its partition
    finally:
        idx.close()


# ---- 4. growth ---------------------------------------------------------------------------------------------------------------

GROWTH = [1, 1, 3, 1000]


@pytest.fixture(scope="module")
def growth_case():
    q = Quantizers4(16, 32, n=sum(GROWTH), seed=3)
    a, codes = q.encoded()
    return q, a, codes, group(a, codes, q.K)


def add_in_turn(idx, vectors, counts=GROWTH):
    at = 0
    for n in counts:
        idx.add_vectors(vectors[at:at + n], labels_offset=at)
        at += n


@path_independent
def test_appends_in_turn_equal_one_call(growth_case):
    q, a, codes, model = growth_case
    grown, once = q.index(), q.index()
    try:
        add_in_turn(grown, q.vectors)
        once.add_vectors(q.vectors)
        assert grown.relocations() > 0
        assert_partitions(read_all(grown), model, "appended in turn")
        assert_partitions(read_all(once), model, "one call")
    finally:
        grown.close()
        once.close()


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
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=["16x4", "32x4"])
def test_a_call_split_at_every_position(shape):
    q = quantizers(shape)
    a, codes = q.encoded()
    model = group(a[:9], codes[:9], q.K)
    for cut in range(10):
        idx = q.index()
        try:
            add_in_turn(idx, q.vectors[:9], [cut, 9 - cut])
            assert_partitions(read_all(idx), model, "split at %d" % cut)
        finally:
            idx.close()


# ---- 5. consolidation: add_vectors on top of add_partitions -------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=["16x4", "32x4"])
def test_add_vectors_on_top_of_add_partitions(shape):
    q = quantizers(shape)
    a, codes = q.encoded()
    half, empty = 500, 3
    keep = np.flatnonzero(a[:half] != empty)                                     # partition 3 starts empty
    first = group(a[keep], codes[keep], q.K)
    first = [(c, (keep[l] + 100000).astype(np.uint32)) for c, l in first]        # labels of their own
    assert len(first[empty][0]) == 0 and all(len(c) for p, (c, _) in enumerate(first) if p != empty)
    idx = build_from_model(q, first)
    try:
        assert_partitions(read_all(idx), first, "add_partitions, read back")     # read_partition works however the rows came
        idx.add_vectors(q.vectors[half:], labels_offset=half)
        want = append(first, group(a[half:], codes[half:], q.K, half))
        assert len(want[empty][0]) > 0
        assert_partitions(read_all(idx), want)
        for p in range(q.K):
            assert np.array_equal(idx.read_codes(p, 0, idx.partition_size(p)), want[p][0])
        assert idx.relocations() == 1
    finally:
        idx.close()


# ---- 6. flat -----------------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=["16x4", "32x4"])
def test_flat_add_vectors_writes_rows_at_the_offset(shape):
    """flat_db::add_vectors (databases.hpp:136-156) on a numpy model: resize to max(size, offset + count), rows at offset + i"""
    q = quantizers(shape)
    _, codes = q.encode(q.vectors[:200], coarse=False)
    idx = q.index(coarse=False)
    model = np.zeros((0, q.nsq // 2), np.uint8)

    def step(vectors, at, enc):
        nonlocal model
        if vectors is None:
            raw_add(idx, None, 0, at, 1)
        else:
            idx.add_vectors(vectors, labels_offset=at)
        grown = np.zeros((max(len(model), at + len(enc)), q.nsq // 2), np.uint8)
        grown[:len(model)] = model
        grown[at:at + len(enc)] = enc
        model = grown
        got, labels = idx.read_partition(0)
        assert labels is None and idx.partition_count() == 1
        assert_partitions([(got, None)], [(model, None)], "after the rows at %d" % at)

    try:
        step(q.vectors[:101], 0, codes[:101])
        step(q.vectors[101:150], 201, codes[101:150])                            # a gap of zero rows
        assert not model[101:201].any() and model[201:250].any()
        step(q.vectors[150:181], 90, codes[150:181])                             # rows that exist are overwritten
        step(None, 401, codes[:0])                                               # count 0, an offset beyond the size
        assert idx.partition_size(0) == 401 and not model[250:].any()
    finally:
        idx.close()


# ---- 7. device input ---------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("kind", ["ivf-opq", "flat"])
def test_add_vectors_device_equals_add_vectors(kind):
    import torch
    q = quantizers((16, 32))
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


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------

def refused(idx, match, f, *args):
    before = read_all(idx)
    with pytest.raises(pyqadc.QadcError, match=match):
        f(*args)
    assert_partitions(read_all(idx), before, "after the refused call")


@path_independent
def test_refusals_leave_the_index_as_it_was():
    import torch
    q = quantizers((16, 32))
    a, codes = q.encoded()
    v = q.vectors

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
        ivf.set_coarse(q.coarse)
        # a busy slot
        ivf.finalize(0.5)
        tables = float_tables(np.random.default_rng(1), 1, 1, 16)
        ivf.submit(0, np.zeros((1, 1), np.int32), tables, 10)
        refused(ivf, "not been collected", ivf.add_vectors, v[50:60], 50)
        refused(ivf, "not been collected", ivf.reserve, [100] * q.K)
        ivf.collect(0)
        # under the multi-GPU merge (one process standing in for a world of one)
        ivf.dist_init_loopback(0, 1)
        refused(ivf, "multi-GPU", ivf.add_vectors, v[50:60], 50)
        ivf.dist_shutdown()
        ivf.add_vectors(v[50:100], labels_offset=50)                             # the good call: the index is usable
        assert_partitions(read_all(ivf), group(a[:100], codes[:100], q.K))
    finally:
        ivf.close()

    many = q.index(coarse=False)                                                 # no coarse quantizer, more than one partition
    try:
        many.add_partitions([codes[:20], codes[20:30]])
        refused(many, "one partition", many.add_vectors, v[:10])
    finally:
        many.close()

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

    bare = pyqadc.Index(16)                                                      # no set_pq
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

    shard = q.index(coarse=False)                                                # a shard with a starts replica
    try:
        shard.add_partition_shard(codes[16:48], 16, 64, starts=codes[:8])
        with pytest.raises(pyqadc.QadcError, match="shard"):
            shard.add_vectors(v[:10])
        with pytest.raises(pyqadc.QadcError, match="shard"):
            shard.read_partition(0, 0, 1)
        assert shard.partition_size(0) == 32 and np.array_equal(shard.read_codes(0, 0, 32), codes[16:48])
    finally:
        shard.close()

    lent = q.index(coarse=False)                                                 # a borrowed partition
    try:
        t = torch.from_numpy(codes[:64].copy()).to("cuda:0")
        lent.add_partition_device(t.data_ptr(), 64, keepalive=t)
        refused(lent, "borrowed", lent.add_vectors, v[:10])
        refused(lent, "borrowed", lent.reserve, [100])
        assert np.array_equal(lent.read_partition(0)[0], codes[:64])             # (held whole: readable)
    finally:
        lent.close()


@path_independent
def test_a_live_view_refuses_growth_and_a_new_view_sees_it():
    q = quantizers((16, 32))
    a, codes = q.encoded()
    idx = q.index()
    try:
        idx.add_vectors(q.vectors[:500])
        idx.finalize(0.01)
        view = pyqadc.AdcIndex.view_of(idx)
        try:
            refused(idx, "view", idx.add_vectors, q.vectors[500:600], 500)
            refused(idx, "view", idx.reserve, [1000] * q.K)
            assert [view.partition_size(p) for p in range(q.K)] == np.bincount(a[:500], minlength=q.K).tolist()
        finally:
            view.close()
        idx.add_vectors(q.vectors[500:], labels_offset=500)
        idx.finalize(0.01)
        view = pyqadc.AdcIndex.view_of(idx)
        try:
            assert [view.partition_size(p) for p in range(q.K)] == np.bincount(a, minlength=q.K).tolist()
        finally:
            view.close()
        assert_partitions(read_all(idx), group(a, codes, q.K))
    finally:
        idx.close()


@path_independent
def test_a_move_of_the_partitions_asks_for_finalize_again():
    """whatever replaces the storage invalidates what finalize recorded of it (the partition table, the byte-plane copies): a
    reserve that relocates does, one that changes nothing does not"""
    q = quantizers((16, 32))
    a, codes = q.encoded()
    idx = build_from_model(q, group(a[:500], codes[:500], q.K))
    queries = q.vectors[:4]
    try:
        idx.finalize(0.5)
        idx.search(queries, 2, 10)
        idx.reserve([1000] * q.K)                                                # consolidates: the partitions move into the arena
        with pytest.raises(pyqadc.QadcError, match="finalize"):
            idx.search(queries, 2, 10)
        idx.finalize(0.5)
        want = idx.search(queries, 2, 10)
        idx.reserve([10] * q.K)                                                  # nothing to do: still finalized
        got = idx.search(queries, 2, 10)
        assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["sizes"], want["sizes"])
        assert_partitions(read_all(idx), group(a[:500], codes[:500], q.K))
    finally:
        idx.close()


# ---- 9. queries see the new rows (through every scan path) ---------------------------------------------------------------------

def test_search_after_add_vectors_equals_search_after_add_partitions():
    n, ma, R, nq, keep = 3000, 4, 100, 16, 0.5                                    # (keep: the pre-scanned starts of four partitions fill a heap of R)
    q = Quantizers4(16, 32, n=n, seed=4)
    a, codes = q.encoded()
    rng = np.random.default_rng(44)
    queries = (q.coarse[rng.integers(0, q.K, nq)] + rng.normal(size=(nq, q.dim))).astype(np.float32)
    grown, built = q.index(), build_from_model(q, group(a, codes, q.K))
    try:
        add_in_turn(grown, q.vectors, [700, 1, n - 701])
        assert grown.relocations() >= 2
        grown.finalize(keep)
        built.finalize(keep)
        got, want = grown.search(queries, ma, R), built.search(queries, ma, R)
        assert (want["status"] == 0).all() and (want["sizes"] > 0).all()
        for name in ("keys", "values", "sizes", "assign", "status"):
            assert np.array_equal(got[name], want[name]), name
    finally:
        grown.close()
        built.close()


def test_split_scan_after_add(po):
    """one code past a byte-plane tile: finalize builds the copy of a partition that lives in the arena, and the split scan reads
    it"""
    n, R, keep = SPLIT_TILE + 1, 100, 0.01
    q = Quantizers4(16, 16, K=0, n=n, seed=8)
    idx = q.index(coarse=False)
    try:
        for k, v in dict(share_variant=0, mq=0, front_run_max=0, wgq=0).items():   # one query per pass: the launches that read the copy
            idx.set_option(k, v)
        idx.set_split(1, 1)
        idx.add_vectors(q.vectors)
        idx.finalize(keep)
        assert idx.profile()["split_copy_bytes"] == 2 * 7 * SPLIT_TILE
        codes, labels = idx.read_partition(0)
        assert labels is None and len(codes) == n and np.array_equal(codes, q.encode(q.vectors, coarse=False)[1])
        tables = float_tables(np.random.default_rng(5), 3, 1, 16)
        res = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
        for i in range(3):
            want = po.query_scan(16, [codes], None, keep, [0], tables[i].copy(), R)
            assert want["rc"] == res["status"][i] == 0
            assert heaps_equal((res["keys"][i, :res["sizes"][i]], res["values"][i, :res["sizes"][i]]), (want["keys"], want["values"])), i
    finally:
        idx.close()
