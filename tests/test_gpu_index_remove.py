"""Remove by label on the 4-bit index (qadc_index_remove_labels, pyqadc.Index.remove_labels): the rows
whose label is in the caller's list leave their partitions in device memory — allocations of their own as add_partitions left
them, or regions of the arena after a reserve — and the others keep their order.

Every comparison is for equality.  The model is numpy: partition p keeps codes[~np.isin(labels, removed)], in order; read_partition
is compared against it, and every query call after finalize(keep) against a fresh index built from the model's partitions and
finalized with the same keep — which is what shows that the start sizes and the zeroed bytes behind an odd number of 8-byte rows
are right.  kRemoveTile (csrc/qadc_adc_kernels.h) is the number of rows one iteration of the compaction holds in registers."""
import numpy as np
import pytest

import pyqadc
from helpers import float_tables, heaps_equal, path_independent, rand_codes, rand_qtables
from test_gpu_adc_add import assert_partitions, read_all
from test_gpu_adc_remove import PATTERNS, T, check, model_remove
from test_gpu_index_add import SPLIT_TILE, Quantizers4

pytestmark = pytest.mark.gpu

SHAPES = [(16, 32), (32, 64)]                                                    # (M, dim): rows of 8 and 16 bytes
# every size of the float-ADC matrix, each also odd and even (the half 16-byte word behind an odd number of 8-byte rows), and a
# partition no pattern touches, so that the index never runs empty
SIZES = [0, 1, 2, T - 1, T, T + 1, T + 2, 2 * T + 3, 2 * T + 4]
ANCHOR = 301
KEEP = 0.5


def shape_id(s):
    return "%dx4" % s[0]


_cases = {}


def case(shape):
    """(quantizers with one coarse centroid per partition, [(codes, labels)]): random code bytes, distinct labels in no order"""
    if shape not in _cases:
        M, dim = shape
        sizes = SIZES + [ANCHOR]
        q = Quantizers4(M, dim, K=len(sizes), n=64, seed=21)
        rng = np.random.default_rng(300 + M)
        total = sum(sizes)
        labels = rng.permutation(4 * total)[:total].astype(np.uint32)
        parts, at = [], 0
        for n in sizes:
            parts.append((rand_codes(rng, n, M), labels[at:at + n].copy()))
            at += n
        _cases[shape] = (q, parts)
    return _cases[shape]


def build(q, parts, mode="own"):
    """mode "own": the partitions as add_partitions left them, each an allocation of its own; "arena": moved into the arena by a reserve"""
    idx = q.index()
    idx.add_partitions([c for c, _ in parts], [l for _, l in parts])
    if mode == "arena":
        idx.reserve([len(c) for c, _ in parts])
    return idx


def pattern_list(parts, pattern):
    """the labels of the rows the pattern takes from every partition but the anchor, and one label the index does not hold"""
    absent = np.uint32(max(int(l.max()) for _, l in parts if len(l)) + 5)
    return np.concatenate([l[pattern(len(l))] for _, l in parts[:-1]] + [np.array([absent], np.uint32)])


# ---- 1. partition sizes x removal patterns, read back ----------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("mode", ["own", "arena"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_pattern_on_every_partition_size(shape, mode):
    q, parts = case(shape)
    for name, pattern in PATTERNS.items():
        removed = pattern_list(parts, pattern)
        want, gone = model_remove(parts, removed)
        assert gone == len(removed) - 1
        idx = build(q, parts, mode)
        try:
            moved = idx.relocations()
            assert idx.remove_labels(np.random.default_rng(2).permutation(removed)) == gone, name
            check(idx, want, name)
            for p in range(len(want)):
                if len(want[p][0]):
                    assert np.array_equal(idx.read_codes(p, 0, len(want[p][0])), want[p][0]), name
            assert idx.relocations() == moved, name
        finally:
            idx.close()


# ---- 2. queries after finalize: every scan path ----------------------------------------------------------------------------------

def same_queries(got, ref, q, K, what):
    """query_scan, search and scan_i8 of both indexes, bit for bit; the anchor partition is every query's first probe"""
    M = q.nsq
    rng = np.random.default_rng(77)
    nq, ma, R = K - 1, 3, 100
    assign = np.array([[K - 1, i, (i + 4) % (K - 1)] for i in range(nq)], np.int32)
    tables = float_tables(rng, nq, ma, M)
    a, b = got.query_scan(assign, tables.copy(), R), ref.query_scan(assign, tables.copy(), R)
    for name in ("keys", "values", "sizes", "status", "qmin", "qmax"):
        assert np.array_equal(a[name], b[name]), "%s: query_scan %s" % (what, name)
    queries = (q.coarse[K - 1] + 0.1 * rng.normal(size=(8, q.dim))).astype(np.float32)
    a, b = got.search(queries, ma, R), ref.search(queries, ma, R)
    for name in ("keys", "values", "sizes", "assign", "status"):
        assert np.array_equal(a[name], b[name]), "%s: search %s" % (what, name)
    qt = rand_qtables(rng, (nq, ma), M, 7)
    for x, y in zip(got.scan_i8(assign, qt, R), ref.scan_i8(assign, qt, R)):
        assert heaps_equal(x, y), "%s: scan_i8" % what


@pytest.mark.parametrize("mode", ["own", "arena"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_queries_after_a_removal_equal_a_fresh_index(shape, mode):
    q, parts = case(shape)
    for name, pattern in PATTERNS.items():
        removed = pattern_list(parts, pattern)
        want, gone = model_remove(parts, removed)
        got, ref = build(q, parts, mode), build(q, want)
        try:
            assert got.remove_labels(removed) == gone
            got.finalize(KEEP)
            ref.finalize(KEEP)
            assert [got.start_size(p) for p in range(len(want))] == [ref.start_size(p) for p in range(len(want))], name
            same_queries(got, ref, q, len(parts), "%s, %s" % (name, mode))
        finally:
            got.close()
            ref.close()


# ---- 3. finalized or not -----------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("mode", ["own", "arena"])
def test_a_no_hit_call_keeps_the_index_finalized_and_a_hit_does_not(mode):
    shape = SHAPES[0]
    q, parts = case(shape)
    K = len(parts)
    rng = np.random.default_rng(5)
    assign = np.array([[K - 1, 3]], np.int32)
    tables = float_tables(rng, 1, 2, shape[0])
    absent = np.uint32(max(int(l.max()) for _, l in parts if len(l)) + 5)
    idx = build(q, parts, mode)
    try:
        idx.finalize(KEEP)
        before = idx.query_scan(assign, tables.copy(), 50)
        assert idx.remove_labels([absent, absent + 1]) == 0                      # no hit
        assert idx.remove_labels([]) == 0                                        # nothing to look for
        after = idx.query_scan(assign, tables.copy(), 50)                        # no second finalize
        assert np.array_equal(before["keys"], after["keys"]) and np.array_equal(before["values"], after["values"])
        check(idx, parts)
        assert idx.remove_labels([parts[3][1][0], absent]) == 1                  # a hit
        with pytest.raises(pyqadc.QadcError, match="finalize") as e:
            idx.query_scan(assign, tables.copy(), 50)
        assert "qadc error %d:" % pyqadc.QADC_E_STATE in str(e.value)            # as after add_vectors
        idx.finalize(KEEP)
        idx.query_scan(assign, tables.copy(), 50)
        check(idx, model_remove(parts, [parts[3][1][0]])[0])
    finally:
        idx.close()


# ---- 4. the byte-plane form --------------------------------------------------------------------------------------------------------

def test_split_scan_after_remove(po):
    """a partition one code past a byte-plane tile once 100 of its rows are gone: finalize builds the copy from the compacted rows,
    and the split scan reads it"""
    extra, R, keep = 100, 100, 0.01
    n = SPLIT_TILE + 1 + extra
    rng = np.random.default_rng(8)
    codes = rand_codes(rng, n, 16)
    labels = rng.permutation(3 * n)[:n].astype(np.uint32)
    removed = labels[rng.permutation(n)[:extra]]
    idx = pyqadc.Index(16)
    try:
        for k, v in dict(share_variant=0, mq=0, front_run_max=0, wgq=0).items():   # one query per pass: the launches that read the copy
            idx.set_option(k, v)
        idx.set_split(1, 1)
        idx.add_partitions([codes], [labels])
        idx.finalize(keep)                                                       # a copy of the old rows exists
        assert idx.remove_labels(removed) == extra
        idx.finalize(keep)
        assert idx.profile()["split_copy_bytes"] == 2 * 7 * SPLIT_TILE
        (want_codes, want_labels), = model_remove([(codes, labels)], removed)[0]
        got_codes, got_labels = idx.read_partition(0)
        assert len(got_codes) == SPLIT_TILE + 1 and np.array_equal(got_codes, want_codes) and np.array_equal(got_labels, want_labels)
        tables = float_tables(np.random.default_rng(5), 3, 1, 16)
        res = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
        for i in range(3):
            want = po.query_scan(16, [want_codes], [want_labels], keep, [0], tables[i].copy(), R)
            assert want["rc"] == res["status"][i] == 0
            assert heaps_equal((res["keys"][i, :res["sizes"][i]], res["values"][i, :res["sizes"][i]]), (want["keys"], want["values"])), i
    finally:
        idx.close()


# ---- 5. a view sees the survivors --------------------------------------------------------------------------------------------------

@path_independent
def test_a_view_created_after_a_removal_sees_the_survivors():
    shape = SHAPES[0]
    q, parts = case(shape)
    removed = pattern_list(parts, PATTERNS["every-other-row"])
    want, gone = model_remove(parts, removed)
    got, ref = build(q, parts), build(q, want)
    views = []
    try:
        assert got.remove_labels(removed) == gone
        for idx in (got, ref):
            idx.finalize(KEEP)
            views.append(pyqadc.AdcIndex.view_of(idx))
        assert [views[0].partition_size(p) for p in range(len(want))] == [len(c) for c, _ in want]
        queries = np.random.default_rng(3).normal(size=(6, q.dim)).astype(np.float32) * 2
        for x, y in zip(views[0].search(queries, 3, 100), views[1].search(queries, 3, 100)):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    finally:
        for v in views:
            v.close()
        got.close()
        ref.close()


# ---- 6. the list in device memory --------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_remove_labels_device_equals_remove_labels(shape):
    import torch
    q, parts = case(shape)
    removed = pattern_list(parts, PATTERNS["run-across-a-tile-edge"])
    want, gone = model_remove(parts, removed)
    idx = build(q, parts, "arena")
    try:
        t = torch.from_numpy(removed.view(np.int32).copy()).to("cuda:0")
        assert idx.remove_labels_device(t) == gone > 0
        check(idx, want)
        assert idx.remove_labels_device(t) == 0
        with pytest.raises(TypeError):
            idx.remove_labels_device(removed)
        with pytest.raises(TypeError):
            idx.remove_labels_device(t.to(torch.int64))
        with pytest.raises(pyqadc.QadcError, match="device"):
            idx.remove_labels_device(t.cpu())
        check(idx, want)
    finally:
        idx.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def refused(idx, code, match, f, *args):
    before = read_all(idx)
    with pytest.raises(pyqadc.QadcError, match=match) as e:
        f(*args)
    assert "qadc error %d:" % code in str(e.value)
    assert_partitions(read_all(idx), before, "after the refused call")


@path_independent
def test_refusals_leave_the_index_as_it_was():
    import torch
    shape = SHAPES[0]
    q, parts = case(shape)
    some = parts[3][1][:5].copy()
    codes = parts[-1][0]
    ARG, STATE = pyqadc.QADC_E_ARG, pyqadc.QADC_E_STATE

    idx = build(q, parts)
    try:
        refused(idx, ARG, "labels is null", idx.remove_labels_raw, None, 3)
        idx.finalize(KEEP)
        view = pyqadc.AdcIndex.view_of(idx)                                      # a live view keeps the partitions' rows
        try:
            refused(idx, ARG, "view", idx.remove_labels, some)
        finally:
            view.close()
        tables = float_tables(np.random.default_rng(1), 1, 1, 16)               # a busy slot
        idx.submit(0, np.full((1, 1), len(parts) - 1, np.int32), tables, 10)
        refused(idx, STATE, "not been collected", idx.remove_labels, some)
        refused(idx, STATE, "not been collected", idx.remove_labels_device, torch.from_numpy(some.view(np.int32).copy()).to("cuda:0"))
        idx.collect(0)
        idx.dist_init_loopback(0, 1)                                             # under the multi-GPU merge
        refused(idx, ARG, "multi-GPU", idx.remove_labels, some)
        idx.dist_shutdown()
        assert idx.remove_labels(some) == 5                                      # the good call: the index is usable
        check(idx, model_remove(parts, some)[0])
    finally:
        idx.close()

    unl = q.index()                                                              # unlabelled add_partitions
    try:
        unl.add_partitions([codes[k:k + 3] for k in range(4)])
        refused(unl, ARG, "by position", unl.remove_labels, some)
    finally:
        unl.close()

    flat = q.index(coarse=False)                                                 # a flat index
    try:
        flat.add_vectors(q.vectors[:20])
        refused(flat, ARG, "by position", flat.remove_labels, some)
    finally:
        flat.close()

    shard = q.index(coarse=False)                                                # a shard with a starts replica
    try:
        shard.add_partition_shard(codes[16:48], 16, 64, labels=np.arange(32, dtype=np.uint32), starts=codes[:8])
        with pytest.raises(pyqadc.QadcError, match="shard") as e:
            shard.remove_labels(some)
        assert "qadc error %d:" % ARG in str(e.value)
        assert shard.partition_size(0) == 32 and np.array_equal(shard.read_codes(0, 0, 32), codes[16:48])
    finally:
        shard.close()

    lent = q.index(coarse=False)                                                 # a borrowed partition
    try:
        tc = torch.from_numpy(codes[:64].copy()).to("cuda:0")
        tl = torch.arange(64, dtype=torch.int32, device="cuda:0")
        lent.add_partition_device(tc.data_ptr(), 64, tl.data_ptr(), keepalive=(tc, tl))
        refused(lent, ARG, "borrowed", lent.remove_labels, np.arange(5, dtype=np.uint32))
        assert np.array_equal(lent.read_partition(0)[1], np.arange(64, dtype=np.uint32))
    finally:
        lent.close()
