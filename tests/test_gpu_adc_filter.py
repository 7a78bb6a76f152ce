"""Filtered float-ADC search (pyqadc.AdcFilter, AdcIndex.set_filter; qadc_adc_filter_*, qadc_adc_index_set_filter in include/qadc.h;
DESIGN.md section 11.10): with a key set S and a mode set on an index, every scanning call returns the heap arrays — keys, values
bit for bit, sizes — of the reference's scanner_simple::query_scan over the partitions from which the dropped rows have been
deleted, the surviving rows' keys given as labels.

Expected arrays come from tests/adc_filter_compose.py, which only deletes the rows and calls the helpers the unfiltered tests use
(test_gpu_adc.expected, adc4_compose.expected, adc16_compose.heap).  Sizes: kLevel0 = 512 and kLevelGrowth = 16 (host/adc_plan.hpp),
so the 12 000 codes of a query are three levels for R <= 512 (512 + 8192 + the rest); one loop iteration of the scan kernel is
256 x 4 = 1024 codes."""
import numpy as np
import pytest

import adc4_compose as a4
import adc_filter_compose as fc
import pyqadc
from helpers import path_independent
from test_gpu_adc_add import Quantizers, append, group
from test_gpu_adc_remove import model_remove, same_bits
from test_gpu_adc_rerun import descending, descending_table

pytestmark = pytest.mark.gpu

N = 12000
TOP = 2 ** 32 - 1
ZERO = np.zeros((1, 1), np.int32)


class Source:
    """An index of the shape over the given partitions: an owned AdcIndex (8 and 16 bits), or a view of a 4-bit Index"""

    def __init__(self, shape, parts, labels=None, key_bases=None):
        nsq, bits = shape
        self.src = None
        if bits == 4:
            self.src = pyqadc.Index(nsq)
            self.src.add_partitions(parts, labels)
            for p, base in enumerate(key_bases or []):
                self.src.set_key_base(p, int(base))
            self.src.finalize(0.01)
            self.idx = pyqadc.AdcIndex.view_of(self.src)
        else:
            assert key_bases is None
            self.idx = pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)
            self.idx.add_partitions(parts, labels)

    def close(self):
        self.idx.close()
        if self.src is not None:
            self.src.close()


def filtered(idx, S, mode, call):
    """call(idx) under the filter (S, mode); the filter is cleared and closed afterwards"""
    f = pyqadc.AdcFilter(S, mode)
    try:
        idx.set_filter(f)
        return call(idx)
    finally:
        idx.set_filter(None)
        f.close()


def heaps_equal(a, b):
    return len(a[0]) == len(b[0]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- 1. drop patterns x all eight shapes ---------------------------------------------------------------------------------------

def patterns(po, shape, codes, labels, tables, R, rng):
    """name -> bool [N]: the rows the case drops"""
    n = len(codes)
    rows = np.arange(n)

    def all_but(k):
        m = np.ones(n, bool)
        m[rng.permutation(n)[:k]] = False
        return m

    def best(k):                                                                 # the k rows of the unfiltered heap of capacity k
        return np.isin(labels, fc.unfiltered(po, shape, [codes], [labels], tables, k)[0])

    return {
        "nothing": np.zeros(n, bool),
        "everything": np.ones(n, bool),
        "the-first-512-rows": rows < 512,                                        # all of level 0: no dropped row may reach the select
        "the-first-8704-rows": rows < 8704,                                      # levels 0 and 1: the bound is still FLT_MAX entering level 2
        "every-other-row": rows % 2 == 0,
        "rows-1023-1024-1025-and-the-last": np.isin(rows, [1023, 1024, 1025, n - 1]),
        "all-but-R-1-rows": all_but(R - 1),                                      # the heap is not full
        "all-but-exactly-R-rows": all_but(R),
        "the-R-best-rows": best(R),                                              # a filter behind the bounds loses the rows that should win
        "the-4R-best-rows": best(4 * R),
    }


@path_independent
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.shape_id)
def test_every_drop_pattern_in_both_modes(po, shape):
    rng = np.random.default_rng(31 * shape[0] + shape[1])
    codes = fc.rand_codes(rng, shape, N)
    labels = rng.permutation(4 * N)[:N].astype(np.uint32) + np.uint32(77)
    tables = fc.rand_tables(rng, shape, 1, 1)
    db = Source(shape, [codes], [labels])
    try:
        for R in (1, 100):
            plain = fc.unfiltered(po, shape, [codes], [labels], tables[0], R)
            fc.assert_heap(db.idx.query_scan(ZERO, tables, R), plain, 0, "no filter R=%d" % R)
            for name, drop in patterns(po, shape, codes, labels, tables[0], R, rng).items():
                want = fc.unfiltered(po, shape, [codes[~drop]], [labels[~drop]], tables[0], R)
                if name.endswith("best-rows"):                                   # else the case would pass with the filter ignored
                    assert drop.sum() == (R if name.startswith("the-R-") else 4 * R) and not heaps_equal(want, plain), name
                for mode, S in (("exclude", labels[drop]), ("allow", labels[~drop])):
                    assert heaps_equal(want, fc.expected(po, shape, [codes], [labels], tables[0], R, S, mode))
                    got = filtered(db.idx, rng.permutation(S), mode, lambda idx: idx.query_scan(ZERO, tables, R))
                    fc.assert_heap(got, want, 0, "%s %s R=%d" % (mode, name, R))
    finally:
        db.close()


# ---- 2. IVF: every entry point, both finishes ----------------------------------------------------------------------------------

def replayed(po, keys, vals, offsets, nq, R):
    """the heaps a candidate stream replays to, in the layout of query_scan's result"""
    ok, ov, osz = np.zeros((nq, R), np.uint32), np.zeros((nq, R), np.float32), np.zeros(nq, np.int32)
    for q in range(nq):
        a, b = int(offsets[q]), int(offsets[q + 1])
        k, v = a4.replay(po, keys[a:b], vals[a:b], R)
        ok[q, :len(k)], ov[q, :len(k)], osz[q] = k, v, len(k)
    return ok, ov, osz


@path_independent
@pytest.mark.parametrize("shape", [(8, 8), (16, 4), (4, 16)], ids=fc.shape_id)
def test_ivf_through_every_entry_point_and_both_finishes(po, shape):
    import torch
    rng = np.random.default_rng(900 + shape[0])
    sizes = [0, 1, 511, 512, 513, 1025, 3000, 7000]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    perm = rng.permutation(4 * sum(sizes))[:sum(sizes)].astype(np.uint32)
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])].copy() for i in range(len(sizes))]
    labels[6][5] = labels[7][6000]                                               # one label held by two rows in two partitions
    nq, ma = 5, 4
    assign = np.stack([rng.permutation(np.arange(1, 8))[:ma] for _ in range(nq)]).astype(np.int32)
    assign[0] = [7, 6, 7, 0]                                                     # a duplicate probe and the empty partition
    assign[1] = [0, 6, 7, 5]                                                     # the empty partition first; both holders of the double label
    tables = fc.rand_tables(rng, shape, nq, ma)
    held = np.concatenate(labels)
    S = np.concatenate([rng.permutation(held)[:len(held) * 3 // 10], labels[6][5:6]])
    db = Source(shape, parts, labels)
    try:
        for mode in ("exclude", "allow"):
            f = pyqadc.AdcFilter(S, mode)
            db.idx.set_filter(f)
            for R in (1, 100):
                want = [fc.expected(po, shape, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R, S, mode)
                        for q in range(nq)]
                for finish in (0, 1):
                    db.idx.set_finish(finish)
                    got = db.idx.query_scan(assign, tables, R)
                    for q in range(nq):
                        fc.assert_heap(got, want[q], q, "query_scan %s R=%d finish %d" % (mode, R, finish))
                db.idx.set_finish(0)
                dk, dv, ds = db.idx.query_scan_device(assign, torch.from_numpy(tables).to("cuda:0"), R)
                got = (dk.cpu().numpy().view(np.uint32), dv.cpu().numpy(), ds.cpu().numpy())
                keys, vals, offsets = db.idx.query_scan_candidates(assign, tables, R)
                stream = replayed(po, keys, vals, offsets, nq, R)
                for q in range(nq):
                    fc.assert_heap(got, want[q], q, "query_scan_device %s R=%d" % (mode, R))
                    fc.assert_heap(stream, want[q], q, "the replayed stream %s R=%d" % (mode, R))
                    a, b = int(offsets[q]), int(offsets[q + 1])
                    assert not fc.dropped(keys[a:b], S, mode).any(), "a dropped row is in the stream"
            db.idx.set_filter(None)
            f.close()
    finally:
        db.close()


@path_independent
def test_search_equals_query_scan_on_its_tables_under_the_same_filter(po):
    import torch
    q = Quantizers(8, 8, 32, K=8, n=6000, seed=21)
    a, codes = q.encoded()
    full = group(a, codes, q.K)
    rng = np.random.default_rng(5)
    nq, ma, R = 5, 3, 100
    queries = (q.coarse[rng.integers(0, q.K, nq)] + rng.normal(size=(nq, 32))).astype(np.float32)
    S = rng.permutation(6000)[:1800].astype(np.uint32)
    idx = q.index()
    try:
        idx.add_partitions([c for c, _ in full], [l for _, l in full])
        assign, tables = idx.search_tables(queries, ma)
        for mode in ("exclude", "allow"):
            f = pyqadc.AdcFilter(S, mode)
            idx.set_filter(f)
            assign2, tables2 = idx.search_tables(queries, ma)                    # the feeders do not scan: unaffected
            assert np.array_equal(assign, assign2) and same_bits(tables, tables2)
            want = [fc.expected(po, (8, 8), [full[k][0] for k in assign[i]], [full[k][1] for k in assign[i]], tables[i], R, S, mode)
                    for i in range(nq)]
            for finish in (0, 1):
                idx.set_finish(finish)
                scan = idx.query_scan(assign, tables, R)
                got = idx.search(queries, ma, R)
                assert np.array_equal(got[3], assign)
                for i in range(nq):
                    fc.assert_heap(scan, want[i], i, "query_scan %s finish %d" % (mode, finish))
                    fc.assert_heap(got[:3], want[i], i, "search %s finish %d" % (mode, finish))
            dk, dv, ds = idx.search_device(torch.from_numpy(queries).to("cuda:0"), ma, R)
            got = (dk.cpu().numpy().view(np.uint32), dv.cpu().numpy(), ds.cpu().numpy())
            ck, cv, off, _ = idx.search_candidates(queries, ma, R)
            stream = replayed(po, ck, cv, off, nq, R)
            for i in range(nq):
                fc.assert_heap(got, want[i], i, "search_device %s" % mode)
                fc.assert_heap(stream, want[i], i, "search_candidates %s" % mode)
            idx.set_filter(None)
            f.close()
    finally:
        idx.close()


# ---- 3. unlabelled sources: keys are positions ---------------------------------------------------------------------------------

@path_independent
def test_an_owned_flat_index_is_filtered_by_position(po):
    shape = (8, 8)
    rng = np.random.default_rng(3)
    codes = fc.rand_codes(rng, shape, N)
    tables = fc.rand_tables(rng, shape, 1, 1)
    db = Source(shape, [codes])
    try:
        for S in ([0, N - 1, N, N + 5], np.arange(0, N, 3), np.arange(512), fc.unfiltered(po, shape, [codes], None, tables[0], 100)[0]):
            for mode in ("exclude", "allow"):
                for R in (1, 100):
                    want = fc.expected(po, shape, [codes], None, tables[0], R, S, mode)
                    got = filtered(db.idx, S, mode, lambda idx: idx.query_scan(ZERO, tables, R))
                    fc.assert_heap(got, want, 0, "positions %s R=%d" % (mode, R))
    finally:
        db.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
def test_a_view_with_a_key_base_is_filtered_by_base_plus_position(po, M):
    shape = (M, 4)
    rng = np.random.default_rng(40 + M)
    n2 = 700
    parts = [fc.rand_codes(rng, shape, N), fc.rand_codes(rng, shape, n2)]
    bases = [123456, TOP - n2 + 1]                                               # the second partition's last key is 2^32 - 1
    assign = np.array([[1, 0]], np.int32)
    tables = fc.rand_tables(rng, shape, 1, 2)
    db = Source(shape, parts, None, bases)
    try:
        b = bases[0]
        edges = [b - 1, b, b + 1, b + N - 1, b + N, TOP, TOP - n2 + 1, TOP - n2, 0]   # just below and above the base, first and last position
        best = fc.unfiltered(po, shape, parts[::-1], fc.keys_of(parts, None, bases)[::-1], tables[0], 100)[0]
        for S in (edges, best, b + np.arange(0, N, 2)):
            for mode in ("exclude", "allow"):
                for R in (1, 100):
                    want = fc.expected(po, shape, parts[::-1], None, tables[0], R, S, mode, key_bases=bases[::-1])
                    got = filtered(db.idx, S, mode, lambda idx: idx.query_scan(assign, tables, R))
                    fc.assert_heap(got, want, 0, "key base %s R=%d" % (mode, R))
    finally:
        db.close()


# ---- 4. key edges (after test_gpu_adc_remove.test_label_edges) -----------------------------------------------------------------

@path_independent
def test_key_edges_in_both_modes(po):
    shape = (8, 8)
    rng = np.random.default_rng(7)
    sizes = [40, 1500, 0, 17]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    perm = rng.permutation(20000)[:sum(sizes)].astype(np.uint32) + np.uint32(10000)   # labels from 10000, then the hand-made ones
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])].copy() for i in range(len(sizes))]
    labels[0][:6] = [0, TOP, 999, 1000, 1036, 1037]
    labels[1][[0, 1024, 1499]] = [1010, 1001, TOP - 1]
    labels[3][:3] = [1010, 1, 998]                                               # 1010: two rows in two partitions
    # tables that make the hand-made rows the best of their query, so that dropping them shows in every heap
    tables = fc.rand_tables(rng, shape, 1, 4) + np.float32(1.0)
    for p, rows in ((0, range(6)), (1, (0, 1024, 1499)), (3, range(3))):
        for r in rows:
            tables[0, p].reshape(8, 256)[np.arange(8), parts[p][r]] = np.float32(0.001) * rng.random(8, dtype=np.float32)
    assign = np.array([[0, 1, 2, 3]], np.int32)
    db = Source(shape, parts, labels)
    cases = [
        ([2000, 2001, 5000], "a set that holds no key of the database", (2000, 5000)),
        ([], "an empty set", (TOP, 0)),
        # lo = 1000 and hi = 1036 are held; 999 = lo - 1 and 1037 = hi + 1 are held too; the span, 37 bits, is no multiple of 32
        ([1036, 1000, 1036, 1000, 1000], "lo and hi, duplicates", (1000, 1036)),
        ([1010, 1010], "a key held by two rows in two partitions", (1010, 1010)),
        ([TOP, 0], "keys 0 and 2^32 - 1: the full-span bitmap", (0, TOP)),
        (np.array([TOP - 1, 1], np.uint32), "a span that ends one below the top", (1, TOP - 1)),
    ]
    try:
        for R in (1, 12):
            plain = fc.unfiltered(po, shape, parts, labels, tables[0], R)
            for S, what, (lo, hi) in cases:
                for mode in ("exclude", "allow"):
                    f = pyqadc.AdcFilter(S, mode)
                    nbytes = 4 if lo > hi else ((hi - lo + 1 + 31) // 32) * 4
                    assert f.info() == dict(mode=mode, lo=lo, hi=hi, bitmap_bytes=nbytes), what
                    db.idx.set_filter(f)
                    want = fc.expected(po, shape, parts, labels, tables[0], R, S, mode)
                    fc.assert_heap(db.idx.query_scan(assign, tables, R), want, 0, "%s, %s, R=%d" % (what, mode, R))
                    db.idx.set_filter(None)
                    f.close()
                    if R == 12 and what.startswith(("lo and hi", "a key held", "keys 0", "a span")):   # (R = 1: one winner, which few sets hold)
                        assert not heaps_equal(want, plain), what                # the case is not vacuous
                    if R == 12 and mode == "exclude" and what.startswith("lo and hi"):
                        assert {999, 1037} <= set(want[0].tolist()) and not {1000, 1036} & set(want[0].tolist())
        assert pyqadc.AdcFilter([TOP, 0]).info()["bitmap_bytes"] == 512 << 20
    finally:
        db.close()


# ---- 5. the re-run path --------------------------------------------------------------------------------------------------------

@path_independent
def test_a_filtered_descending_scan_order_reruns_and_stays_exact(po):
    """test_gpu_adc_rerun's descending scan order, n = 20 000, every other row excluded: the 10 000 survivors are all pushes of the
    reference.  At R = 1 the region holds 512 + 32 + 32 + 4096 = 4672 entries (host/adc_plan.hpp: three levels), so the batch must
    re-run; at R = 100 it holds 11 008 and takes the survivors without one, so the re-run count is asserted to grow at R = 1 only."""
    n = 20000
    rng = np.random.default_rng(n)
    codes = descending(n, rng)
    tdesc = descending_table().reshape(1, 1, -1)
    keep = np.arange(n) % 2 == 1
    S = np.flatnonzero(~keep).astype(np.uint32)
    idx = pyqadc.AdcIndex(4, 8)
    idx.add_partitions([codes])
    f = pyqadc.AdcFilter(S, "exclude")
    idx.set_filter(f)
    try:
        survivors = np.arange(n, 0, -1).astype(np.float32)[keep]
        for finish in (0, 1):
            idx.set_finish(finish)
            for R in (1, 100):
                runs = idx.reruns()
                got = idx.query_scan(ZERO, tdesc, R)
                fc.assert_heap(got, fc.expected(po, (4, 8), [codes], None, tdesc[0], R, S, "exclude"), 0, "descending R=%d finish %d" % (R, finish))
                if R == 1:
                    assert idx.reruns() > runs, "the candidate region did not overflow: the re-run path was not taken"
                if finish == 0:
                    keys, vals, offsets = idx.query_scan_candidates(ZERO, tdesc, R)
                    assert int(offsets[1]) == n // 2 and np.array_equal(vals, survivors)
                    assert np.array_equal(keys, np.flatnonzero(keep).astype(np.uint32))
    finally:
        idx.close()
        f.close()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------

@path_independent
def test_setting_clearing_replacing_and_sharing_a_filter(po):
    rng = np.random.default_rng(60)
    shape = (8, 8)
    codes = fc.rand_codes(rng, shape, N)
    labels = rng.permutation(N).astype(np.uint32)
    tables = fc.rand_tables(rng, shape, 1, 1)
    codes4 = fc.rand_codes(rng, (16, 4), N)
    tables4 = fc.rand_tables(rng, (16, 4), 1, 1)
    R = 100
    own, view = Source(shape, [codes], [labels]), Source((16, 4), [codes4], [labels])
    S1, S2 = labels[::2].copy(), fc.unfiltered(po, shape, [codes], [labels], tables[0], R)[0]
    f1, f2 = pyqadc.AdcFilter(S1, "exclude"), pyqadc.AdcFilter(S2, "exclude")
    try:
        before = own.idx.query_scan(ZERO, tables, R)
        own.idx.set_filter(f1)
        fc.assert_heap(own.idx.query_scan(ZERO, tables, R), fc.expected(po, shape, [codes], [labels], tables[0], R, S1, "exclude"), 0, "f1")
        own.idx.set_filter(f2)                                                   # replacing one filter by another releases the first
        fc.assert_heap(own.idx.query_scan(ZERO, tables, R), fc.expected(po, shape, [codes], [labels], tables[0], R, S2, "exclude"), 0, "f2")
        f1.close()
        f1 = pyqadc.AdcFilter(S1, "exclude")
        view.idx.set_filter(f2)                                                  # one filter on two indexes, an owned one and a view
        fc.assert_heap(view.idx.query_scan(ZERO, tables4, R), fc.expected(po, (16, 4), [codes4], [labels], tables4[0], R, S2, "exclude"), 0, "view")
        with pytest.raises(pyqadc.QadcError, match="qadc error %d:" % pyqadc.QADC_E_STATE):
            f2.close()                                                           # set on two indexes
        own.idx.set_filter(None)
        with pytest.raises(pyqadc.QadcError, match="qadc error %d:" % pyqadc.QADC_E_STATE):
            f2.close()                                                           # ... on one
        fc.assert_heap(view.idx.query_scan(ZERO, tables4, R), fc.expected(po, (16, 4), [codes4], [labels], tables4[0], R, S2, "exclude"), 0,
                       "the view after the refused destroy")
        after = own.idx.query_scan(ZERO, tables, R)
        assert all(same_bits(x, y) for x, y in zip(before, after)), "set_filter(None) did not restore the unfiltered arrays"
        own.idx.set_filter(f2)
        own.idx.set_filter(f2)                                                   # the filter that is set already: one use, not two
        own.idx.set_filter(None)
        view.idx.set_filter(None)
        f2.close()                                                               # succeeds after clearing
        f2 = None
        own.idx.set_filter(f1)                                                   # destroying the index releases its use
    finally:
        own.close()
        view.close()
    f1.close()
    assert f2 is None


@path_independent
def test_add_vectors_and_remove_labels_with_a_filter_set(po):
    q = Quantizers(8, 8, 64, n=4000, seed=33)
    a, codes = q.encoded()
    rng = np.random.default_rng(34)
    nq, ma, R = 4, 3, 50
    queries = (q.coarse[rng.integers(0, q.K, nq)] + rng.normal(size=(nq, 64))).astype(np.float32)
    S = np.concatenate([np.arange(0, 3000, 3), 100000 + np.arange(0, 1000, 2)]).astype(np.uint32)   # keys of rows that come later too
    idx = q.index()
    f = pyqadc.AdcFilter(S, "exclude")
    try:
        idx.set_filter(f)

        def check(model, what):
            assign, tables = idx.search_tables(queries, ma)
            got = idx.search(queries, ma, R)
            for i in range(nq):
                want = fc.expected(po, (8, 8), [model[k][0] for k in assign[i]], [model[k][1] for k in assign[i]], tables[i], R, S, "exclude")
                fc.assert_heap(got[:3], want, i, what)

        idx.add_vectors(q.vectors[:3000])
        model = group(a[:3000], codes[:3000], q.K)
        check(model, "after add_vectors")
        idx.add_vectors(q.vectors[3000:], labels_offset=100000)
        model = append(model, group(a[3000:], codes[3000:], q.K, 100000))
        check(model, "after a second add_vectors")
        removed = np.concatenate([np.arange(1, 3000, 3), 100000 + np.arange(1, 1000, 4)]).astype(np.uint32)
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == len(removed)
        check(model, "after remove_labels")
        assert f.info()["lo"] == 0 and f.info()["hi"] == 100998                  # the filter stays as it is
    finally:
        idx.close()
        f.close()


@path_independent
def test_sub_batches_and_batches_equal_their_single_queries(po):
    rng = np.random.default_rng(64)
    shape = (8, 8)
    sizes = [3000, 0, 5000, 4000]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    perm = rng.permutation(sum(sizes)).astype(np.uint32)
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))]
    nq, ma, R = 64, 3, 100
    assign = rng.integers(0, 4, (nq, ma)).astype(np.int32)
    tables = fc.rand_tables(rng, shape, nq, ma)
    S = rng.permutation(sum(sizes))[:sum(sizes) * 3 // 10].astype(np.uint32)
    db = Source(shape, parts, labels)
    f = pyqadc.AdcFilter(S, "allow")
    try:
        db.idx.set_filter(f)
        batch = db.idx.query_scan(assign, tables, R)
        for q in (0, 17, 63):                                                    # the oracle on three of them; the others against the single calls
            want = fc.expected(po, shape, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R, S, "allow")
            fc.assert_heap(batch, want, q, "batch of 64")
        for q in range(nq):
            one = db.idx.query_scan(assign[q:q + 1], tables[q:q + 1], R)
            assert all(same_bits(x[0], y[q]) for x, y in zip(one, batch)), "query %d alone differs from the batch" % q
        db.idx.set_table_budget(ma * 8 * 256 * 4)                                # one query per pass
        for finish in (0, 1):
            db.idx.set_finish(finish)
            passes = db.idx.query_scan(assign, tables, R)
            assert all(same_bits(x, y) for x, y in zip(passes, batch)), "one query per pass, finish %d" % finish
    finally:
        db.close()
        f.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

@path_independent
def test_refusals():
    import ctypes as C
    import torch
    L = pyqadc.lib()
    some = np.arange(5, dtype=np.uint32)
    h = C.c_void_p()

    def refused(rc, match):
        assert rc == pyqadc.QADC_E_ARG and match in L.qadc_last_error().decode(), (rc, L.qadc_last_error())

    refused(L.qadc_adc_filter_create(None, 0, pyqadc._p(some, pyqadc.u32p), 5, 0), "out is null")
    refused(L.qadc_adc_filter_create_device(None, 0, None, 0, 0), "out is null")
    for mode in (2, -1):
        refused(L.qadc_adc_filter_create(C.byref(h), mode, pyqadc._p(some, pyqadc.u32p), 5, 0), "mode")
        assert not h.value
    refused(L.qadc_adc_filter_create(C.byref(h), 1, None, 3, 0), "keys is null")
    refused(L.qadc_adc_filter_create_device(C.byref(h), 1, None, 3, 0), "keys is null")
    assert not h.value
    with pytest.raises(ValueError):
        pyqadc.AdcFilter(some, "only")
    with pytest.raises(pyqadc.QadcError, match="keys is null"):
        pyqadc.AdcFilter.create_raw(0, None, 2)
    for bad, exc in ((torch.arange(5, dtype=torch.int64, device="cuda:0"), TypeError), (some, TypeError),
                     (torch.arange(5, dtype=torch.int32), pyqadc.QadcError),
                     (torch.zeros((5, 2), dtype=torch.int32, device="cuda:0"), pyqadc.QadcError)):
        with pytest.raises(exc):
            pyqadc.AdcFilter.from_device(bad)
    idx = pyqadc.AdcIndex(8, 8)
    f = pyqadc.AdcFilter.create_raw(0, None, 0)                                  # count 0 looks at no list
    try:
        with pytest.raises(TypeError):
            idx.set_filter(some)
        refused(L.qadc_adc_index_set_filter(None, f._h), "index is null")
        assert L.qadc_adc_filter_destroy(None) == 0
        if torch.cuda.device_count() > 1:                                        # a filter of another device
            other = pyqadc.AdcFilter(some, device=1)
            with pytest.raises(pyqadc.QadcError, match="device"):
                idx.set_filter(other)
            other.close()
    finally:
        idx.close()
        f.close()


@path_independent
def test_a_filter_from_the_keys_a_device_search_returned(po):
    import torch
    q = Quantizers(8, 8, 32, K=8, n=5000, seed=71)
    a, codes = q.encoded()
    full = group(a, codes, q.K)
    idx = q.index()
    try:
        idx.add_partitions([c for c, _ in full], [l for _, l in full])
        dq = torch.from_numpy(q.vectors[:6]).to("cuda:0")
        keys, _, sizes = idx.search_device(dq, 2, 50)                            # "not the rows this search returned"
        assert int(sizes.min().item()) == 50
        S = keys.reshape(-1).cpu().numpy().view(np.uint32)
        assign, tables = idx.search_tables(q.vectors[:6], 2)
        for mode in ("exclude", "allow"):
            f = pyqadc.AdcFilter.from_device(keys.reshape(-1), mode)
            host = pyqadc.AdcFilter(S, mode)
            assert f.info() == host.info() == dict(mode=mode, lo=int(S.min()), hi=int(S.max()), bitmap_bytes=((int(S.max()) - int(S.min())) // 32 + 1) * 4)
            host.close()
            idx.set_filter(f)
            got = idx.search(q.vectors[:6], 2, 50)
            for i in range(6):
                want = fc.expected(po, (8, 8), [full[k][0] for k in assign[i]], [full[k][1] for k in assign[i]], tables[i], 50, S, mode)
                fc.assert_heap(got[:3], want, i, "from_device %s" % mode)
                if mode == "exclude":
                    assert not np.isin(got[0][i, :got[2][i]], S).any()
            idx.set_filter(None)
            f.close()
    finally:
        idx.close()
