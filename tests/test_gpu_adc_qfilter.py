"""One key filter per query of a float-ADC batch (filters= of pyqadc.AdcIndex's scanning calls; qadc_adc_*_filtered in
include/qadc.h): a row is emitted for query q iff it passes the index's filter, if one is set, and
filters[q], if that is not None — so every query's heap arrays are the reference's scanner_simple::query_scan over the partitions
from which the rows dropped for THAT query have been deleted, the surviving keys given as labels.

Expected arrays come from tests/adc_filter_compose.py, once per query with that query's (S, mode); under an index filter the
database is reduced by the index's set first and by the query's then.  Sizes as in tests/test_gpu_adc_filter.py: kLevel0 = 512 and
kLevelGrowth = 16 (host/adc_plan.hpp), so at most 12 000 codes per query are three levels for R <= 512, and one loop iteration of
the scan kernel is 256 x 4 = 1024 codes."""
import numpy as np
import pytest

import adc_filter_compose as fc
import pyqadc
from helpers import path_independent
from test_gpu_adc_add import Quantizers, append, group
from test_gpu_adc_filter import Source, heaps_equal, replayed
from test_gpu_adc_remove import model_remove, same_bits
from test_gpu_adc_rerun import descending, descending_table

pytestmark = pytest.mark.gpu

N = 12000


def want_heap(po, shape, parts, labels, tables, R, spec, key_bases=None, index_spec=None):
    """heap arrays of one query: spec = its own (S, mode) or None; index_spec = the (S, mode) of the filter set on the index"""
    keys = fc.keys_of(parts, labels, key_bases)
    if index_spec is not None:
        parts, keys = fc.reduce(parts, keys, *index_spec)
    if spec is None:
        return fc.unfiltered(po, shape, parts, keys, tables, R)
    return fc.expected(po, shape, parts, keys, tables, R, *spec)


def make(specs):
    """[(S, mode) | None | an int: the filter object made for that earlier position] -> the AdcFilter | None list"""
    out = []
    for s in specs:
        out.append(None if s is None else out[s] if isinstance(s, int) else pyqadc.AdcFilter(np.asarray(s[0], np.uint32), s[1]))
    return out


def spec_of(specs, q):
    return specs[specs[q]] if isinstance(specs[q], int) else specs[q]


def close_all(filters):
    for f in {id(f): f for f in filters if f is not None}.values():
        f.close()


def host(dev):
    k, v, s = dev
    return k.cpu().numpy().view(np.uint32), v.cpu().numpy(), s.cpu().numpy()


# ---- 1. a mixed batch on one partition, all eight shapes ---------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.shape_id)
def test_a_mixed_batch_gives_every_query_its_own_heap(po, shape):
    rng = np.random.default_rng(57 * shape[0] + shape[1])
    codes = fc.rand_codes(rng, shape, N)
    labels = rng.permutation(4 * N)[:N].astype(np.uint32) + np.uint32(77)
    nq = 6
    tables = fc.rand_tables(rng, shape, nq, 1)
    A = np.concatenate([rng.permutation(labels)[:N * 3 // 10], [5, 4 * N + 1000]]).astype(np.uint32)  # with keys no row holds
    B = rng.permutation(labels)[:N * 4 // 10].astype(np.uint32)
    specs = [None, (A, "exclude"), (B, "allow"), 1, ([], "allow"), ([], "exclude")]                 # position 3: the same object as 1
    filters = make(specs)
    assert filters[3] is filters[1]
    assign = np.zeros((nq, 1), np.int32)
    db = Source(shape, [codes], [labels])
    try:
        for R in (1, 100):
            got = db.idx.query_scan(assign, tables, R, filters=filters)
            for q in range(nq):
                want = want_heap(po, shape, [codes], [labels], tables[q], R, spec_of(specs, q))
                plain = fc.unfiltered(po, shape, [codes], [labels], tables[q], R)
                if q in (0, 5):
                    assert heaps_equal(want, plain)
                elif q == 4:
                    assert np.array_equal(want[0], np.zeros(R, np.uint32)) and (want[1] >= np.float32(3e38)).all()
                elif R == 100:
                    assert not heaps_equal(want, plain), "query %d's filter leaves its heap as it was: the case is vacuous" % q
                fc.assert_heap(got, want, q, "mixed batch R=%d" % R)
    finally:
        db.close()
        close_all(filters)


# ---- 2. filters can be neither swapped nor broadcast --------------------------------------------------------------------------------

@path_independent
def test_every_query_loses_its_own_best_rows_and_no_other(po):
    shape, nq, R = (8, 8), 5, 50
    rng = np.random.default_rng(202)
    codes = fc.rand_codes(rng, shape, N)
    labels = rng.permutation(N).astype(np.uint32)
    tables = fc.rand_tables(rng, shape, nq, 1)
    plain = [fc.unfiltered(po, shape, [codes], [labels], tables[q], R) for q in range(nq)]
    specs = [(plain[q][0], "exclude") for q in range(nq)]                         # query q's filter: its own R winners
    want = [want_heap(po, shape, [codes], [labels], tables[q], R, specs[q]) for q in range(nq)]
    for q in range(nq):
        assert not heaps_equal(want[q], plain[q]), "query %d: the heap without its winners is the unfiltered heap" % q
        for other in ((q + 1) % nq, (q - 1) % nq, 0):
            if other != q:                                                       # a neighbour's filter, or the first one for everyone
                wrong = want_heap(po, shape, [codes], [labels], tables[q], R, specs[other])
                assert not heaps_equal(want[q], wrong), "query %d under query %d's filter has the same heap" % (q, other)
    filters = make(specs)
    db = Source(shape, [codes], [labels])
    try:
        for finish in (0, 1):
            db.idx.set_finish(finish)
            got = db.idx.query_scan(np.zeros((nq, 1), np.int32), tables, R, filters=filters)
            for q in range(nq):
                fc.assert_heap(got, want[q], q, "own winners excluded, finish %d" % finish)
    finally:
        db.close()
        close_all(filters)


# ---- 3. every entry point, both finishes --------------------------------------------------------------------------------------------

def nine_specs(rng, held):
    def some(share):
        return rng.permutation(held)[:len(held) * share // 10].astype(np.uint32)
    return [None, (some(3), "exclude"), (some(4), "allow"), (some(5), "exclude"), (some(2), "allow"), None, ([], "exclude"), 2,
            (some(7), "exclude")]


@path_independent
@pytest.mark.parametrize("shape", [(8, 8), (16, 4), (4, 16)], ids=fc.shape_id)
def test_ivf_through_every_entry_point_and_both_finishes(po, shape):
    import torch
    nsq, bits = shape
    rng = np.random.default_rng(1900 + nsq)
    sizes = [0, 1, 511, 512, 513, 1025, 3000, 7000]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    if bits == 4:                                                                # a view: unlabelled partitions with key bases
        labels, bases = None, [1000000 * p + 17 for p in range(len(sizes))]
    else:
        perm = rng.permutation(4 * sum(sizes))[:sum(sizes)].astype(np.uint32)
        labels, bases = [perm[sum(sizes[:i]):sum(sizes[:i + 1])].copy() for i in range(len(sizes))], None
    held = np.concatenate(fc.keys_of(parts, labels, bases))
    nq, ma = 9, 3
    specs = nine_specs(rng, held)
    filters = make(specs)
    assign = np.stack([rng.permutation(np.arange(1, 8))[:ma] for _ in range(nq)]).astype(np.int32)
    assign[0] = [7, 0, 7]                                                        # a duplicate probe and the empty partition
    assign[1] = [0, 6, 7]
    tables = fc.rand_tables(rng, shape, nq, ma)
    dim = 2 * nsq
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    db = Source(shape, parts, labels, bases)
    quant = db.src if bits == 4 else db.idx
    quant.set_pq(rng.normal(size=(nsq, 1 << bits, 2)).astype(np.float32))
    quant.set_coarse((rng.normal(size=(len(sizes), dim)) * 2).astype(np.float32))

    def wants(assign_, tables_, R):
        return [want_heap(po, shape, [parts[k] for k in assign_[q]], None if labels is None else [labels[k] for k in assign_[q]], tables_[q], R,
                          spec_of(specs, q), None if bases is None else [bases[k] for k in assign_[q]]) for q in range(nq)]

    def check_stream(keys, vals, offsets, want, R, what):
        stream = replayed(po, keys, vals, offsets, nq, R)
        for q in range(nq):
            fc.assert_heap(stream, want[q], q, what)
            if spec_of(specs, q) is not None:
                a, b = int(offsets[q]), int(offsets[q + 1])
                assert not fc.dropped(keys[a:b], *spec_of(specs, q)).any(), "%s: a row dropped for query %d is in its stream" % (what, q)

    try:
        s_assign, s_tables = db.idx.search_tables(queries, ma)
        d_tables, d_queries = torch.from_numpy(tables).to("cuda:0"), torch.from_numpy(queries).to("cuda:0")
        for R in (1, 100):
            want_scan, want_search = wants(assign, tables, R), wants(s_assign, s_tables, R)
            for finish in (0, 1):
                db.idx.set_finish(finish)
                tag = "R=%d finish %d" % (R, finish)
                got = {
                    "query_scan": (db.idx.query_scan(assign, tables, R, filters=filters), want_scan),
                    "query_scan_device": (host(db.idx.query_scan_device(assign, d_tables, R, filters=filters)), want_scan),
                    "search": (db.idx.search(queries, ma, R, filters=filters)[:3], want_search),
                    "search_device": (host(db.idx.search_device(d_queries, ma, R, filters=filters)), want_search),
                }
                for name, (arrays, want) in got.items():
                    for q in range(nq):
                        fc.assert_heap(arrays, want[q], q, "%s %s" % (name, tag))
                check_stream(*db.idx.query_scan_candidates(assign, tables, R, filters=filters), want_scan, R, "query_scan_candidates " + tag)
                ck, cv, off, a = db.idx.search_candidates(queries, ma, R, filters=filters)
                assert np.array_equal(a, s_assign)
                check_stream(ck, cv, off, want_search, R, "search_candidates " + tag)
    finally:
        db.close()
        close_all(filters)


# ---- 4. sub-batches of the table budget ---------------------------------------------------------------------------------------------

@path_independent
def test_sub_batches_see_the_filters_of_their_own_queries(po):
    """a budget of two queries' tables cuts nq = 5 into passes of 2, 2 and 1 queries, each numbered from 0: five different filters,
    so a table indexed by the pass's query number hands queries 2, 3 and 4 the filters of 0, 1 and 0"""
    shape, nq, ma = (8, 8), 5, 2
    rng = np.random.default_rng(404)
    sizes = [5000, 3000, 4000]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    perm = rng.permutation(sum(sizes)).astype(np.uint32)
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))]
    assign = np.array([[0, 1], [2, 0], [1, 2], [0, 2], [2, 1]], np.int32)
    tables = fc.rand_tables(rng, shape, nq, ma)
    specs = [(rng.permutation(perm)[:len(perm) * (2 + q) // 10], "exclude" if q % 2 == 0 else "allow") for q in range(nq)]
    filters = make(specs)
    queries = rng.normal(size=(nq, 16)).astype(np.float32)
    db = Source(shape, parts, labels)
    db.idx.set_pq(rng.normal(size=(8, 256, 2)).astype(np.float32))
    db.idx.set_coarse((rng.normal(size=(3, 16)) * 2).astype(np.float32))
    try:
        for R in (1, 100):
            want = [want_heap(po, shape, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R, specs[q]) for q in range(nq)]
            want_plain = [want_heap(po, shape, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R, None) for q in range(nq)]
            for q in range(2, nq):
                wrong = want_heap(po, shape, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R, specs[q % 2])
                assert R == 1 or not heaps_equal(want[q], wrong), "query %d under the filter of query %d has the same heap" % (q, q % 2)
            for finish in (0, 1):
                db.idx.set_finish(finish)
                db.idx.set_table_budget(0)
                whole = db.idx.query_scan(assign, tables, R, filters=filters)
                whole_search = db.idx.search(queries, ma, R, filters=filters)
                whole_stream = db.idx.query_scan_candidates(assign, tables, R, filters=filters)
                db.idx.set_table_budget(2 * ma * 8 * 256 * 4)                    # the tables of two queries
                passes = db.idx.query_scan(assign, tables, R, filters=filters)
                passes_search = db.idx.search(queries, ma, R, filters=filters)
                passes_stream = db.idx.query_scan_candidates(assign, tables, R, filters=filters)
                for q in range(nq):
                    fc.assert_heap(whole, want[q], q, "one pass R=%d finish %d" % (R, finish))
                    fc.assert_heap(passes, want[q], q, "passes of two queries R=%d finish %d" % (R, finish))
                assert all(same_bits(x, y) for x, y in zip(passes, whole))
                assert all(same_bits(x, y) for x, y in zip(passes_search, whole_search)), "search in passes of two queries differs"
                assert all(same_bits(x, y) for x, y in zip(passes_stream, whole_stream)), "the stream in passes of two queries differs"
                sparse = [filters[0], None, None, None, filters[4]]              # the middle pass has no filter at all: the plain kernels
                got = db.idx.query_scan(assign, tables, R, filters=sparse)
                for q in range(nq):
                    fc.assert_heap(got, want[q] if sparse[q] is not None else want_plain[q], q, "a pass without filters R=%d finish %d" % (R, finish))
    finally:
        db.close()
        close_all(filters)


# ---- 5. the re-run path -------------------------------------------------------------------------------------------------------------

@path_independent
def test_a_region_overflow_in_a_filtered_batch_reruns_under_the_same_filters(po):
    """test_gpu_adc_rerun's descending scan order for query 2 of four, n = 12 000, every fourth position excluded for it: its 9000
    survivors are all pushes of the reference, the region holds 512 + 32 * 2 + 4096 = 4672 entries at R = 1 (host/adc_plan.hpp:
    three levels), so the batch re-runs — and must scan under the same four filters again"""
    shape, n, nq = (4, 8), N, 4
    rng = np.random.default_rng(n + 1)
    codes = descending(n, rng)
    tables = fc.rand_tables(rng, shape, nq, 1)
    tables[2, 0] = descending_table()
    rows = np.arange(n, dtype=np.uint32)
    specs = [(rows[::3], "allow"), None, (rows[::4], "exclude"), (rng.permutation(rows)[:n // 2], "exclude")]
    filters = make(specs)
    assign = np.zeros((nq, 1), np.int32)
    idx = pyqadc.AdcIndex(4, 8)
    idx.add_partitions([codes])
    try:
        for finish in (0, 1):
            idx.set_finish(finish)
            for R in (1, 100):
                runs = idx.reruns()
                got = idx.query_scan(assign, tables, R, filters=filters)
                for q in range(nq):
                    fc.assert_heap(got, want_heap(po, shape, [codes], None, tables[q], R, specs[q]), q, "R=%d finish %d" % (R, finish))
                if R == 1:
                    assert idx.reruns() > runs, "the candidate region did not overflow: the re-run path was not taken"
        keys, vals, offsets = idx.query_scan_candidates(assign, tables, 1, filters=filters)
        a, b = int(offsets[2]), int(offsets[3])
        keep = rows % 4 != 0
        assert b - a == int(keep.sum()) and np.array_equal(keys[a:b], rows[keep])
        assert np.array_equal(vals[a:b], np.arange(n, 0, -1).astype(np.float32)[keep])
    finally:
        idx.close()
        close_all(filters)


# ---- 6. composition with the index's filter -----------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(8, 8), (32, 4), (2, 16)], ids=fc.shape_id)
def test_the_filter_of_the_index_and_the_filters_of_the_queries_compose(po, shape):
    rng = np.random.default_rng(606 + shape[0])
    sizes = [7000, 5000]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    perm = rng.permutation(3 * N)[:N].astype(np.uint32)
    labels = [perm[:7000], perm[7000:]]
    nq, ma, R = 5, 2, 100
    assign = np.array([[0, 1], [1, 0], [0, 0], [1, 1], [0, 1]], np.int32)
    tables = fc.rand_tables(rng, shape, nq, ma)
    tomb = rng.permutation(perm)[:N * 3 // 10]                                   # index-wide EXCLUDE: tombstones
    tenant = [np.concatenate([tomb[q::7], rng.permutation(perm)[:N // 3]]) for q in range(nq)]   # ALLOW sets that overlap the tombstones
    specs = [(tenant[0], "allow"), (tenant[1], "allow"), None, (tenant[3], "exclude"), (tenant[4], "allow")]
    filters = make(specs)
    f_tomb = pyqadc.AdcFilter(tomb, "exclude")
    db = Source(shape, parts, labels)

    def args(q):
        return [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R

    try:
        plain = db.idx.query_scan(assign, tables, R)
        for fl in (None, [None] * nq):                                           # no filter anywhere: the plain call, bit for bit
            for finish in (0, 1):
                db.idx.set_finish(finish)
                assert all(same_bits(x, y) for x, y in zip(db.idx.query_scan(assign, tables, R, filters=fl), plain))
        db.idx.set_finish(0)
        keys, vals, offsets = db.idx.query_scan_candidates(assign, tables, R)
        for x, y in zip(db.idx.query_scan_candidates(assign, tables, R, filters=[None] * nq), (keys, vals, offsets)):
            assert same_bits(x, y)
        db.idx.set_filter(f_tomb)
        alone = db.idx.query_scan(assign, tables, R)
        assert all(same_bits(x, y) for x, y in zip(db.idx.query_scan(assign, tables, R, filters=[None] * nq), alone))
        for finish in (0, 1):
            db.idx.set_finish(finish)
            got = db.idx.query_scan(assign, tables, R, filters=filters)
            for q in range(nq):
                want = want_heap(po, shape, *args(q), specs[q], index_spec=(tomb, "exclude"))
                fc.assert_heap(got, want, q, "composed, finish %d" % finish)
                if finish == 0:
                    fc.assert_heap(alone, want_heap(po, shape, *args(q), None, index_spec=(tomb, "exclude")), q, "the index's filter alone")
                    if specs[q] is not None:                                     # neither filter alone gives the composed heap
                        assert not heaps_equal(want, want_heap(po, shape, *args(q), specs[q]))
                        assert not heaps_equal(want, want_heap(po, shape, *args(q), None, index_spec=(tomb, "exclude")))
                    assert not np.isin(want[0][want[1] < np.float32(3e38)], tomb).any()
        db.idx.set_filter(None)
        db.idx.set_finish(0)
        assert all(same_bits(x, y) for x, y in zip(db.idx.query_scan(assign, tables, R), plain))
    finally:
        db.close()
        f_tomb.close()
        close_all(filters)


# ---- 7. across add_vectors and remove_labels ----------------------------------------------------------------------------------------

@path_independent
def test_the_same_filter_objects_before_and_after_add_vectors_and_remove_labels(po):
    q = Quantizers(8, 8, 64, n=4000, seed=35)
    a, codes = q.encoded()
    rng = np.random.default_rng(36)
    nq, ma, R = 4, 3, 50
    queries = (q.coarse[rng.integers(0, q.K, nq)] + rng.normal(size=(nq, 64))).astype(np.float32)
    later = 100000 + np.arange(1000)                                             # keys of rows that come with the second add
    specs = [(np.concatenate([np.arange(0, 3000, 3), later[::2]]), "exclude"), None,
             (np.concatenate([np.arange(0, 3000, 2), later[::3]]), "allow"), (np.arange(1500, 100500), "exclude")]
    filters = make(specs)
    idx = q.index()
    try:
        def check(model, what):
            assign, tables = idx.search_tables(queries, ma)
            got = idx.search(queries, ma, R, filters=filters)
            assert np.array_equal(got[3], assign)
            for i in range(nq):
                want = want_heap(po, (8, 8), [model[k][0] for k in assign[i]], [model[k][1] for k in assign[i]], tables[i], R, specs[i])
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
    finally:
        idx.close()
        close_all(filters)


# ---- 8. re-ranking ------------------------------------------------------------------------------------------------------------------

@path_independent
def test_search_refined_reranks_the_filtered_search(po):
    import torch
    q = Quantizers(8, 8, 32, n=6000, seed=81)
    rng = np.random.default_rng(82)
    nq, ma, R, r_in = 4, 3, 20, 100
    queries = (q.vectors[rng.integers(0, 6000, nq)] + 0.3 * rng.normal(size=(nq, 32))).astype(np.float32)
    idx = q.index()
    store = pyqadc.Refine(32, "f32")
    filters = []
    try:
        idx.add_vectors(q.vectors, labels_offset=0)
        store.add(q.vectors)
        open_keys, open_vals, _, _ = idx.search(queries, ma, r_in)
        specs = [(open_keys[0][open_vals[0] < np.float32(3e38)], "exclude"), (rng.permutation(6000)[:3000], "allow"), None,
                 (open_keys[3][open_vals[3] < np.float32(3e38)][::2], "exclude")]
        filters = make(specs)
        keys, vals, sizes, _ = idx.search(queries, ma, r_in, filters=filters)
        want = store.rerank(queries, keys, R, values=vals)
        got = idx.search_refined(queries, ma, R, r_in, store, filters=filters)
        dev = idx.search_refined_device(torch.from_numpy(queries).cuda(), ma, R, r_in, store, filters=filters)
        dev = host(dev[:3]) + (dev[3],)
        for x, y, z in zip(got[:3], want[:3], dev[:3]):
            assert same_bits(x, y) and same_bits(z, y)
        assert got[3] == want[3] == dev[3]
        unfiltered = idx.search_refined(queries, ma, R, r_in, store)
        for i in range(nq):
            n = int(got[2][i])
            assert n > 0
            if specs[i] is not None:
                assert not fc.dropped(got[0][i, :n], *specs[i]).any(), "query %d: a dropped key was refined" % i
                assert not np.array_equal(got[0][i, :n], unfiltered[0][i, :n]), "query %d: the filter changed nothing" % i
            else:
                assert np.array_equal(got[0][i, :n], unfiltered[0][i, :n])
    finally:
        idx.close()
        store.close()
        close_all(filters)


# ---- 9. front-end errors ------------------------------------------------------------------------------------------------------------

@path_independent
def test_a_wrong_length_and_a_closed_filter_raise_before_anything_runs():
    import torch
    rng = np.random.default_rng(9)
    q = Quantizers(8, 8, 16, K=2, n=300, seed=9)
    idx = q.index()
    idx.add_vectors(q.vectors)
    nq, ma, R = 3, 2, 10
    assign = np.zeros((nq, ma), np.int32)
    tables = fc.rand_tables(rng, (8, 8), nq, ma)
    queries = rng.normal(size=(nq, 16)).astype(np.float32)
    d_tables, d_queries = torch.from_numpy(tables).to("cuda:0"), torch.from_numpy(queries).to("cuda:0")
    store = pyqadc.Refine(16, "f32")
    store.add(q.vectors)
    live, closed = pyqadc.AdcFilter([1, 2, 3]), pyqadc.AdcFilter([4, 5])
    closed.close()
    calls = {
        "query_scan": lambda fl: idx.query_scan(assign, tables, R, filters=fl),
        "query_scan_device": lambda fl: idx.query_scan_device(assign, d_tables, R, filters=fl),
        "query_scan_candidates": lambda fl: idx.query_scan_candidates(assign, tables, R, filters=fl),
        "search": lambda fl: idx.search(queries, ma, R, filters=fl),
        "search_device": lambda fl: idx.search_device(d_queries, ma, R, filters=fl),
        "search_candidates": lambda fl: idx.search_candidates(queries, ma, R, filters=fl),
        "search_refined": lambda fl: idx.search_refined(queries, ma, 5, R, store, filters=fl),
        "search_refined_device": lambda fl: idx.search_refined_device(d_queries, ma, 5, R, store, filters=fl),
    }
    try:
        for name, call in calls.items():
            for bad in ([live] * (nq - 1), [live] * (nq + 1), []):
                with pytest.raises(ValueError, match="filters has %d entries for %d queries" % (len(bad), nq)):
                    call(bad)
            with pytest.raises(pyqadc.QadcError, match=r"filters\[1\] is closed"):
                call([live, closed, None])
            with pytest.raises(TypeError):
                call([live, [1, 2], None])
            call([live, None, live])                                             # and the call itself works
        if torch.cuda.device_count() > 1:                                        # a filter of another device: refused by the C call
            other = pyqadc.AdcFilter([1], device=1)
            with pytest.raises(pyqadc.QadcError, match=r"filters\[2\] is on device 1"):
                idx.query_scan(assign, tables, R, filters=[None, live, other])
            other.close()
    finally:
        idx.close()
        store.close()
        live.close()
