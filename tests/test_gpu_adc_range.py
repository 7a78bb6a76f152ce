"""Float-ADC range search on the GPU (pyqadc.AdcIndex.range_scan / range_search and their _device forms; qadc_adc_range_* in
include/qadc.h): for every query, every row of its probed partitions whose candidate is < radius and whose
key passes the filters, ascending by (candidate, key).

Expected results are the numpy restatement of tests/adc_range_cases.py, to which tests/test_adc_range_host.py holds the host twin
scanner_simple::range_scan.  Every comparison is exact: lims, keys and the value bit patterns."""
import numpy as np
import pytest

import adc_filter_compose as fc
import adc_range_cases as rc
import pyqadc
from helpers import path_independent
from test_gpu_adc_add import Quantizers
from test_gpu_adc_filter import Source

pytestmark = pytest.mark.gpu

T = pyqadc.ADC_RANGE_SORT_LDS
INF = np.float32(np.inf)
SHAPES = [(8, 8), (16, 4), (4, 16)]


def run_case(shape, case, what):
    db = Source(shape, case["parts"], case["labels"])
    try:
        got = db.idx.range_scan(case["assign"], case["tables"], case["radius"])
        want = rc.expected_batch(shape, case["parts"], case["labels"], case["assign"], case["tables"], case["radius"])
        rc.assert_same(got, want, what)
        return got
    finally:
        db.close()


# ---- 1. kernel edges: partition sizes around one loop iteration (1024 rows) and one run (2048), a probed empty partition ----------

@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_partition_sizes_at_the_scan_kernels_edges(shape):
    case = rc.kernel_edges(shape)
    lims, _, _ = run_case(shape, case, "kernel edges")
    assert (np.diff(lims) > 100).all(), "every query keeps rows"


# ---- 2. ties and the strict compare ------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_tied_rows_all_come_out_and_the_radius_itself_does_not(shape):
    case = rc.ties(shape)
    lims, keys, vals = run_case(shape, case, "ties")
    at, below = [], []
    for q in range(2):
        k, v = keys[lims[q]:lims[q + 1]], vals[lims[q]:lims[q + 1]]
        at.append(int((v == case["present"]).sum()))
        below.append(int((v < case["present"]).sum()))
        w = rc.words(k, v)
        assert (w[1:] == w[:-1]).any(), "no two rows share key and candidate: the case is vacuous"
    assert at[0] == 0 and at[1] >= 2 and below[0] == below[1] > 0, "the radius' own value is kept only under its nextafter"
    twins = (keys[lims[1]:] == 7) & (vals[lims[1]:] == case["present"])
    assert twins.sum() >= 2, "both one-row partitions with the same label and code come out"


# ---- 3. a region overflows: exactly one re-run ---------------------------------------------------------------------------------------

@path_independent
def test_an_overflowing_query_re_runs_the_batch_once():
    shape, n = (8, 8), 20000
    rng = np.random.default_rng(3)
    codes = fc.rand_codes(rng, shape, n)
    tables = fc.rand_tables(rng, shape, 3, 1)
    handful = rc.radius_for(rc.candidates(shape, codes, tables[2, 0]), 7)
    radius = np.array([INF, -INF, handful], np.float32)
    assign = np.zeros((3, 1), np.int32)
    idx = pyqadc.AdcIndex(8, 8)
    idx.add_partitions([codes])
    try:
        before = idx.reruns()
        got = idx.range_scan(assign, tables, radius)
        assert idx.reruns() == before + 1
        rc.assert_same(got, rc.expected_batch(shape, [codes], None, assign, tables, radius), "re-run")
        assert list(np.diff(got[0])) == [n, 0, 7]
        got = idx.range_scan(assign[1:], tables[1:], radius[1:])              # nothing overflows: no re-run
        assert idx.reruns() == before + 1 and list(np.diff(got[0])) == [0, 7]
    finally:
        idx.close()


# ---- 4. the sort: lengths around the LDS threshold, radix passes skipped and not ---------------------------------------------------

@path_independent
def test_result_lengths_around_the_lds_threshold():
    shape, n = (8, 8), T + 2000
    rng = np.random.default_rng(4)
    codes = fc.rand_codes(rng, shape, n)
    labels = rng.permutation(5 * n)[:n].astype(np.uint32)
    lengths = [0, 1, T - 1, T, T + 1]
    tables = fc.rand_tables(rng, shape, len(lengths), 1)
    radius = np.array([-INF if rows == 0 else rc.radius_for(rc.candidates(shape, codes, tables[q, 0]), rows)
                       for q, rows in enumerate(lengths)], np.float32)
    case = dict(parts=[codes], labels=[labels], assign=np.zeros((len(lengths), 1), np.int32), tables=tables, radius=radius)
    lims, _, _ = run_case(shape, case, "lengths 0, 1, T - 1, T, T + 1")
    assert list(np.diff(lims)) == lengths


@path_independent
def test_long_segments_ordered_by_key_bits_alone_and_by_value_bits_alone():
    shape, n = (8, 8), 20000
    rng = np.random.default_rng(5)
    parts = [fc.rand_codes(rng, shape, n), fc.rand_codes(rng, shape, n)]
    labels = [rng.permutation(1 << 24)[:n].astype(np.uint32), np.full(n, 5, np.uint32)]
    tables = fc.rand_tables(rng, shape, 2, 1)
    tables[0] = np.float32(0.5)                                               # every candidate of query 0 is 4.0: only the key orders it
    case = dict(parts=parts, labels=labels, assign=np.array([[0], [1]], np.int32), tables=tables, radius=np.array([INF, INF], np.float32))
    lims, keys, vals = run_case(shape, case, "long segments")
    assert list(np.diff(lims)) == [n, n]
    assert (vals[:n] == np.float32(4.0)).all() and (np.diff(keys[:n].astype(np.int64)) > 0).all()
    assert (keys[n:] == 5).all() and len(np.unique(vals[n:])) > n // 2


# ---- 5. filters: the index's EXCLUDE under per-query ALLOWs, None entries and an empty set ---------------------------------------------

@path_independent
def test_an_index_exclude_composes_with_per_query_allows():
    shape = (8, 8)
    rng = np.random.default_rng(6)
    sizes = [3000, 2500, 1500]
    parts = [fc.rand_codes(rng, shape, s) for s in sizes]
    perm = rng.permutation(4 * sum(sizes))[:sum(sizes)].astype(np.uint32)
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(3)]
    nq = 5
    assign = np.array([[0, 1], [2, 0], [1, 2], [0, 2], [1, 0]], np.int32)
    tables = fc.rand_tables(rng, shape, nq, 2)
    radius = np.full(nq, 30.0, np.float32)
    radius[3] = INF
    tomb = rng.permutation(perm)[:len(perm) // 4]
    specs = [(rng.permutation(perm)[:len(perm) // 2], "allow"), None, ([], "allow"), (rng.permutation(perm)[:len(perm) // 3], "allow"), None]
    filters = [None if s is None else pyqadc.AdcFilter(np.asarray(s[0], np.uint32), s[1]) for s in specs]
    index_filter = pyqadc.AdcFilter(tomb, "exclude")
    idx = pyqadc.AdcIndex(8, 8)
    idx.add_partitions(parts, labels)
    try:
        plain = idx.range_scan(assign, tables, radius)
        rc.assert_same(plain, rc.expected_batch(shape, parts, labels, assign, tables, radius), "no filter")
        idx.set_filter(index_filter)
        both = idx.range_scan(assign, tables, radius, filters=filters)
        want = rc.expected_batch(shape, parts, labels, assign, tables, radius, specs, (tomb, "exclude"))
        rc.assert_same(both, want, "EXCLUDE on the index, ALLOW per query")
        rows, base = np.diff(both[0]), np.diff(plain[0])
        assert rows[2] == 0 and (0 < rows[[0, 1, 3, 4]]).all() and (rows < base).all(), "every filter drops rows and none drops all: %s of %s" % (rows, base)
        assert not np.isin(both[1], tomb).any()
        only = idx.range_scan(assign, tables, radius, filters=[None] * nq)
        rc.assert_same(only, rc.expected_batch(shape, parts, labels, assign, tables, radius, None, (tomb, "exclude")), "the index's filter alone")
    finally:
        idx.close()
        index_filter.close()
        for f in filters:
            if f is not None:
                f.close()


# ---- 6. passes of the table budget, device forms, the held result: one index with quantizers ------------------------------------------

class Ivf:
    """an 8x8 IVF index filled by add_vectors, and its partitions read back as the model"""

    def __init__(self, seed=0, n=6000):
        self.q = Quantizers(8, 8, 32, K=8, n=n, seed=seed)
        self.shape = (8, 8)
        self.idx = self.q.index()
        self.idx.add_vectors(self.q.vectors)
        self.read()
        rng = np.random.default_rng(70 + seed)
        self.queries = (self.q.vectors[rng.integers(0, n, 5)] + rng.normal(size=(5, 32)) * 0.3).astype(np.float32)
        self.rng = rng

    def read(self):
        rows = [self.idx.read_partition(p) for p in range(self.idx.partition_count())]
        self.parts, self.labels = [r[0] for r in rows], [r[1] for r in rows]

    def want(self, queries, ma, radius, specs=None, index_spec=None):
        assign, tables = self.idx.search_tables(queries, ma)
        return assign, tables, rc.expected_batch(self.shape, self.parts, self.labels, assign, tables, radius, specs, index_spec)

    def radii(self, queries, ma, rows):
        """per query, a radius that keeps about rows[q] rows"""
        assign, tables = self.idx.search_tables(queries, ma)
        out = []
        for q in range(len(queries)):
            v = np.sort(np.concatenate([rc.candidates(self.shape, self.parts[p], tables[q, a]) for a, p in enumerate(assign[q])]))
            out.append(v[min(rows[q], len(v) - 1)])
        return np.array(out, np.float32)


@pytest.fixture(scope="module")
def ivf():
    db = Ivf()
    yield db
    db.idx.close()


@path_independent
def test_passes_of_the_table_budget_append_behind_each_other(ivf):
    ma, nq = 3, 5
    radius = ivf.radii(ivf.queries, ma, [50, 0, 900, 5, 300])
    held = np.concatenate(ivf.labels)
    specs = [(ivf.rng.permutation(held)[:len(held) // 2], "allow"), (ivf.rng.permutation(held)[:len(held) // 5], "exclude"), None,
             ([], "exclude"), (ivf.rng.permutation(held)[:len(held) // 3], "allow")]
    filters = [None if s is None else pyqadc.AdcFilter(np.asarray(s[0], np.uint32), s[1]) for s in specs]
    try:
        assign, tables, want = ivf.want(ivf.queries, ma, radius, specs)
        assert len(set(np.diff(want[0]))) == nq, "five queries, five different row counts: %s" % np.diff(want[0])
        one_pass_scan = ivf.idx.range_scan(assign, tables, radius, filters=filters)
        one_pass_search = ivf.idx.range_search(ivf.queries, ma, radius, filters=filters)
        ivf.idx.set_table_budget(2 * ma * 8 * 256 * 4)                       # the tables of two queries: passes of 2, 2 and 1
        rc.assert_same(ivf.idx.range_scan(assign, tables, radius, filters=filters), want, "range_scan in passes of two")
        rc.assert_same(ivf.idx.range_search(ivf.queries, ma, radius, filters=filters), want, "range_search in passes of two")
        rc.assert_same(one_pass_scan, want, "range_scan in one pass")
        rc.assert_same(one_pass_search, want, "range_search in one pass")
    finally:
        ivf.idx.set_table_budget(0)
        for f in filters:
            if f is not None:
                f.close()


@path_independent
def test_the_device_forms_equal_the_host_forms(ivf):
    import torch
    ma = 2
    radius = ivf.radii(ivf.queries, ma, [40, 700, 1, 0, T + 50])
    assign, tables, want = ivf.want(ivf.queries, ma, radius)
    dev = torch.device("cuda", 0)
    lims, keys, vals = ivf.idx.range_search_device(torch.from_numpy(ivf.queries).to(dev), ma, radius)
    assert isinstance(lims, np.ndarray) and keys.is_cuda and vals.is_cuda and keys.dtype == torch.int32 and vals.dtype == torch.float32
    rc.assert_same((lims, keys.cpu().numpy(), vals.cpu().numpy()), want, "range_search_device")
    lims, keys, vals = ivf.idx.range_scan_device(assign, torch.from_numpy(tables).to(dev), radius)
    rc.assert_same((lims, keys.cpu().numpy(), vals.cpu().numpy()), want, "range_scan_device")
    rc.assert_same(ivf.idx.range_search(ivf.queries, ma, radius), want, "range_search")
    rc.assert_same(ivf.idx.range_scan(assign, tables, float(radius[0])), ivf.want(ivf.queries, ma, radius[0])[2], "a scalar radius")


@path_independent
def test_the_result_is_held_until_the_next_range_call(ivf):
    ma = 3
    radius = ivf.radii(ivf.queries, ma, [60, 500, 3, 0, T + 10])
    _, _, want = ivf.want(ivf.queries, ma, radius)
    fresh = ivf.q.index()
    try:
        rc_, _, _ = fresh.range_collect_raw(10)
        assert rc_ == pyqadc.QADC_E_STATE, "nothing to collect on an index that never ranged"
    finally:
        fresh.close()
    lims, keys, vals = ivf.idx.range_search(ivf.queries, ma, radius)
    rc.assert_same((lims, keys, vals), want, "range_search")
    for finish in (0, 1):                                                    # top-R calls in between, both finishes
        ivf.idx.set_finish(finish)
        ivf.idx.search(ivf.queries, ma, 100)
    ivf.idx.set_finish(0)
    n = int(lims[-1])
    short, _, _ = ivf.idx.range_collect_raw(n - 1)
    assert short == pyqadc.QADC_E_CAPACITY
    k, v = ivf.idx.range_collect(lims)
    rc.assert_same((lims, k, v), want, "collect after two searches and a short collect")
    k, v = ivf.idx.range_collect()
    rc.assert_same((lims, k, v), want, "a second collect")


@path_independent
def test_after_add_and_remove_the_range_is_the_twins_on_the_new_database():
    db = Ivf(seed=1, n=4000)
    try:
        ma = 4
        more = (db.q.vectors[:1500] + np.float32(0.05)).astype(np.float32)
        db.idx.add_vectors(more, labels_offset=100000)
        gone = np.concatenate([np.arange(0, 4000, 3), np.arange(100000, 100400)]).astype(np.uint32)
        assert db.idx.remove_labels(gone) == len(gone)
        db.read()
        assert sum(len(p) for p in db.parts) == 5500 - len(gone)
        radius = db.radii(db.queries, ma, [100, 1000, 10, 2000, 1])
        _, _, want = db.want(db.queries, ma, radius)
        got = db.idx.range_search(db.queries, ma, radius)
        rc.assert_same(got, want, "after add_vectors and remove_labels")
        assert not np.isin(got[1], gone).any() and (got[1] >= 100400).any()
    finally:
        db.idx.close()
