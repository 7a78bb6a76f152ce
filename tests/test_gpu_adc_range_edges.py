"""Float-ADC range search on the GPU where tests/test_gpu_adc_range.py does not reach: candidates of both
signs, signed zeros, subnormals, NaN, infinities and FLT_MAX under every kind of radius; every digit of adc_range_sort_kernel's radix
sort and every number of passes it can take; a re-run, a radix sort and a growing result buffer in a later pass of a call, behind
rows already held; unlabelled keys with a base in the top byte.

Expected results come from the numpy restatement tests/adc_range_cases.py alone (rc.expected_batch), to which
tests/test_adc_range_host.py holds the host twin on the same builders.  Every comparison is exact: lims, keys, value bit patterns."""
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


def device_tables(tables):
    import torch
    return torch.from_numpy(np.ascontiguousarray(tables, np.float32)).to(torch.device("cuda", 0))


def scan(idx, case, sum_mode=1, device=False):
    """range_scan, or range_scan_device with its tensors fetched"""
    if not device:
        return idx.range_scan(case["assign"], case["tables"], case["radius"], sum_mode=sum_mode)
    lims, keys, vals = idx.range_scan_device(case["assign"], device_tables(case["tables"]), case["radius"], sum_mode=sum_mode)
    return lims, keys.cpu().numpy(), vals.cpu().numpy()


@path_independent
def test_the_cases_are_built_for_this_lds_threshold():
    assert T == rc.RANGE_SORT_LDS


# ---- 1. the sort's digits: segments whose words differ in exactly the bytes a mask names ------------------------------------------------

DIGIT_RUNS = [((8, 8), m) for m in rc.DIGIT_MASKS] + [(s, m) for s in ((16, 4), (4, 16)) for m in (0xff, 0x80)]


@path_independent
@pytest.mark.parametrize("shape,mask", DIGIT_RUNS, ids=["%s-%#04x" % (fc.shape_id(s), m) for s, m in DIGIT_RUNS])
def test_segments_that_differ_in_chosen_digits_sort_in_the_radix_passes_and_in_lds(shape, mask):
    """6000 rows under radius +inf: the region overflows, the call re-runs once and the segment takes one radix pass per set bit of the
    mask (rc.digit_case asserts that the expected words differ in exactly those bytes); 3000 rows: no re-run, the bitonic sort"""
    for n, reruns in ((6000, 1), (3000, 0)):
        case = rc.digit_case(shape, mask, n)
        db = Source(shape, case["parts"], case["labels"])
        try:
            before = db.idx.reruns()
            got = scan(db.idx, case)
            assert db.idx.reruns() == before + reruns
            rc.assert_same(got, rc.expected_of(case), "mask %#04x, %d rows" % (mask, n))
        finally:
            db.close()


# ---- 2. sign, signed zeros, subnormals; NaN, infinities and FLT_MAX under every radius: all eight shapes, both groupings ----------------

@path_independent
@pytest.mark.parametrize("sum_mode", [1, 0], ids=["as_compiled", "source_order"])
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.shape_id)
def test_candidates_of_both_signs_with_signed_zeros_and_subnormals(shape, sum_mode):
    case = rc.signed_case(shape)
    want = rc.expected_of(case, sum_mode)
    db = Source(shape, case["parts"], case["labels"])
    try:
        for device in (False, True):
            before = db.idx.reruns()
            got = scan(db.idx, case, sum_mode, device)
            assert db.idx.reruns() == before + 1, "query 0 keeps more than the first region holds"
            rc.assert_same(got, want, "signed, device tables" if device else "signed")
    finally:
        db.close()


@path_independent
@pytest.mark.parametrize("sum_mode", [1, 0], ids=["as_compiled", "source_order"])
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.shape_id)
def test_nan_infinite_and_flt_max_candidates_under_every_radius(shape, sum_mode):
    """radii +inf, FLT_MAX, its predecessor, NaN, -inf, +0, -0 and 1e-45, four to a call"""
    case = rc.nonfinite_case(shape)
    db = Source(shape, case["parts"], case["labels"])
    try:
        for radii in (case["radii"][:4], case["radii"][4:]):
            batch = rc.nonfinite_batch(case, radii)
            want = rc.expected_of(batch, sum_mode)
            tables = device_tables(batch["tables"])
            rc.assert_same(scan(db.idx, batch, sum_mode), want, "radii %s" % radii)
            lims, keys, vals = db.idx.range_scan_device(batch["assign"], tables, batch["radius"], sum_mode=sum_mode)
            rc.assert_same((lims, keys.cpu().numpy(), vals.cpu().numpy()), want, "radii %s, device tables" % radii)
    finally:
        db.close()


@path_independent
@pytest.mark.parametrize("shape", [s for s in fc.SHAPES if s not in ((8, 8), (16, 4), (4, 16))], ids=fc.shape_id)
def test_partition_sizes_at_the_scan_kernels_edges_on_the_other_shapes(shape):
    case = dict(rc.kernel_edges(shape), shape=shape)
    db = Source(shape, case["parts"], case["labels"])
    try:
        got = scan(db.idx, case)
        rc.assert_same(got, rc.expected_of(case), "kernel edges")
        assert (np.diff(got[0]) > 100).all(), "every query keeps rows"
    finally:
        db.close()


# ---- 3. later passes of a call: a re-run, a radix sort and a growing result behind rows already held -----------------------------------

class World:
    """an IVF index of four partitions of about 3000 rows filled by add_vectors, its partitions read back as the model, six queries
    probing two partitions each and their tables, from the feeders"""
    MA = 2

    def __init__(self, nsq, bits):
        n = 12000
        self.shape = (nsq, bits)
        self.q = Quantizers(nsq, bits, 32, K=4, n=n)
        self.idx = self.q.index()
        self.idx.add_vectors(self.q.vectors)
        rows = [self.idx.read_partition(p) for p in range(self.idx.partition_count())]
        self.parts, self.labels = [r[0] for r in rows], [r[1] for r in rows]
        rng = np.random.default_rng(90 + nsq + bits)
        self.queries = (self.q.vectors[rng.integers(0, n, 6)] + rng.normal(size=(6, 32)) * 0.3).astype(np.float32)
        self.assign, self.tables = self.idx.search_tables(self.queries, self.MA)
        self.cands = [np.concatenate([rc.candidates(self.shape, self.parts[p], self.tables[q, a]) for a, p in enumerate(self.assign[q])])
                      for q in range(6)]
        self.budget = 2 * self.MA * (nsq << bits) * 4                        # the tables of two queries: passes of 2, 2 and 2

    def radii(self, rows):
        """per query a radius that keeps exactly rows[q] rows; a negative entry counts back from all the query probes"""
        out = []
        for q, r in enumerate(rows):
            r = r if r >= 0 else len(self.cands[q]) + r
            out.append(-INF if r == 0 else rc.radius_for(self.cands[q], r))
        return np.array(out, np.float32)


def later_passes(w):
    import torch
    assert min(len(c) for c in w.cands) > T + 1000, "every query probes well over T rows"
    dq = torch.from_numpy(w.queries).to(torch.device("cuda", 0))
    calls = [("short | above T and short | T and empty", [30, 700, -500, 12, T, 0]),
             ("a larger result, every pass overflows", [-900, 3, T + 400, T + 1, 0, -7]),
             ("a smaller one in the buffers held", [10, T + 1, 0, 50, 2000, 1])]
    w.idx.set_table_budget(w.budget)
    try:
        for what, rows in calls:
            radius = w.radii(rows)
            want = rc.expected_batch(w.shape, w.parts, w.labels, w.assign, w.tables, radius)
            kept = np.diff(want[0])
            assert list(kept) == [r if r >= 0 else len(w.cands[q]) + r for q, r in enumerate(rows)], "the radii do not cut where they are meant to"
            overflowing = sum(int(kept[p:p + 2].max() > T) for p in (0, 2, 4))   # (a region of exactly T rows does not overflow)
            forms = [("range_scan", overflowing, lambda: w.idx.range_scan(w.assign, w.tables, radius)),
                     ("range_search", overflowing, lambda: w.idx.range_search(w.queries, w.MA, radius)),
                     ("range_search_device", overflowing, lambda: w.idx.range_search_device(dq, w.MA, radius)),   # (table passes, as range_search)
                     ("range_scan_device", 1, lambda: w.idx.range_scan_device(w.assign, device_tables(w.tables), radius))]   # (one pass)
            for name, reruns, call in forms:
                before = w.idx.reruns()
                lims, keys, vals = call()
                assert w.idx.reruns() == before + reruns, "%s, %s: %d re-runs, expected %d" % (what, name, w.idx.reruns() - before, reruns)
                if not isinstance(keys, np.ndarray):
                    keys, vals = keys.cpu().numpy(), vals.cpu().numpy()
                rc.assert_same((lims, keys, vals), want, "%s, %s" % (what, name))
                k, v = w.idx.range_collect(lims)
                rc.assert_same((lims, k, v), want, "%s, range_collect after %s" % (what, name))
    finally:
        w.idx.set_table_budget(0)
        w.idx.close()


@path_independent
@pytest.mark.parametrize("shape", [(8, 8), (4, 16)], ids=fc.shape_id)
def test_a_re_run_and_a_radix_sort_behind_rows_held_by_earlier_passes(shape):
    """six queries in passes of two.  First call: pass 1 holds short segments, pass 2 one above T (a re-run and radix passes at
    held > 0 and a result buffer that grows with rows in it), pass 3 a segment of exactly T rows and an empty one.  Then a larger result
    in which every pass overflows, then a smaller one; each through all four forms, collected again after each."""
    later_passes(World(*shape))


# ---- 4. unlabelled keys: a view's key bases in the top byte, an owned index's positions ---------------------------------------------------

@path_independent
@pytest.mark.parametrize("sum_mode", [1, 0], ids=["as_compiled", "source_order"])
def test_a_views_key_bases_near_the_top_of_the_key_range(sum_mode):
    shape = (16, 4)
    rng = np.random.default_rng(14)
    parts = [fc.rand_codes(rng, shape, 5000), fc.rand_codes(rng, shape, 3000)]
    bases = [0xfefff000, 0xffffe000]                                         # partition 0 crosses 0xff000000 at row 4096
    assign = np.array([[0, 1], [1, 0]], np.int32)
    tables = fc.rand_tables(rng, shape, 2, 2)
    v1 = np.concatenate([rc.candidates(shape, parts[p], tables[1, a], sum_mode) for a, p in enumerate(assign[1])])
    radius = np.array([INF, rc.radius_for(v1, 2000)], np.float32)
    want = rc.expected_batch(shape, parts, None, assign, tables, radius, sum_mode=sum_mode, key_bases=bases)
    assert list(np.diff(want[0])) == [8000, 2000]
    assert rc.active_digits(rc.words(want[1][:8000], want[2][:8000])) & 0x0f == 0x0f, "the keys differ in all four bytes"
    assert int(want[1].max()) == 0xffffe000 + 2999
    db = Source(shape, parts, None, key_bases=bases)
    try:
        before = db.idx.reruns()
        got = db.idx.range_scan(assign, tables, radius, sum_mode=sum_mode)
        assert db.idx.reruns() == before + 1
        rc.assert_same(got, want, "key bases %s" % [hex(b) for b in bases])
    finally:
        db.close()


@path_independent
def test_an_unlabelled_index_above_the_lds_threshold_keys_are_positions():
    shape = (8, 8)
    rng = np.random.default_rng(15)
    parts = [fc.rand_codes(rng, shape, n) for n in (3000, 2500, 1200)]
    assign = np.array([[2, 0, 1], [1, 2, 0]], np.int32)
    tables = fc.rand_tables(rng, shape, 2, 3)
    v1 = np.concatenate([rc.candidates(shape, parts[p], tables[1, a]) for a, p in enumerate(assign[1])])
    radius = np.array([INF, rc.radius_for(v1, T + 1)], np.float32)
    want = rc.expected_batch(shape, parts, None, assign, tables, radius)
    assert list(np.diff(want[0])) == [6700, T + 1] and len(np.unique(want[1][:6700])) == 3000, "the partitions' keys overlap"
    idx = pyqadc.AdcIndex(8, 8)
    idx.add_partitions(parts)
    try:
        before = idx.reruns()
        got = idx.range_scan(assign, tables, radius)
        assert idx.reruns() == before + 1
        rc.assert_same(got, want, "unlabelled partitions")
    finally:
        idx.close()
