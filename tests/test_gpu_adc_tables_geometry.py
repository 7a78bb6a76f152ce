"""The float-ADC feeders at the launch geometries of tests/adc_tables_cases.py (host/adc_tables_plan.hpp): a workgroup that walks
several sub-quantizers with several probes in LDS, the loop that halves the probes until the residuals fit, a short last probe
group, the largest dimension, 16-bit sub-quantizers with several probes, several sub-quantizers and many centroid blocks per
workgroup, and the second trip of the 8-bit encoder's outer loop.  tests/test_adc_tables_plan_host.py asserts on a CPU that every
case is planned as its name says.

Assign and every table entry are compared bit for bit with the composition of the oracle's functions (tests/adc_compose.py,
tests/adc16_compose.py), the heaps with the oracle's scan of the composed tables, the codes with the oracle's encoder; nothing
is compared with another call of the library.  The composition runs query block by query block on a pool of threads (the oracle's
functions keep no state), so that the large cases hold no second copy of their tables and the CPU's share stays short.

Every test prints the plan of its case, the bytes of its tables and the wall times of the GPU call and of the composition."""
import os
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import adc16_compose as a16
import adc_compose as ac
import adc_tables_cases as cases
import pyqadc
from helpers import path_independent
from test_gpu_adc import assert_heap, expected, ivf_db

pytestmark = pytest.mark.gpu

WORKERS = max(1, min(16, os.cpu_count() or 1))
FORMS = [(0, 1), (1, 1), (0, 0), (1, 0)]                         # (table_form, sum_mode): both forms in both sum modes
IDS = ["direct-sum1", "expansion-sum1", "direct-sum0", "expansion-sum0"]


def seed_of(name):
    return zlib.crc32(name.encode())


def dense_rotation(rng, dim):
    """a dense [dim][dim] matrix with rows of about unit norm: every output component is a sum over all `dim` inputs, which is all
    the feeder's rotation step can tell (an orthonormal one would cost a 4096 x 4096 QR and check no more)"""
    return (rng.standard_normal((dim, dim), dtype=np.float32) / np.float32(np.sqrt(dim))).astype(np.float32)


def blocks(n, size):
    return [slice(lo, min(n, lo + size)) for lo in range(0, n, size)]


def on_pool(fn, items):
    with ThreadPoolExecutor(WORKERS) as pool:
        return list(pool.map(fn, items))


def report(case, what, gpu_s, cpu_s):
    print("GEOMETRY %s %s: plan %s, tables %d bytes, GPU call %.3f s, composition %.3f s"
          % (case.c["name"], what, case.c["plan"], cases.table_bytes(case.c), gpu_s, cpu_s))


def differing(got, want):
    """(count, first index) of the entries whose float bits differ"""
    diff = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    n = int(diff.sum())
    return n, (tuple(int(i) for i in np.argwhere(diff)[0]) if n else None)


class Feeder:
    """The quantizers, a small database and the GPU index of one case; queries [nq][dim].  8-bit sub-quantizers: K = 64
    partitions of skewed sizes, six empty; 16-bit: K = 8, one empty.  Both labelled."""

    def __init__(self, c):
        rng = np.random.default_rng(seed_of(c["name"]))
        self.c, self.nsq, self.dim, self.nq, self.ma = c, c["nsq"], c["dim"], c["nq"], c["ma"]
        self.wide = c["centroids"] == 65536
        ds = self.dim // self.nsq
        self.codebooks = rng.standard_normal((self.nsq, c["centroids"], ds), dtype=np.float32)
        self.rotation = dense_rotation(rng, self.dim) if c["opq"] else None
        if self.wide:
            self.K = 8
            sizes = [700, 0, 310, 1, 500, 17, 250, 138]
            perm = rng.permutation(sum(sizes)).astype(np.uint32)
            self.parts = [rng.integers(0, 65536, (s, self.nsq)).astype(np.uint16) for s in sizes]
            self.labels = list(np.split(perm, np.cumsum(sizes)[:-1]))
            self.idx = pyqadc.AdcIndex.create16(self.nsq)
        else:
            self.K = 64
            self.parts, self.labels = ivf_db(rng, self.nsq, self.K, 6000)
            self.idx = pyqadc.AdcIndex(self.nsq, 8)
        assert self.ma <= self.K
        self.coarse = (rng.standard_normal((self.K, self.dim), dtype=np.float32) * np.float32(2)).astype(np.float32)
        self.idx.add_partitions(self.parts, self.labels)
        self.idx.set_pq(self.codebooks)
        self.idx.set_rotation(self.rotation)
        self.idx.set_coarse(self.coarse)
        self.queries = (rng.standard_normal((self.nq, self.dim), dtype=np.float32) + self.coarse[rng.integers(0, self.K, self.nq)]).astype(np.float32)
        self._res = {}

    def assign(self, po, sum_mode):
        return ac.assign(po, self.queries, self.coarse, self.ma, sum_mode)

    def residuals(self, a, qs):
        """adc_compose.residuals of the queries `qs` (a slice or an index list) -> [len][ma][dim]; kept per assignment, since both
        sum modes nearly always probe the same partitions and the rotation is the slow step"""
        key = (a[qs].tobytes(), str(qs))
        if key not in self._res:
            self._res[key] = ac.residuals(self.queries[qs], self.coarse, a[qs], self.rotation)
        return self._res[key]

    def tables(self, po, a, qs, expansion, sum_mode):
        """the composed tables of the queries `qs` -> [len][ma][nsq * centroids]"""
        res = self.residuals(a, qs)
        n = res.shape[0]
        if self.wide:
            f = a16.tables_expansion if expansion else a16.tables_direct
            return f(po, self.codebooks, res.reshape(n * self.ma, self.dim), sum_mode).reshape(n, self.ma, -1)
        return ac.tables(po, self.codebooks, res, int(expansion), sum_mode)

    def heap(self, po, a, tables_q, q, R, sum_mode):
        parts, labels = [self.parts[k] for k in a[q]], [self.labels[k] for k in a[q]]
        if self.wide:
            return a16.heap(po, self.nsq, parts, labels, tables_q, R, sum_mode)
        return expected(po, self.nsq, parts, labels, tables_q, R, sum_mode)

    def probe_group_ends(self):
        """the first and the last probe of every probe group of the plan"""
        p = self.c["plan"]
        ends = set()
        for y in range(p["pgroups"]):
            ends |= {y * p["probes"], min(self.ma, (y + 1) * p["probes"]) - 1}
        return sorted(ends)


def make_fixture(case_list):
    @pytest.fixture(scope="module", params=case_list, ids=[c["name"] for c in case_list])
    def fx(request):
        f = Feeder(request.param)
        yield f
        f.idx.close()
    return fx


case8 = make_fixture(cases.TABLES8)
case16 = make_fixture(cases.TABLES16)


def check_every_entry(po, f, table_form, sum_mode, per_block):
    """search_tables against the composition, query block by query block"""
    t0 = time.perf_counter()
    got_a, got_t = f.idx.search_tables(f.queries, f.ma, table_form, sum_mode)
    gpu_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_a = f.assign(po, sum_mode)
    assert np.array_equal(got_a, want_a), "assign differs"

    def one(qs):
        n, first = differing(got_t[qs], f.tables(po, want_a, qs, bool(table_form), sum_mode))
        return n, (None if first is None else (first[0] + qs.start,) + first[1:])

    out = on_pool(one, blocks(f.nq, per_block))
    report(f, "form %d sum_mode %d" % (table_form, sum_mode), gpu_s, time.perf_counter() - t0)
    bad = [(n, first) for n, first in out if n]
    assert not bad, "%d table entries differ, first at (query, probe, entry) %s" % (sum(n for n, _ in bad), bad[0][1])


# ---- 8-bit sub-quantizers -----------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("table_form,sum_mode", FORMS, ids=IDS)
def test_tables8_equal_the_composition(po, case8, table_form, sum_mode):
    check_every_entry(po, case8, table_form, sum_mode, per_block=max(1, -(-case8.nq // (2 * WORKERS))))


@path_independent
@pytest.mark.parametrize("table_form,sum_mode", [(0, 1), (1, 1), (1, 0)], ids=["direct-sum1", "expansion-sum1", "expansion-sum0"])
def test_search8_heaps_on_tables_of_workgroups_that_walk_every_sub_quantizer(po, table_form, sum_mode):
    """msplit 1, probes 9, a short last group: the scan reads tables laid out by those workgroups"""
    f = Feeder(cases.by_name(cases.TABLES8, "msplit1_probes9_short_last"))
    try:
        check_heaps(po, f, table_form, sum_mode)
    finally:
        f.idx.close()


def check_heaps(po, f, table_form, sum_mode):
    picked = [0, f.nq // 2, f.nq - 1]
    want_a = f.assign(po, sum_mode)
    want_t = f.tables(po, want_a, picked, bool(table_form), sum_mode)
    for R in (1, 100):
        t0 = time.perf_counter()
        keys, vals, sizes, a = f.idx.search(f.queries, f.ma, R, table_form, sum_mode)
        report(f, "search R %d form %d sum_mode %d" % (R, table_form, sum_mode), time.perf_counter() - t0, 0.0)
        assert np.array_equal(a, want_a), "assign differs"
        for i, q in enumerate(picked):
            assert_heap((keys, vals, sizes), f.heap(po, want_a, want_t[i], q, R, sum_mode), q, "R %d" % R)


# ---- 16-bit sub-quantizers ----------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("sum_mode", [1, 0])
def test_tables16_expansion_form_equals_the_composition(po, case16, sum_mode):
    """every entry, a few queries at a time"""
    check_every_entry(po, case16, 1, sum_mode, per_block=8 if case16.nq > 8 else 1)


@path_independent
@pytest.mark.parametrize("sum_mode", [1, 0])
def test_tables16_direct_form_equals_the_composition(po, case16, sum_mode):
    """The direct form's entries do not depend on the geometry beyond where they are stored: the two large cases compare the
    first and the last probe of every probe group of the first and the last query, the small ones every entry."""
    f = case16
    if f.nq <= 8:
        check_every_entry(po, f, 0, sum_mode, per_block=1)
        return
    t0 = time.perf_counter()
    got_a, got_t = f.idx.search_tables(f.queries, f.ma, 0, sum_mode)
    gpu_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_a = f.assign(po, sum_mode)
    assert np.array_equal(got_a, want_a), "assign differs"
    picked, probes = [0, f.nq - 1], f.probe_group_ends()
    want_t = f.tables(po, want_a, picked, False, sum_mode)
    report(f, "form 0 sum_mode %d" % sum_mode, gpu_s, time.perf_counter() - t0)
    for i, q in enumerate(picked):
        for a in probes:
            n, first = differing(got_t[q, a], want_t[i, a])
            assert n == 0, "query %d probe %d: %d table entries differ, first at %s" % (q, a, n, first)


@path_independent
@pytest.mark.parametrize("table_form,sum_mode", [(1, 1), (0, 1), (1, 0)], ids=["expansion-sum1", "direct-sum1", "expansion-sum0"])
def test_search16_heaps_on_tables_of_two_probes_per_workgroup(po, table_form, sum_mode):
    f = Feeder(cases.by_name(cases.TABLES16, "2x16_msplit1_probes2"))
    try:
        check_heaps(po, f, table_form, sum_mode)
    finally:
        f.idx.close()


# ---- the 8-bit encoder's second trip --------------------------------------------------------------------------------------------

def encoder_inputs(rng, nsq, dim):
    """ENCODE_ROWS distinct vectors and codebooks that hold what tests/test_gpu_adc_search.py::test_encode_ties_duplicates_and_nan
    walks: sub-quantizer 0 grid-valued (exact ties between different centroids on the grid-valued vectors), 1 with every centroid
    twice (the first is picked), 2 with NaN centroids inside waves and at their starts, 3 with a NaN centroid at a wave's last lane;
    the vectors: random ones, grid-valued ones, and rows with NaN and infinities"""
    ds = dim // nsq
    cb = rng.standard_normal((nsq, 256, ds), dtype=np.float32)
    cb[0] = rng.integers(-1, 2, (256, ds)).astype(np.float32)
    cb[1, 128:] = cb[1, :128]
    cb[2, [0, 64, 200], rng.integers(0, ds, 3)] = np.nan
    cb[3, [63, 127], rng.integers(0, ds, 2)] = np.nan
    x = rng.standard_normal((cases.ENCODE_ROWS, dim), dtype=np.float32)
    x[100:400] = rng.integers(-1, 2, (300, dim)).astype(np.float32)
    x[1, 0] = np.nan
    x[2, dim - 1] = np.inf
    x[3, :] = -np.inf
    x[33, ds] = np.nan                                            # (rows 32, 33: the second chunks of workgroups 0 and 1 start here)
    x[996, :] = np.nan
    return cb, x


@path_independent
@pytest.mark.parametrize("case", cases.ENCODE, ids=[c["name"] for c in cases.ENCODE])
@pytest.mark.parametrize("sum_mode", [1, 0])
def test_encode_second_trip_of_the_outer_loop(po, case, sum_mode):
    rng = np.random.default_rng(seed_of(case["name"]))
    nsq, dim, n = case["nsq"], case["dim"], case["n"]
    cb, base = encoder_inputs(rng, nsq, dim)
    with np.errstate(all="ignore"):
        _, want = ac.encode(po, cb, base, None, None, sum_mode)
        ties = po.cross_dists(cb[0], base[100:400, :dim // nsq], sum_mode)
    assert ((ties == ties.min(axis=1, keepdims=True)).sum(axis=1) > 1).any(), "no exact tie among the grid rows"
    assert len(np.unique(want[:, 2])) > 1 and len(np.unique(want[:, 3])) > 1
    rows = np.arange(n) % cases.ENCODE_ROWS
    vectors = base[rows]
    t0 = time.perf_counter()
    got_a, got = pyqadc.adc_encode(cb, vectors, sum_mode=sum_mode)
    print("GEOMETRY %s sum_mode %d: plan %s, %d vectors, GPU call %.3f s" % (case["name"], sum_mode, case["plan"], n, time.perf_counter() - t0))
    assert got_a is None and got.shape == (n, nsq)
    bad = np.argwhere(got != want[rows])
    assert len(bad) == 0, "%d codes differ, first (vector, sub-quantizer) %s; the second trip starts at vector %d" % (
        len(bad), bad[0], case["plan"]["grid"] * case["plan"]["vper"])
