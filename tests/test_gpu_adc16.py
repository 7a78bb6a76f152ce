"""The float-ADC engine on 16-bit codes (pyqadc.AdcIndex.create16, qadc_adc_index_create16 in include/qadc.h): the heap ARRAYS
(keys, values bit for bit, sizes) of scanner_simple::query_scan over scan_standard<uint16_t, NSQ>, NSQ 2, 4 or 8, whose tables
[NSQ][65536] the scan kernel gathers from global memory.  Expected arrays come from tests/adc16_compose.py: numpy gathers, float32
adds in the grouping of the sum mode, the reference's own kv_binheap for the replay; its grouping is pinned to the reference as
compiled by tests/golden/ref_scan_standard_u16_cases.npz (tests/test_adc16_host.py), which is also scanned here as it is."""
import zlib

import numpy as np
import pytest

import adc16_compose as a16
import pyqadc
from adc16_compose import assert_heap
from helpers import path_independent

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(np.finfo(np.float32).max)
NSQS = [2, 4, 8]
ZERO = np.zeros((1, 1), np.int32)


def rand_tables(rng, nq, ma, nsq, kind="dist"):
    """test_gpu_adc.rand_tables with 65536 centroids per sub-quantizer"""
    shape = (nq, ma, nsq, 65536)
    if kind == "dist":           # squared-distance-like, continuous
        t = (rng.random(shape, dtype=np.float32) * np.float32(4.0)) ** 2
    elif kind == "ties":         # small integers: massive ties among candidates
        t = rng.integers(0, 4, shape).astype(np.float32)
    elif kind == "negative":     # negative entries too
        t = rng.standard_normal(shape, dtype=np.float32)
    elif kind == "constant":
        t = np.full(shape, np.float32(1.5))
    elif kind == "nonfinite":    # NaN of either sign, +-inf, FLT_MAX in some entries
        t = rng.random(shape, dtype=np.float32)
        specials = np.array([np.nan, -np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX], np.float32)
        m = rng.random(shape, dtype=np.float32) < 0.01
        t[m] = specials[rng.integers(0, len(specials), int(m.sum()))]
        neg = rng.random(shape, dtype=np.float32) < 0.002
        t[neg] = -np.abs(np.float32(np.nan))                  # NaN with the sign bit set
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(t.reshape(nq, ma, nsq * 65536), np.float32)


def rand_codes(rng, n, nsq):
    return rng.integers(0, 65536, (n, nsq)).astype(np.uint16)


def flat_index(nsq, codes):
    idx = pyqadc.AdcIndex.create16(nsq)
    idx.add_partitions([codes])
    return idx


@path_independent
@pytest.mark.parametrize("nsq", NSQS)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 1025, 65535, 65537, 200000])
def test_flat_unlabeled_matches_the_composition(po, nsq, n):
    """n around the 16-byte tail padding, the 1024 codes of one workgroup step, the 64 Ki run and over several bound levels"""
    rng = np.random.default_rng(nsq * 1000003 + n)
    codes = rand_codes(rng, n, nsq)
    tables = rand_tables(rng, 1, 1, nsq)
    idx = flat_index(nsq, codes)
    assert idx.table_dim == nsq * 65536 and idx.partition_size(0) == n
    for sum_mode in (1, 0):
        k, v = a16.stream(nsq, [codes], None, tables[0], sum_mode)
        for R in (1, 7, 100, 1000):
            got = idx.query_scan(ZERO, tables, R, sum_mode=sum_mode)
            assert_heap(got, a16.replay(po, k, v, R), 0, "n=%d R=%d sum_mode=%d" % (n, R, sum_mode))
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", NSQS)
def test_the_reference_fixture_through_query_scan(nsq):
    """the reference's own heaps, two probes; the byte form of the codes where labelled, the uint16 form where not"""
    cases = [c for c in a16.fixture() if c["nsq"] == nsq]
    idx = {}
    for labelled in (False, True):
        idx[labelled] = pyqadc.AdcIndex.create16(nsq)
        parts = cases[0]["parts"]
        if labelled:
            labels = next(c["labels"] for c in cases if c["labelled"])
            idx[labelled].add_partitions([np.ascontiguousarray(p, "<u2").view(np.uint8) for p in parts], labels)
        else:
            idx[labelled].add_partitions(parts)
    for c in cases:
        got = idx[c["labelled"]].query_scan(np.array([[0, 1]], np.int32), c["tables"], c["R"])
        assert_heap(got, (c["keys"], c["vals"]), 0, c["cid"])
    for i in idx.values():
        i.close()


@path_independent
@pytest.mark.parametrize("nsq", NSQS)
def test_the_whole_16_bit_index_selects_the_entry(po, nsq):
    """value = f(e) with f(e) != f(e & 255), f(e >> 8) and f(byteswap e) on the forced code values: a lookup that drops, shifts or
    swaps a byte of the index changes the heap"""
    rng = np.random.default_rng(160 + nsq)
    e = np.arange(65536, dtype=np.int64)
    f = ((e * 40503 + 977) % 65521).astype(np.float32)
    special = np.array(a16.SPECIAL, np.int64)
    swapped = ((special & 255) << 8) | (special >> 8)
    for s, w in zip(special, swapped):
        assert s < 256 or (f[s] != f[s & 255] and f[s] != f[s >> 8])
        assert w == s or f[w] != f[s]
    table = np.stack([f + np.float32(m) for m in range(nsq)]).reshape(1, 1, -1)      # (integers below 2^24: every sum is exact)
    codes = special[rng.integers(0, 5, (3000, nsq))].astype(np.uint16)
    codes[100:200] = rand_codes(rng, 100, nsq)
    idx = flat_index(nsq, codes)
    for sum_mode in (1, 0):
        for R in (1, 100, 3000):
            got = idx.query_scan(ZERO, table, R, sum_mode=sum_mode)
            assert_heap(got, a16.heap(po, nsq, [codes], None, table[0], R, sum_mode), 0, "R=%d" % R)
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", NSQS)
@pytest.mark.parametrize("kind", ["ties", "negative", "constant", "nonfinite"])
def test_special_tables(po, nsq, kind):
    rng = np.random.default_rng(zlib.crc32(("16 %d %s" % (nsq, kind)).encode()))
    n = 50000
    codes = rand_codes(rng, n, nsq)
    tables = rand_tables(rng, 1, 1, nsq, kind)
    idx = flat_index(nsq, codes)
    for sum_mode in (1, 0):
        k, v = a16.stream(nsq, [codes], None, tables[0], sum_mode)
        for R in (1, 7, 100, 1000):
            got = idx.query_scan(ZERO, tables, R, sum_mode=sum_mode)
            assert_heap(got, a16.replay(po, k, v, R), 0, "%s R=%d sum_mode=%d" % (kind, R, sum_mode))
    idx.close()


def ivf_db(rng, nsq, K=64, n=60000):
    """K partitions of skewed sizes, some empty, labels = a permutation of 0 .. n-1"""
    w = rng.pareto(1.2, K) + 0.05
    w[rng.choice(K, 6, replace=False)] = 0
    sizes = np.floor(w / w.sum() * n).astype(np.int64)
    perm = rng.permutation(int(sizes.sum())).astype(np.uint32)
    parts, labels, o = [], [], 0
    for s in sizes:
        parts.append(rand_codes(rng, int(s), nsq))
        labels.append(perm[o:o + s].copy())
        o += s
    return parts, labels


class Ivf:
    """one IVF database per shape with a batch of 4 queries probing 5 partitions each, and its expected streams"""

    def __init__(self, nsq, kind="dist"):
        rng = np.random.default_rng(1600 + nsq)
        self.nsq, self.nq, self.ma = nsq, 4, 5
        self.parts, self.labels = ivf_db(rng, nsq)
        self.idx = pyqadc.AdcIndex.create16(nsq)
        self.idx.add_partitions(self.parts, self.labels)
        a = rng.integers(0, 64, (self.nq, self.ma)).astype(np.int32)
        a[0, 1] = a[0, 0]                                      # a duplicate probe
        a[1, :] = a[1, 0]                                      # every probe the same partition
        a[2, 0] = [k for k in range(64) if len(self.parts[k]) == 0][0]   # an empty partition first
        self.assign = a
        self.tables = rand_tables(rng, self.nq, self.ma, nsq, kind)
        self.streams = {}

    def want(self, po, q, R, sum_mode=1):
        if (q, sum_mode) not in self.streams:
            self.streams[q, sum_mode] = a16.stream(self.nsq, [self.parts[k] for k in self.assign[q]], [self.labels[k] for k in self.assign[q]],
                                                   self.tables[q], sum_mode)
        return a16.replay(po, *self.streams[q, sum_mode], R)


@pytest.fixture(scope="module", params=NSQS)
def ivf(request):
    case = Ivf(request.param)
    yield case
    case.idx.close()


@path_independent
def test_ivf_with_labels_and_duplicate_probes(po, ivf):
    assert ivf.idx.partition_count() == 64 and ivf.idx.partition_size(3) == len(ivf.parts[3])
    for sum_mode, Rs in ((1, (1, 100, 1000)), (0, (100,))):
        for R in Rs:
            got = ivf.idx.query_scan(ivf.assign, ivf.tables, R, sum_mode=sum_mode)
            for q in range(ivf.nq):
                assert_heap(got, ivf.want(po, q, R, sum_mode), q, "R=%d sum_mode=%d" % (R, sum_mode))


@path_independent
def test_one_query_per_pass_gives_the_same_heaps(po, ivf):
    """the table budget cuts a batch of caller's tables into passes of whole queries; no result depends on it"""
    R = 100
    whole = ivf.idx.query_scan(ivf.assign, ivf.tables, R)
    stream = ivf.idx.query_scan_candidates(ivf.assign, ivf.tables, R)
    per_query = ivf.ma * ivf.nsq * 65536 * 4
    try:
        for budget in (per_query, per_query - 1, 3 * per_query):       # one query per pass (twice), three
            ivf.idx.set_table_budget(budget)
            got = ivf.idx.query_scan(ivf.assign, ivf.tables, R)
            for a, b in zip(got, whole):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            for q in range(ivf.nq):
                assert_heap(got, ivf.want(po, q, R), q, "budget %d" % budget)
            again = ivf.idx.query_scan_candidates(ivf.assign, ivf.tables, R)
            for a, b in zip(again, stream):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        ivf.idx.set_table_budget(0)


@path_independent
def test_device_finish_and_device_tables_equal_the_host_finish(po, ivf):
    torch = pytest.importorskip("torch")
    dt = torch.from_numpy(ivf.tables).cuda()
    try:
        for R in (1, 100, 1000):
            ivf.idx.set_finish(0)
            host = ivf.idx.query_scan(ivf.assign, ivf.tables, R)
            ivf.idx.set_finish(1)
            dev = ivf.idx.query_scan(ivf.assign, ivf.tables, R)
            out = ivf.idx.query_scan_device(ivf.assign, dt, R)
            mem = (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy())
            for got in (dev, mem):
                for a, b in zip(got, host):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            for q in range(ivf.nq):
                assert_heap(host, ivf.want(po, q, R), q, "R=%d" % R)
        assert ivf.idx.host_finishes() == 0
    finally:
        ivf.idx.set_finish(0)


@path_independent
def test_candidate_stream_replays_to_the_direct_arrays(po, ivf):
    R = 64
    direct = ivf.idx.query_scan(ivf.assign, ivf.tables, R)
    keys, vals, offsets = ivf.idx.query_scan_candidates(ivf.assign, ivf.tables, R)
    assert offsets[0] == 0 and offsets[-1] == len(keys)
    for q in range(ivf.nq):
        a, b = int(offsets[q]), int(offsets[q + 1])
        assert not np.isnan(vals[a:b]).any()
        assert_heap(direct, a16.replay(po, keys[a:b], vals[a:b], R), q, "stream replay")
        assert_heap(direct, ivf.want(po, q, R), q, "direct")
    need = int(offsets[-1])
    rc, _, _, off2 = ivf.idx.query_scan_candidates_raw(ivf.assign, ivf.tables, R, 1, need - 1)
    assert rc == pyqadc.QADC_E_CAPACITY and int(off2[-1]) == need


@path_independent
def test_descending_scan_order_reruns_and_stays_exact(po):
    """candidates n, n-1, ..., 1 in scan order (v = 65536 c0 + c1: integers, exact in any grouping): the reference pushes every
    code, the candidate region overflows and the batch is re-run"""
    n, nsq = 20000, 2
    v = np.arange(n, 0, -1, dtype=np.int64)
    codes = np.stack([v >> 16, v & 0xffff], axis=1).astype(np.uint16)
    e = np.arange(65536, dtype=np.float32)
    table = np.concatenate([e * 65536, e]).astype(np.float32).reshape(1, 1, -1)
    idx = flat_index(nsq, codes)
    runs = idx.reruns()
    for R in (1, 100):
        got = idx.query_scan(ZERO, table, R)
        assert_heap(got, a16.heap(po, nsq, [codes], None, table[0], R), 0, "descending R=%d" % R)
        assert idx.reruns() > runs, "the candidate region did not overflow: the re-run path was not taken"
        runs = idx.reruns()
    keys, vals, offsets = idx.query_scan_candidates(ZERO, table, 100)
    assert int(offsets[1]) == n and np.array_equal(vals, np.arange(n, 0, -1).astype(np.float32))
    idx.close()


@path_independent
def test_refusals():
    for sq_count in (1, 3, 16, 32):
        with pytest.raises(pyqadc.QadcError, match="Supported configurations are"):
            pyqadc.AdcIndex.create16(sq_count)
    rng = np.random.default_rng(0)
    idx = pyqadc.AdcIndex.create16(4)
    with pytest.raises(pyqadc.QadcError):
        idx.add_partitions([np.full((10, 4), 70000, np.int64)])              # not a 16-bit code
    idx.add_partitions([rand_codes(rng, 100, 4)])
    tables = rand_tables(rng, 1, 1, 4)
    with pytest.raises(pyqadc.QadcError, match="partition"):
        idx.query_scan(np.array([[1]], np.int32), tables, 10)
    with pytest.raises(ValueError):
        idx.query_scan(ZERO, tables[:, :, :4 * 256], 10)                     # an 8-bit table is not this index's table
    idx.close()
