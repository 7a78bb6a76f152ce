"""The float-ADC engine for whole-byte PQ codes (pyqadc.AdcIndex, qadc_adc_* in include/qadc.h) against the reference's
scanner_simple::query_scan: the heap ARRAYS (keys, values bit for bit, sizes) of kv_binheap<unsigned,float>(R) after each query.
Expected arrays come from the reference's own scanner_simple + scan_standard as compiled (oracle/_ref) where that build
exists, else from the oracle's restatement; sum_mode 0 (source order) always from the restatement."""
import zlib

import numpy as np
import pytest

import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(np.finfo(np.float32).max)


def expected(po, nsq, parts, labels, tables, R, sum_mode=1):
    """heap arrays of one query: parts / labels = the probed partitions in assign order, tables [ma][nsq*256]"""
    tables = np.ascontiguousarray(tables, np.float32).reshape(len(parts), nsq * 256)
    if sum_mode == 1 and po.have_ref_float():
        return po.reff_scan_standard_u8(nsq, parts, labels, tables, R)
    return po.scan_standard_u8(nsq, parts, labels, tables, R, sum_mode=sum_mode)


def assert_heap(got, want, q, what=""):
    keys, vals, sizes = got
    wk, wv = want
    n = int(sizes[q])
    assert n == len(wk), "%s query %d: heap size %d, expected %d" % (what, q, n, len(wk))
    assert np.array_equal(keys[q, :n], wk), "%s query %d: keys differ" % (what, q)
    assert np.array_equal(vals[q, :n].view(np.uint32), wv.view(np.uint32)), "%s query %d: values differ" % (what, q)


def rand_tables(rng, nq, ma, nsq, kind="dist"):
    shape = (nq, ma, nsq, 256)
    if kind == "dist":           # squared-distance-like, continuous
        t = (rng.random(shape, dtype=np.float32) * np.float32(4.0)) ** 2
    elif kind == "ties":         # small integers: massive ties among candidates
        t = rng.integers(0, 4, shape).astype(np.float32)
    elif kind == "negative":     # negative entries too
        t = rng.normal(size=shape).astype(np.float32)
    elif kind == "constant":
        t = np.full(shape, np.float32(1.5))
    elif kind == "nonfinite":    # NaN of either sign, +-inf, FLT_MAX in some entries
        t = rng.random(shape, dtype=np.float32)
        specials = np.array([np.nan, -np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX], np.float32)
        nan_neg = np.float32(np.nan)
        m = rng.random(shape) < 0.01
        t[m] = specials[rng.integers(0, len(specials), int(m.sum()))]
        neg = rng.random(shape) < 0.002
        t[neg] = -np.abs(nan_neg)                   # NaN with the sign bit set
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(t.reshape(nq, ma, nsq * 256), np.float32)


def flat_index(nsq, codes):
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions([codes])
    return idx


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000, 100000, 2000000])
def test_flat_unlabeled_matches_reference(po, nsq, n):
    rng = np.random.default_rng(nsq * 1000003 + n)
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 1, 1, nsq)
    idx = flat_index(nsq, codes)
    for R in (1, 7, 100, 1000):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R)
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R), 0, "n=%d R=%d" % (n, R))
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("n", [17, 1000, 100000])
def test_flat_source_order_sum(po, nsq, n):
    rng = np.random.default_rng(7 + nsq + n)
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 1, 1, nsq)
    idx = flat_index(nsq, codes)
    for R in (1, 100):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R, sum_mode=0)
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R, sum_mode=0), 0, "sum_mode 0 R=%d" % R)
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("kind", ["ties", "negative", "constant", "nonfinite"])
@pytest.mark.parametrize("sum_mode", [1, 0])
def test_special_tables(po, nsq, kind, sum_mode):
    rng = np.random.default_rng(zlib.crc32(("%d %s %d" % (nsq, kind, sum_mode)).encode()))
    n = 50000
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 1, 1, nsq, kind)
    idx = flat_index(nsq, codes)
    for R in (1, 7, 100, 1000):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R, sum_mode=sum_mode)
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R, sum_mode), 0, "%s R=%d" % (kind, R))
    idx.close()


def ivf_db(rng, nsq, K=64, n=60000):
    """K partitions of skewed sizes, some empty, labels = a permutation of 0 .. n-1"""
    w = rng.pareto(1.2, K) + 0.05
    w[rng.choice(K, 6, replace=False)] = 0
    sizes = np.floor(w / w.sum() * n).astype(np.int64)
    perm = rng.permutation(int(sizes.sum())).astype(np.uint32)
    parts, labels, o = [], [], 0
    for s in sizes:
        parts.append(rng.integers(0, 256, (int(s), nsq), dtype=np.uint8))
        labels.append(perm[o:o + s].copy())
        o += s
    return parts, labels


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("ma", [1, 8, 24])
def test_ivf_with_labels_and_duplicate_probes(po, nsq, ma):
    rng = np.random.default_rng(100 * nsq + ma)
    parts, labels = ivf_db(rng, nsq)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    assert idx.partition_count() == 64 and idx.partition_size(3) == len(parts[3])
    nq = 6
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    if ma > 1:
        assign[0, 1] = assign[0, 0]                        # a duplicate probe
        assign[1, :] = assign[1, 0]                        # every probe the same partition
    empty = [k for k in range(64) if len(parts[k]) == 0]
    assign[2, 0] = empty[0]                                # an empty partition first
    tables = rand_tables(rng, nq, ma, nsq)
    for R in (1, 100, 1000):
        got = idx.query_scan(assign, tables, R)
        for q in range(nq):
            want = expected(po, nsq, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
            assert_heap(got, want, q, "ma=%d R=%d" % (ma, R))
    idx.close()


@path_independent
@pytest.mark.parametrize("nq", [1, 2, 64, 1000])
def test_batches_equal_their_per_query_results(po, nq):
    rng = np.random.default_rng(nq)
    nsq, ma, R = 8, 4, 50
    parts, labels = ivf_db(rng, nsq, n=20000)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    tables = rand_tables(rng, nq, ma, nsq, "ties" if nq == 64 else "dist")
    got = idx.query_scan(assign, tables, R)
    for q in range(nq):
        want = expected(po, nsq, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
        assert_heap(got, want, q, "batch of %d" % nq)
    idx.close()


@path_independent
def test_one_query_on_ten_million_codes(po):
    rng = np.random.default_rng(10)
    n, nsq = 10_000_000, 8
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 1, 1, nsq)
    idx = flat_index(nsq, codes)
    for R in (1, 100):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R)
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R), 0, "10^7 R=%d" % R)
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 16])
def test_candidate_stream_replays_to_the_direct_arrays(po, nsq):
    rng = np.random.default_rng(33 + nsq)
    parts, labels = ivf_db(rng, nsq)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    nq, ma, R = 5, 8, 64
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    tables = rand_tables(rng, nq, ma, nsq, "nonfinite")
    direct = idx.query_scan(assign, tables, R)
    keys, vals, offsets = idx.query_scan_candidates(assign, tables, R)
    assert offsets[0] == 0 and offsets[-1] == len(keys)
    sk = np.zeros(R, np.uint32)
    sv = (FLT_MAX - np.arange(R, dtype=np.float32)).astype(np.float32)   # the R sentinel pushes (0, FLT_MAX - t)
    for q in range(nq):
        a, b = int(offsets[q]), int(offsets[q + 1])
        assert not np.isnan(vals[a:b]).any()
        want = po.heap_replay_f32(np.concatenate([sk, keys[a:b]]), np.concatenate([sv, vals[a:b]]), R)
        assert_heap(direct, want, q, "stream replay")
    need = int(offsets[-1])
    assert need > 0
    rc, _, _, off2 = idx.query_scan_candidates_raw(assign, tables, R, 1, need - 1)
    assert rc == pyqadc.QADC_E_CAPACITY and int(off2[-1]) == need
    with pytest.raises(pyqadc.QadcError):
        idx.query_scan_candidates(assign, tables, R, capacity=need - 1)
    idx.close()


@path_independent
def test_refusals():
    for sq_count, sq_bits in ((16, 4), (32, 4), (8, 16), (4, 16), (2, 16), (32, 8)):
        with pytest.raises(pyqadc.QadcError, match="Supported configurations are"):
            pyqadc.AdcIndex(sq_count, sq_bits)
    rng = np.random.default_rng(0)
    codes = [rng.integers(0, 256, (100, 8), dtype=np.uint8) for _ in range(2)]
    idx = pyqadc.AdcIndex(8, 8)
    with pytest.raises(pyqadc.QadcError, match="labels"):     # mixed inside one call
        idx.add_partitions(codes, [np.arange(100, dtype=np.uint32), None])
    idx.add_partitions(codes[:1], [np.arange(100, dtype=np.uint32)])
    with pytest.raises(pyqadc.QadcError, match="labels"):     # mixed over two calls
        idx.add_partitions(codes[1:])
    tables = rand_tables(rng, 1, 1, 8)
    for a in (1, -1):
        with pytest.raises(pyqadc.QadcError, match="partition"):
            idx.query_scan(np.array([[a]], np.int32), tables, 10)
    with pytest.raises(pyqadc.QadcError):
        idx.query_scan(np.zeros((1, 1), np.int32), tables, 0)
    with pytest.raises(pyqadc.QadcError):
        idx.query_scan(np.zeros((1, 1), np.int32), tables, 10, sum_mode=2)
    idx.close()
