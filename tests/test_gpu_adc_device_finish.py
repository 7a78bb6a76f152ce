"""The float-ADC engine's device finish (AdcIndex.set_finish(1): adc_order_kernel + adc_replay_kernel instead of the host's
ordering and heap replay): the case grids of test_gpu_adc.py again, against the same references — the reference's own
scanner_simple build where oracle/_ref exists, else the oracle's restatement — bit for bit on keys, values and sizes.
Every grid case also asserts that no query was finished on the host (host_finishes() == 0): a silent fallback cannot pass."""
import zlib

import numpy as np
import pytest

import pyqadc
from helpers import path_independent
from test_gpu_adc import assert_heap, expected, ivf_db, rand_tables
from test_gpu_adc_rerun import descending, descending_table

pytestmark = pytest.mark.gpu


def device_index(nsq, parts, labels=None):
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    idx.set_finish(1)
    return idx


def same_arrays(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000, 100000, 2000000])
def test_flat_unlabeled_device_finish(po, nsq, n):
    """includes R > n (the sentinels stay) and, at R = 1000 on 2 x 10^6 codes, a stream far too long for the LDS sort"""
    rng = np.random.default_rng(nsq * 1000003 + n)
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 1, 1, nsq)
    idx = device_index(nsq, [codes])
    for R in (1, 7, 100, 1000):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R)
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R), 0, "n=%d R=%d" % (n, R))
    assert idx.host_finishes() == 0
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("n", [17, 1000, 100000])
def test_flat_source_order_sum_device_finish(po, nsq, n):
    rng = np.random.default_rng(7 + nsq + n)
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 1, 1, nsq)
    idx = device_index(nsq, [codes])
    for R in (1, 100):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R, sum_mode=0)
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R, sum_mode=0), 0, "sum_mode 0 R=%d" % R)
    assert idx.host_finishes() == 0
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("kind", ["dist", "ties", "negative", "constant", "nonfinite"])
@pytest.mark.parametrize("sum_mode", [1, 0])
def test_table_kinds_device_finish(po, nsq, kind, sum_mode):
    """ties and negative bring equal values and -0 / +0 to the heap's float compares; nonfinite brings -inf and -FLT_MAX"""
    rng = np.random.default_rng(zlib.crc32(("%d %s %d" % (nsq, kind, sum_mode)).encode()))
    n = 50000
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 1, 1, nsq, kind)
    idx = device_index(nsq, [codes])
    for R in (1, 7, 100, 1000):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R, sum_mode=sum_mode)
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R, sum_mode), 0, "%s R=%d" % (kind, R))
    assert idx.host_finishes() == 0
    idx.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
def test_more_room_than_codes_device_finish(po, nsq):
    """R > n: the heap keeps R - n sentinels (0, FLT_MAX) exactly where the reference's pushes leave them"""
    rng = np.random.default_rng(90 + nsq)
    for n, R in ((1, 2), (100, 101), (100, 4096), (3000, 4000)):
        codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
        tables = rand_tables(rng, 1, 1, nsq, "negative")
        idx = device_index(nsq, [codes])
        got = idx.query_scan(np.zeros((1, 1), np.int32), tables, R)
        assert int(got[2][0]) == R
        assert_heap(got, expected(po, nsq, [codes], None, tables[0], R), 0, "n=%d R=%d" % (n, R))
        assert idx.host_finishes() == 0
        idx.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("ma", [1, 8, 24])
def test_ivf_with_labels_and_duplicate_probes_device_finish(po, nsq, ma):
    rng = np.random.default_rng(100 * nsq + ma)
    parts, labels = ivf_db(rng, nsq)
    idx = device_index(nsq, parts, labels)
    nq = 6
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    if ma > 1:
        assign[0, 1] = assign[0, 0]                        # a duplicate probe
        assign[1, :] = assign[1, 0]                        # every probe the same partition
    empty = [k for k in range(64) if len(parts[k]) == 0]
    assign[2, 0] = empty[0]                                # an empty partition first
    if ma == 1:
        assert len(parts[assign[2, 0]]) == 0               # a query that scans nothing: R sentinels
    tables = rand_tables(rng, nq, ma, nsq)
    for R in (1, 100, 1000):
        got = idx.query_scan(assign, tables, R)
        for q in range(nq):
            want = expected(po, nsq, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
            assert_heap(got, want, q, "ma=%d R=%d" % (ma, R))
    assert idx.host_finishes() == 0
    idx.close()


@path_independent
@pytest.mark.parametrize("nq", [1, 2, 64, 1000])
def test_batches_of_unequal_probe_lengths_device_finish(po, nq):
    """partitions of skewed sizes, some empty: the queries of one call scan from nothing to thousands of codes"""
    rng = np.random.default_rng(nq)
    nsq, ma, R = 8, 4, 50
    parts, labels = ivf_db(rng, nsq, n=20000)
    idx = device_index(nsq, parts, labels)
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    if nq >= 64:
        lengths = {int(sum(len(parts[k]) for k in row)) for row in assign}
        assert len(lengths) > 16
    tables = rand_tables(rng, nq, ma, nsq, "ties" if nq == 64 else "dist")
    got = idx.query_scan(assign, tables, R)
    for q in range(nq):
        want = expected(po, nsq, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
        assert_heap(got, want, q, "batch of %d" % nq)
    assert idx.host_finishes() == 0
    idx.set_finish(0)
    assert same_arrays(got, idx.query_scan(assign, tables, R)), "device and host finish differ"
    idx.close()


@path_independent
def test_heap_too_large_for_lds_is_finished_on_the_host_and_counted(po):
    """R = 20000 on 10^5 codes: beyond the 4096 entries the device replay keeps in LDS.  Same arrays as the reference; the
    queries finished on the host are counted, and only here."""
    rng = np.random.default_rng(20000)
    nsq, n, R = 8, 100000, 20000
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    tables = rand_tables(rng, 2, 1, nsq)
    idx = device_index(nsq, [codes])
    got = idx.query_scan(np.zeros((2, 1), np.int32), tables, R)
    for q in range(2):
        assert_heap(got, expected(po, nsq, [codes], None, tables[q], R), q, "R=%d" % R)
    print("host_finishes after 2 queries at R = %d: %d" % (R, idx.host_finishes()))
    assert idx.host_finishes() in (0, 2)
    before = idx.host_finishes()
    got = idx.query_scan(np.zeros((2, 1), np.int32), tables, 4096)          # the largest heap the device replay must cover
    for q in range(2):
        assert_heap(got, expected(po, nsq, [codes], None, tables[q], 4096), q, "R=4096")
    assert idx.host_finishes() == before
    idx.close()


@path_independent
@pytest.mark.parametrize("n", [20000, 100000])
def test_descending_scan_order_reruns_under_device_finish(po, n):
    """strictly decreasing candidates: the reference pushes every code, the region overflows, the batch re-runs and the order
    kernel sees every code of the query: its longest stream, sorted by radix passes through global scratch"""
    rng = np.random.default_rng(n)
    codes = descending(n, rng)
    other = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    idx = device_index(4, [codes, other])
    tdesc = descending_table().reshape(1, 1, -1)
    runs = idx.reruns()
    for R in (1, 100):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tdesc, R)
        assert_heap(got, expected(po, 4, [codes], None, tdesc[0], R), 0, "descending n=%d R=%d" % (n, R))
        assert idx.reruns() > runs, "the candidate region did not overflow: the re-run path was not taken"
        runs = idx.reruns()
    nq = 5                                                   # one overflowing query among ordinary ones
    tables = rand_tables(rng, nq, 1, 4, "dist")
    tables[2] = tdesc[0]
    got = idx.query_scan(np.zeros((nq, 1), np.int32), tables, 100)
    for q in range(nq):
        assert_heap(got, expected(po, 4, [codes], None, tables[q], 100), q, "mixed batch")
    assert idx.reruns() == runs + 1
    print("host_finishes after the overflowing batches: %d" % idx.host_finishes())
    assert idx.host_finishes() == 0, "the length of a stream is no reason to finish on the host"
    idx.close()


@path_independent
def test_finish_modes(po):
    rng = np.random.default_rng(2)
    nsq = 8
    parts, labels = ivf_db(rng, nsq, n=30000)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    nq, ma, R = 9, 8, 100
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    tables = rand_tables(rng, nq, ma, nsq, "negative")
    host = idx.query_scan(assign, tables, R)                  # the default is the host finish
    assert idx.host_finishes() == 0
    for mode in (2, -1, 7):
        with pytest.raises(pyqadc.QadcError, match="finish mode"):
            idx.set_finish(mode)
    idx.set_finish(1)
    dev = idx.query_scan(assign, tables, R)
    for q in range(nq):
        want = expected(po, nsq, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
        assert_heap(dev, want, q, "device finish")
    assert same_arrays(host, dev)
    ck, cv, off = idx.query_scan_candidates(assign, tables, R)   # the stream itself: the host path whatever the mode
    assert int(off[-1]) == len(ck) > 0
    idx.set_finish(0)
    again = idx.query_scan(assign, tables, R)
    assert same_arrays(host, again), "mode 0 after mode 1 gives other arrays"
    assert idx.host_finishes() == 0
    idx.close()
