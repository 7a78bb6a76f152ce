"""The float-ADC engine's overflow path: a scan order whose candidates strictly decrease makes the reference push every code,
so the engine keeps every code too, its candidate region overflows and the batch is re-run with a grown region.  The heaps
after the re-run must still be the reference's, and the regions of later calls on the same index are sized for those calls."""
import numpy as np
import pytest

import pyqadc
from helpers import path_independent
from test_gpu_adc import assert_heap, expected, rand_tables

pytestmark = pytest.mark.gpu


def descending(n, rng):
    """NSQ-4 codes whose candidates are n, n-1, ..., 1 in scan order under descending_table(): v = 65536 c0 + 256 c1 + c2
    (every partial sum is an integer below 2^24, so exact in float whatever the grouping); c3 looks up zeros."""
    v = np.arange(n, 0, -1, dtype=np.int64)
    codes = np.stack([v >> 16, (v >> 8) & 255, v & 255, rng.integers(0, 256, n)], axis=1).astype(np.uint8)
    return codes


def descending_table():
    c = np.arange(256, dtype=np.float32)
    return np.concatenate([c * 65536, c * 256, c, np.zeros(256, np.float32)]).astype(np.float32)


@path_independent
@pytest.mark.parametrize("n", [20000, 100000])
def test_descending_scan_order_reruns_and_stays_exact(po, n):
    rng = np.random.default_rng(n)
    codes = descending(n, rng)
    other = rng.integers(0, 256, (n, 4), dtype=np.uint8)     # partition 1: random codes in random order
    idx = pyqadc.AdcIndex(4, 8)
    idx.add_partitions([codes, other])
    tdesc = descending_table().reshape(1, 1, -1)
    runs = idx.reruns()
    for R in (1, 100):
        got = idx.query_scan(np.zeros((1, 1), np.int32), tdesc, R)
        assert_heap(got, expected(po, 4, [codes], None, tdesc[0], R), 0, "descending n=%d R=%d" % (n, R))
        assert idx.reruns() > runs, "the candidate region did not overflow: the re-run path was not taken"
        runs = idx.reruns()
        keys, vals, offsets = idx.query_scan_candidates(np.zeros((1, 1), np.int32), tdesc, R)
        assert int(offsets[1]) == n                  # every code is a push of the reference: all of them are in the stream
        assert np.array_equal(vals, np.arange(n, 0, -1).astype(np.float32))
        runs = idx.reruns()

    # one overflowing query in a batch: its region grows, the others keep theirs, every heap is the reference's
    nq = 5
    tables = rand_tables(rng, nq, 1, 4, "dist")
    tables[2] = tdesc[0]
    got = idx.query_scan(np.zeros((nq, 1), np.int32), tables, 100)
    for q in range(nq):
        assert_heap(got, expected(po, 4, [codes], None, tables[q], 100), q, "mixed batch")
    assert idx.reruns() == runs + 1
    runs = idx.reruns()

    # a later ordinary batch on the same index (random codes in random order) is sized for itself: no re-run, same heaps
    # as the reference.  (Partition 0 is no ordinary list even under random tables: its codes walk c0, c1 in order.)
    nq = 64
    tables = rand_tables(rng, nq, 1, 4, "dist")
    got = idx.query_scan(np.ones((nq, 1), np.int32), tables, 100)
    for q in range(nq):
        assert_heap(got, expected(po, 4, [other], None, tables[q], 100), q, "batch after the re-runs")
    assert idx.reruns() == runs
    idx.close()


@path_independent
def test_descending_order_over_ivf_probes(po):
    """the same over several probes: each probe's partition descends and the probes come in descending order of their
    values, so the whole scan order of the query descends across partition ends; keys are labels"""
    rng = np.random.default_rng(3)
    n = 30000
    codes = descending(n, rng)
    cuts = [0, 7000, 7001, 19000, n]
    parts = [codes[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [codes[:0]]
    labels = [rng.permutation(len(p)).astype(np.uint32) + np.uint32(1000 * i) for i, p in enumerate(parts)]
    idx = pyqadc.AdcIndex(4, 8)
    idx.add_partitions(parts, labels)
    assign = np.array([[0, 4, 1, 2, 3, 2]], np.int32)      # an empty partition and a duplicate probe in between
    tables = np.repeat(descending_table().reshape(1, 1, -1), 6, axis=1)
    for R in (1, 64, 1000):
        got = idx.query_scan(assign, tables, R)
        want = expected(po, 4, [parts[k] for k in assign[0]], [labels[k] for k in assign[0]], tables[0], R)
        assert_heap(got, want, 0, "ivf descending R=%d" % R)
    assert idx.reruns() >= 1
    idx.close()
