"""What a filtered float-ADC search (pyqadc.AdcFilter, qadc_adc_index_set_filter) must return: the heap
arrays of scanner_simple::query_scan over the partitions from which the dropped rows have been deleted, with the surviving rows'
keys given as labels.  Nothing is computed here but that reduction; the arrays come from the helpers the unfiltered tests use —
test_gpu_adc.expected (8-bit codes), adc4_compose.expected (4-bit codes) and adc16_compose.heap (16-bit codes)."""
import numpy as np

import adc16_compose as a16
import adc4_compose as a4

SHAPES = [(4, 8), (8, 8), (16, 8), (16, 4), (32, 4), (2, 16), (4, 16), (8, 16)]


def shape_id(s):
    return "%dx%d" % s


def code_dtype(bits):
    return np.uint16 if bits == 16 else np.uint8


def rand_codes(rng, shape, n):
    """n random codes as the index of that shape takes them: uint8 [n][nsq], uint8 [n][M/2] (4 bits) or uint16 [n][nsq]"""
    nsq, bits = shape
    if bits == 4:
        return rng.integers(0, 256, (n, nsq // 2), dtype=np.uint8)
    return rng.integers(0, 1 << bits, (n, nsq)).astype(code_dtype(bits))


def rand_tables(rng, shape, nq, ma):
    """[nq][ma][nsq << bits], squared-distance-like"""
    nsq, bits = shape
    t = (rng.random((nq, ma, nsq << bits), dtype=np.float32) * np.float32(4.0)) ** 2
    return np.ascontiguousarray(t, np.float32)


def keys_of(parts, labels, key_bases=None):
    """the key of every row, per partition: its label, else key_base + position"""
    out = []
    for a, p in enumerate(parts):
        if labels is not None and labels[a] is not None:
            out.append(np.ascontiguousarray(labels[a], np.uint32))
        else:
            base = 0 if key_bases is None else int(key_bases[a])
            out.append((np.arange(len(p), dtype=np.uint64) + base).astype(np.uint32))
    return out


def dropped(keys, S, mode):
    """bool per key: the filter (S, mode) drops it"""
    inside = np.isin(keys, np.asarray(S, np.uint32))
    return inside if mode == "exclude" else ~inside


def reduce(parts, labels, S, mode, key_bases=None):
    """-> (parts, labels) without the dropped rows; the labels are the surviving keys"""
    keys = keys_of(parts, labels, key_bases)
    keep = [~dropped(k, S, mode) for k in keys]
    return [np.asarray(p)[m] for p, m in zip(parts, keep)], [k[m] for k, m in zip(keys, keep)]


def unfiltered(po, shape, parts, labels, tables, R, sum_mode=1):
    """heap arrays (keys, values) of one query through the helper of the shape's width; labels: one array per partition"""
    nsq, bits = shape
    if bits == 8:
        from test_gpu_adc import expected
        return expected(po, nsq, parts, labels, tables, R, sum_mode)
    if bits == 4:
        return a4.expected(po, nsq, parts, labels, tables, R, sum_mode)
    return a16.heap(po, nsq, parts, labels, tables, R, sum_mode)


def expected(po, shape, parts, labels, tables, R, S, mode, sum_mode=1, key_bases=None):
    """heap arrays (keys, values) of one query under the filter (S, mode): parts / labels / key_bases = the probed partitions in
    assign order, tables [ma][nsq << bits]"""
    rp, rl = reduce(parts, labels, S, mode, key_bases)
    return unfiltered(po, shape, rp, rl, tables, R, sum_mode)


def assert_heap(got, want, q, what=""):
    keys, vals, sizes = got
    wk, wv = want
    n = int(sizes[q])
    assert n == len(wk), "%s query %d: heap size %d, expected %d" % (what, q, n, len(wk))
    assert np.array_equal(np.asarray(keys[q, :n]).view(np.uint32), wk), "%s query %d: keys differ" % (what, q)
    assert np.array_equal(np.asarray(vals[q, :n]).view(np.uint32), wv.view(np.uint32)), "%s query %d: values differ" % (what, q)
