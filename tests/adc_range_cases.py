"""What a float-ADC range search (pyqadc.AdcIndex.range_scan / range_search; qadc_adc_range_* in include/qadc.h; DESIGN.md section
11.13) must return, restated in numpy, and the cases the GPU tests share.

For one query: every row of the probed partitions, in assign order, whose key passes every filter and whose candidate is < radius as
a float32 compare (NaN on either side: not kept; equal: not kept), ordered ascending by the 64-bit word
(order_image(candidate) << 32) | key.  The candidate is the sum of the code's table entries in the grouping of host/float_sum.hpp
(sum_mode 1: as the reference compiles; 0: source order from +0), every add rounded to float32.  tests/test_adc_range_host.py holds the
host twin scanner_simple::range_scan to expected(); the GPU tests hold the device to it."""
import numpy as np

import adc_filter_compose as fc


def gather(shape, codes, table):
    """-> t float32 [n][nsq]: the table entries of every code in the source's order (4 bits: low nibble = even sub-quantizer)"""
    nsq, bits = shape
    table = np.asarray(table, np.float32).reshape(nsq, 1 << bits)
    if bits == 4:
        c = np.asarray(codes, np.uint8).reshape(-1, nsq // 2)
        digits = np.empty((len(c), nsq), np.intp)
        digits[:, 0::2] = c & 15
        digits[:, 1::2] = c >> 4
    else:
        digits = np.asarray(codes).reshape(-1, nsq).astype(np.intp)
    return table[np.arange(nsq), digits]


def candidates(shape, codes, table, sum_mode=1):
    """-> float32 [n]: adc_sum<nsq> of host/float_sum.hpp on every code"""
    nsq = shape[0]
    t = gather(shape, codes, table)
    c = [t[:, m] for m in range(nsq)]
    with np.errstate(all="ignore"):
        if sum_mode == 0:
            s = np.zeros(len(t), np.float32)
            for m in range(nsq):
                s = s + c[m]
            return s
        if nsq == 2:
            return c[0] + c[1]
        if nsq == 4:
            return (c[1] + c[2]) + (c[3] + c[0])
        if nsq == 8:
            return ((c[1] + c[2]) + (c[3] + c[4])) + ((c[5] + c[6]) + (c[7] + c[0]))
        assert nsq in (16, 32)
        a = (c[5] + c[6]) + (c[7] + c[8])
        b = (c[1] + c[2]) + (c[3] + c[4])
        cc = (c[11] + c[12]) + (c[9] + c[10])
        d = (c[13] + c[14]) + (c[15] + c[0])
        s = ((a + b) + cc) + d
        for j in range(16, nsq, 4):
            s = s + ((c[j + 2] + c[j + 3]) + (c[j] + c[j + 1]))
        return s


def order_image(v):
    """the order-preserving uint32 image of float32 values: -x < -y < -0 < +0 < y < x"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def words(keys, vals):
    return (order_image(vals).astype(np.uint64) << np.uint64(32)) | np.asarray(keys, np.uint32).astype(np.uint64)


def expected(shape, parts, labels, tables, radius, filters=(), sum_mode=1, key_bases=None):
    """(keys uint32, values float32) of one query: parts / labels / key_bases = its probed partitions in assign order, tables
    [ma][nsq << bits], filters = (S, mode) pairs (or None) a row must all pass"""
    nsq, bits = shape
    tables = np.asarray(tables, np.float32).reshape(len(parts), nsq << bits)
    keys = np.concatenate(fc.keys_of(parts, labels, key_bases) + [np.zeros(0, np.uint32)]).astype(np.uint32)
    vals = np.concatenate([candidates(shape, p, tables[a], sum_mode) for a, p in enumerate(parts)] + [np.zeros(0, np.float32)])
    with np.errstate(invalid="ignore"):
        keep = vals.astype(np.float32) < np.float32(radius)
    for f in filters:
        if f is not None:
            keep &= ~fc.dropped(keys, f[0], f[1])
    keys, vals = keys[keep], vals[keep].astype(np.float32)
    order = np.argsort(words(keys, vals), kind="stable")
    return keys[order], vals[order]


def expected_batch(shape, parts, labels, assign, tables, radius, filters=None, index_filter=None, sum_mode=1, key_bases=None):
    """-> (lims int64 [nq+1], keys, values) of a batch: assign [nq][ma] over the index's partitions, tables [nq][ma][...], radius [nq]"""
    assign = np.asarray(assign).reshape(len(tables), -1)
    radius = np.broadcast_to(np.asarray(radius, np.float32), (len(assign),))
    lims, ks, vs = [0], [], []
    for q, probes in enumerate(assign):
        k, v = expected(shape, [parts[p] for p in probes], None if labels is None else [labels[p] for p in probes], tables[q], radius[q],
                        [index_filter, None if filters is None else filters[q]], sum_mode,
                        None if key_bases is None else [key_bases[p] for p in probes])
        ks.append(k)
        vs.append(v)
        lims.append(lims[-1] + len(k))
    return np.array(lims, np.int64), np.concatenate(ks).astype(np.uint32), np.concatenate(vs).astype(np.float32)


def assert_same(got, want, what=""):
    """lims, keys and the value bit patterns, exactly"""
    gl, gk, gv = (np.asarray(x) for x in got)
    wl, wk, wv = want
    assert np.array_equal(gl, wl), "%s: lims %s, expected %s" % (what, gl, wl)
    assert np.array_equal(gk.view(np.uint32), wk), "%s: keys differ" % what
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), "%s: values differ" % what


def quarter_tables(rng, shape, nq, ma, top=8):
    """tables whose entries are small multiples of 0.25: every sum is exact in any grouping and ties abound"""
    nsq, bits = shape
    return (rng.integers(0, top, (nq, ma, nsq << bits)).astype(np.float32) * np.float32(0.25)).astype(np.float32)


def radius_for(vals, rows):
    """a radius that keeps exactly the `rows` smallest of vals (distinct at the cut), float32"""
    s = np.sort(np.asarray(vals, np.float32))
    assert rows == len(s) or s[rows - 1] < s[rows], "the cut falls into a tie"
    return np.float32(np.inf) if rows == len(s) else s[rows]


# ---- the cases of tests/test_gpu_adc_range.py: name -> dict(parts, labels, assign, tables, radius) per shape ----

EDGE_SIZES = [0, 1, 1023, 1025, 2049]   # 256 x 4 rows per iteration end at 1024; the minimum run ends at 2048; one probed empty partition


def kernel_edges(shape, seed=1):
    """five partitions of the edge sizes, three queries probing three each (ma = 3), the empty one among them; radii keep about a third"""
    rng = np.random.default_rng(seed + 100 * shape[0] + shape[1])
    parts = [fc.rand_codes(rng, shape, n) for n in EDGE_SIZES]
    total = sum(EDGE_SIZES)
    perm = rng.permutation(3 * total)[:total].astype(np.uint32)
    labels = [perm[sum(EDGE_SIZES[:i]):sum(EDGE_SIZES[:i + 1])] for i in range(len(EDGE_SIZES))]
    assign = np.array([[4, 0, 2], [1, 3, 0], [2, 4, 3]], np.int32)
    tables = fc.rand_tables(rng, shape, 3, 3)
    radius = []
    for q in range(3):
        v = np.concatenate([candidates(shape, parts[p], tables[q, a]) for a, p in enumerate(assign[q])])
        radius.append(np.sort(v)[len(v) // 3])
    return dict(parts=parts, labels=labels, assign=assign, tables=tables, radius=np.array(radius, np.float32))


def ties(shape, seed=2):
    """quarter tables; partitions 1 and 2 hold one row each with the same label and the same code; two queries, the radius a value
    present in the data and its nextafter"""
    rng = np.random.default_rng(seed + 100 * shape[0] + shape[1])
    one = fc.rand_codes(rng, shape, 1)
    parts = [fc.rand_codes(rng, shape, 600), one, one.copy(), fc.rand_codes(rng, shape, 300)]
    labels = [rng.integers(0, 200, 600).astype(np.uint32), np.array([7], np.uint32), np.array([7], np.uint32),
              rng.integers(0, 200, 300).astype(np.uint32)]
    assign = np.array([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32)
    t = quarter_tables(rng, shape, 1, 1)[0, 0]
    tables = np.broadcast_to(t, (2, 4, len(t))).copy()                           # one table everywhere: the twin rows tie exactly
    present = candidates(shape, one, t)[0]
    return dict(parts=parts, labels=labels, assign=assign, tables=tables,
                radius=np.array([present, np.nextafter(present, np.float32(np.inf))], np.float32), present=present)
