"""What a float-ADC range search (pyqadc.AdcIndex.range_scan / range_search; qadc_adc_range_* in include/qadc.h; DESIGN.md section
11.13) must return, restated in numpy, and the cases the GPU tests share.

For one query: every row of the probed partitions, in assign order, whose key passes every filter and whose candidate is < radius as
a float32 compare (NaN on either side: not kept; equal: not kept), ordered ascending by the 64-bit word
(order_image(candidate) << 32) | key.  The candidate is the sum of the code's table entries in the grouping of host/float_sum.hpp
(sum_mode 1: as the reference compiles; 0: source order from +0), every add rounded to float32.  tests/test_adc_range_host.py holds the
host twin scanner_simple::range_scan to expected(); the GPU tests hold the device to it."""
import ctypes
import ctypes.util
import functools
import platform

import numpy as np

import adc_filter_compose as fc

RANGE_SORT_LDS = 4096                    # QADC_ADC_RANGE_SORT_LDS of include/qadc.h: longer segments take the radix passes
FLT_MAX = np.float32(np.finfo(np.float32).max)
FLT_MIN = np.float32(np.finfo(np.float32).tiny)
INF = np.float32(np.inf)
TINY = np.array([1], np.uint32).view(np.float32)[0]   # the smallest subnormal, 1e-45 (from its bits: see ieee below)


def ieee(fn):
    """Runs fn with subnormals as IEEE 754 has them.  A shared library built with -ffast-math (the oracle's, the reference build's) sets
    the SSE control register's flush-to-zero and denormals-are-zero bits when it is loaded, for good: from then on numpy adds subnormal
    floats to zero and compares them equal to zero, which is not the arithmetic this module restates.  x86-64 with glibc: the
    register is the last word of fenv_t; elsewhere fn runs as it is."""
    libm = ctypes.util.find_library("m") if platform.machine() in ("x86_64", "AMD64") and platform.system() == "Linux" else None
    if libm is None:
        return fn
    libm = ctypes.CDLL(libm)

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        saved, env = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        if libm.fegetenv(saved) != 0:
            return fn(*args, **kwargs)
        env.raw = saved.raw
        mxcsr = ctypes.c_uint32.from_buffer(env, 28)
        mxcsr.value &= ~0x8040                                   # FZ (bit 15) and DAZ (bit 6)
        libm.fesetenv(env)
        try:
            return fn(*args, **kwargs)
        finally:
            libm.fesetenv(saved)
    return wrapped


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


@ieee
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


@ieee
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


@ieee
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


@ieee
def radius_for(vals, rows):
    """a radius that keeps exactly the `rows` smallest of vals (distinct at the cut), float32"""
    s = np.sort(np.asarray(vals, np.float32))
    assert rows == len(s) or s[rows - 1] < s[rows], "the cut falls into a tie"
    return np.float32(np.inf) if rows == len(s) else s[rows]


# ---- the cases of tests/test_gpu_adc_range.py: name -> dict(parts, labels, assign, tables, radius) per shape ----

EDGE_SIZES = [0, 1, 1023, 1025, 2049]   # 256 x 4 rows per iteration end at 1024; the minimum run ends at 2048; one probed empty partition


@ieee
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


@ieee
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


# ---- the cases of tests/test_gpu_adc_range_edges.py; tests/test_adc_range_host.py holds the twin to the restatement on each first.  Every
# ---- builder asserts on expected() that it reaches what it is for, so a vacuous case fails on a CPU.  The returned arrays are shared
# ---- (lru_cache): read only.

def image_value(img):
    """the inverse of order_image: float32 values of uint32 images"""
    img = np.ascontiguousarray(img, np.uint32)
    return np.where(img & np.uint32(0x80000000), img & np.uint32(0x7fffffff), ~img).astype(np.uint32).view(np.float32)


def active_digits(w):
    """the radix sort's active-digit mask of the words w: bit d set iff byte d of the word differs anywhere (OR xor AND)"""
    differ = int(np.bitwise_or.reduce(w)) ^ int(np.bitwise_and.reduce(w))
    return sum(1 << d for d in range(8) if (differ >> (8 * d)) & 255)


def codes_of_digits(shape, digits):
    """digits [n][nsq] -> codes as the index of that shape takes them (4 bits: low nibble = even sub-quantizer)"""
    nsq, bits = shape
    digits = np.asarray(digits).reshape(-1, nsq)
    if bits == 4:
        return (digits[:, 0::2] | (digits[:, 1::2] << 4)).astype(np.uint8)
    return digits.astype(fc.code_dtype(bits))


def queries_of(case, sum_mode=1):
    """a batch case -> one dict per query as tests/test_adc_range_host.py's driver takes them"""
    return [dict(shape=case["shape"], parts=[case["parts"][p] for p in probes], labels=[case["labels"][p] for p in probes],
                 tables=case["tables"][q], radius=np.float32(case["radius"][q]), sum_mode=sum_mode)
            for q, probes in enumerate(case["assign"])]


def expected_of(case, sum_mode=1):
    return expected_batch(case["shape"], case["parts"], case["labels"], case["assign"], case["tables"], case["radius"], sum_mode=sum_mode)


def byte_mask(nibble):
    """bit b of nibble -> byte b of a 32-bit mask"""
    return np.uint32(sum(0xff << (8 * b) for b in range(4) if (nibble >> b) & 1))


DIGIT_MASKS = [0xff, 0x01, 0x10, 0x80, 0x42, 0x15, 0x0f, 0xf8, 0x7f]    # 8, 1, 1, 1, 2, 3, 4, 5 and 7 radix passes
DIGIT_IMAGE = np.uint32(0xbfc4a1b2)      # the image of 1.5361845: finite, no byte 0x00 or 0xff
DIGIT_KEY = np.uint32(0x9c3a5e71)


@functools.lru_cache(maxsize=None)
@ieee
def digit_case(shape, mask, n=6000, seed=11):
    """one partition of n random codes, one query, radius +inf: all n rows are kept and their words differ exactly in the bytes `mask`
    names (bits 0-3: key bytes, bits 4-7: bytes of the candidate's image).  Only sub-quantizer 0's table row is non-zero, the rest
    is +0, so the candidate is table[0][code 0] bit for bit in either grouping; row 0 holds the values whose image is DIGIT_IMAGE
    with random bytes where the mask says (a NaN or an infinity among them: DIGIT_IMAGE itself); the labels are DIGIT_KEY likewise."""
    nsq, bits = shape
    rng = np.random.default_rng(seed + 1000 * mask + 100 * nsq + bits + n)
    codes = fc.rand_codes(rng, shape, n)
    images = DIGIT_IMAGE ^ (rng.integers(0, 1 << 32, 1 << bits, dtype=np.uint64).astype(np.uint32) & byte_mask(mask >> 4))
    row = image_value(images)
    row[~np.isfinite(row)] = image_value([DIGIT_IMAGE])[0]
    table = np.zeros((nsq, 1 << bits), np.float32)
    table[0] = row
    labels = DIGIT_KEY ^ (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & byte_mask(mask & 15))
    case = dict(shape=shape, parts=[codes], labels=[labels], assign=np.zeros((1, 1), np.int32), tables=table.reshape(1, 1, -1),
                radius=np.array([INF], np.float32))
    first = gather(shape, codes, table)[:, 0]
    for sum_mode in (1, 0):
        lims, keys, vals = expected_of(case, sum_mode)
        assert lims[-1] == n, "radius +inf keeps %d of %d rows" % (lims[-1], n)
        assert np.array_equal(np.sort(vals.view(np.uint32)), np.sort(first.view(np.uint32))), "the candidate is not table[0][code 0]"
        got = active_digits(words(keys, vals))
        assert got == mask, "the words differ in the digits %#04x, not %#04x" % (got, mask)
    if mask & 0x80:
        assert (vals < 0).any() and (vals > 0).any(), "a segment that varies in the sign byte holds both signs"
    return case


SIGNED_SIZES = [5000, 2500]              # with the 44 crafted rows: a segment above RANGE_SORT_LDS and one below
SIGNED_TWIN = 77                         # the label the all -0 row and the all +0 row share


@functools.lru_cache(maxsize=None)
@ieee
def signed_case(shape, seed=12):
    """tables of rand_tables minus their mean, so the candidates straddle zero.  Partition 2 holds crafted rows, and its tables say in
    every sub-quantizer m: digit 0 -> -0, digit 1 -> +0, digit 2 -> 3 (m + 1) 2^-149, digit 3 -> -5 (m + 1) 2^-149 (sums of those are exact
    in any grouping and subnormal).  Its rows: all-0 and all-1 digits under SIGNED_TWIN and two more labels, all-2, all-3, 2/3 and 0/1
    alternating, 32 random ones.  Query 0 keeps more than RANGE_SORT_LDS rows of partitions 0 and 2 (radix passes), query 1 fewer of
    1 and 2 (LDS), query 2 every row of 2 and 0 (radius +inf)."""
    nsq, bits = shape
    rng = np.random.default_rng(seed + 100 * nsq + bits)
    m = np.arange(nsq)
    crafted = [np.full(nsq, d) for d in (0, 1, 0, 1, 0, 1, 2, 3)] + [np.where(m & 1, 3, 2), np.where(m & 1, 2, 3), np.where(m & 1, 1, 0),
                                                                     np.where(m & 1, 0, 1)]
    p2 = np.concatenate([codes_of_digits(shape, np.array(crafted)), fc.rand_codes(rng, shape, 32)])
    l2 = np.concatenate([[SIGNED_TWIN, SIGNED_TWIN, 5, 5, 200, 200, 9, 10, 11, 12, 13, 14], rng.integers(0, 300, 32)]).astype(np.uint32)
    parts = [fc.rand_codes(rng, shape, s) for s in SIGNED_SIZES] + [p2]
    perm = rng.permutation(4 * sum(SIGNED_SIZES))[:sum(SIGNED_SIZES)].astype(np.uint32)
    labels = [perm[:SIGNED_SIZES[0]], perm[SIGNED_SIZES[0]:], l2]
    assign = np.array([[0, 2], [1, 2], [2, 0]], np.int32)
    tables = (fc.rand_tables(rng, shape, 3, 2) - np.float32(16.0 / 3.0)).astype(np.float32).reshape(3, 2, nsq, 1 << bits)
    for q, slot in ((0, 1), (1, 1), (2, 0)):
        tables[q, slot, :, 0] = np.float32(-0.0)
        tables[q, slot, :, 1] = np.float32(0.0)
        tables[q, slot, :, 2] = (3 * (m + 1)).astype(np.float32) * TINY
        tables[q, slot, :, 3] = (-5 * (m + 1)).astype(np.float32) * TINY
    tables = tables.reshape(3, 2, -1)
    radius = []
    for q, rows in enumerate((4600, 2200)):
        v = np.sort(np.concatenate([candidates(shape, parts[p], tables[q, a]) for a, p in enumerate(assign[q])]))
        radius.append(v[rows])
    case = dict(shape=shape, parts=parts, labels=labels, assign=assign, tables=tables, radius=np.array(radius + [INF], np.float32))
    assert radius[0] > FLT_MIN and radius[1] > FLT_MIN, "both radii lie above the zeros and the subnormals"
    for sum_mode in (1, 0):
        lims, keys, vals = expected_of(case, sum_mode)
        rows = np.diff(lims)
        assert rows[0] > RANGE_SORT_LDS > rows[1] > 1000 and rows[2] == SIGNED_SIZES[0] + len(p2), "segment lengths %s" % rows
        for q in range(3):
            k, v = keys[lims[q]:lims[q + 1]], vals[lims[q]:lims[q + 1]]
            assert (v < 0).sum() > 500 and (v > 0).sum() > 500, "query %d does not straddle zero" % q
            assert ((v != 0) & (np.abs(v) < FLT_MIN) & (v > 0)).any() and ((v != 0) & (np.abs(v) < FLT_MIN) & (v < 0)).any(), "no subnormals"
            zeros = np.flatnonzero((v == 0) & (k == SIGNED_TWIN))
            assert len(zeros) == 2, "the twin rows are both zero"
            if sum_mode == 1:            # (source order starts from +0, and +0 + -0 is +0: there the two rows are the same pair)
                assert np.signbit(v[zeros[0]]) and not np.signbit(v[zeros[1]]), "under one label the -0 row comes first"
    return case


NONFINITE_RADII = np.array([np.inf, FLT_MAX, np.nextafter(FLT_MAX, np.float32(0)), np.nan, -np.inf, 0.0, -0.0, TINY], np.float32)


@functools.lru_cache(maxsize=None)
@ieee
def nonfinite_case(shape, seed=13):
    """the tables of test_adc_range_host's test_tables_with_nan_inf_and_signed_zeros_and_tied_rows on any shape (quarter tables, few keys;
    partition 0 sums signed zeros; partition 3 has NaN in sub-quantizer 0, +inf in 1, -inf in 2 mod nsq), and partition 2 with three rows
    of one label whose digits are all 7, all 8, all 9: its table says, in the first and the last sub-quantizer, 7 -> FLT_MAX / 2, 8 ->
    FLT_MAX, 9 -> -FLT_MAX / 2 and +0 in between, so the rows sum to exactly FLT_MAX, to +inf by overflow and to exactly -FLT_MAX in
    either grouping.  One query probing all four partitions; case["radii"]: the radii to run it under."""
    nsq, bits = shape
    rng = np.random.default_rng(seed + 100 * nsq + bits)
    sizes = [700, 0, 3, 1300]
    parts = [fc.rand_codes(rng, shape, s) for s in sizes]
    parts[0][:350] = 0
    parts[2] = codes_of_digits(shape, np.array([np.full(nsq, d) for d in (7, 8, 9)]))
    labels = [rng.integers(0, 40, s).astype(np.uint32) for s in sizes]
    labels[2][:] = 3
    tables = quarter_tables(rng, shape, 1, 4)[0].reshape(4, nsq, 1 << bits).copy()
    tables[0, :, :] = np.float32(0.0)
    tables[0, :, 0] = np.float32(-0.0)
    tables[2, :, 7:10] = np.float32(0.0)
    for sq in (0, nsq - 1):
        tables[2, sq, 7:10] = [FLT_MAX / np.float32(2), FLT_MAX, -FLT_MAX / np.float32(2)]
    tables[3, 0, ::5] = np.nan
    tables[3, 1, 1::5] = np.inf
    tables[3, 2 % nsq, 2::7] = -np.inf
    case = dict(shape=shape, parts=parts, labels=labels, assign=np.arange(4, dtype=np.int32).reshape(1, 4), tables=tables.reshape(1, 4, -1),
                radii=NONFINITE_RADII)
    assert NONFINITE_RADII[-1].view(np.uint32) == 1 and NONFINITE_RADII[2].view(np.uint32) == FLT_MAX.view(np.uint32) - 1
    for sum_mode in (1, 0):
        v = np.concatenate([candidates(shape, p, tables.reshape(4, -1)[a], sum_mode) for a, p in enumerate(parts)])
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any(), "a NaN, a +inf and a -inf candidate"
        assert list(v[700:703].view(np.uint32)) == list(np.array([FLT_MAX, INF, -FLT_MAX], np.float32).view(np.uint32)), "partition 2's sums"
        assert (v == FLT_MAX).sum() == 1
        zeros = v[v == 0]
        assert np.signbit(zeros).any() == (sum_mode == 1) and not np.signbit(zeros).all(), "the zeros among the candidates"
        for r in NONFINITE_RADII:
            _, _, vals = expected_of(dict(case, radius=[r]), sum_mode)
            kept_all_neg_inf = int(np.isneginf(vals).sum()) == int(np.isneginf(v).sum())
            assert not np.isnan(vals).any() and not np.isposinf(vals).any()
            if np.isnan(r) or np.isneginf(r):
                assert len(vals) == 0, "radius %r keeps nothing" % r
            else:
                assert kept_all_neg_inf and np.isneginf(vals).any(), "radius %r keeps every -inf row" % r
                assert (vals == -FLT_MAX).sum() == 1
            assert (vals == FLT_MAX).sum() == (1 if np.isposinf(r) else 0), "the FLT_MAX row is kept under +inf only"
    return case


def nonfinite_batch(case, radii):
    """the one-query case under several radii at once: the query repeated"""
    n = len(radii)
    return dict(case, assign=np.repeat(case["assign"], n, 0), tables=np.repeat(case["tables"], n, 0), radius=np.asarray(radii, np.float32))
