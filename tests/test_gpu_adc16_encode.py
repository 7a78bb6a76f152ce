"""The GPU encoder for 16-bit sub-quantizers (qadc_adc_encode16_host, pyqadc.adc_encode16): codes, and assign where there is a
coarse quantizer, compared for equality with tests/adc16_encode_compose.py — the reference's own capacity-1 heap on the
oracle's expansion distances.  No tolerance anywhere: device and oracle evaluate the same float sums in the same order.

The kernel (csrc/qadc_adc_kernels.h): a workgroup encodes V = 256 * encode16_lane_vectors vectors of one sub-quantizer and
stages kEnc16Tile = 256 centroid rows at a time; a small call cuts the 65536 centroids into up to 64 runs of kEnc16MinSlice =
1024 or a power-of-two multiple of it.  The shapes below sit on those edges."""
import ctypes as C

import numpy as np
import pytest

import adc16_compose as a16
import adc16_encode_compose as e16
import adc_compose as ac
import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

CHUNK = pyqadc.QADC_ADC_ENCODE16_CHUNK
MIN_SLICE = 1024                                                  # kEnc16MinSlice
# (nsq, dim): sq_dim 8, 16, 32 = the register paths, 2 and 5 = the any-size path
SHAPES = [(2, 16), (4, 64), (2, 64), (8, 16), (4, 20)]
WIDE = (2, 128)                                                   # sq_dim 64: the register path of 2x16 at 128 dimensions


def wg_vectors(nsq, dim):
    """V: vectors per workgroup (256 lanes x encode16_lane_vectors of the path)"""
    return {8: 1024, 16: 1024, 32: 512, 64: 512}.get(dim // nsq, 256)


def shape_id(s):
    return "%dx16-d%d" % s


class Data:
    """One shape's quantizers and vectors, and the oracle's answers: each computed once, on the longest prefix any test asks
    for (every vector is encoded on its own, so a shorter call must return a prefix)"""

    def __init__(self, nsq, dim):
        rng = np.random.default_rng(1600 + 10 * nsq + dim)
        self.nsq, self.dim, self.V = nsq, dim, wg_vectors(nsq, dim)
        self.codebooks = rng.standard_normal((nsq, 65536, dim // nsq), dtype=np.float32)
        self.coarse = (rng.normal(size=(8, dim)) * 2).astype(np.float32)
        self.rotation = ac.random_rotation(rng, dim)
        self.vectors = rng.normal(size=(max(self.V + 1, 1000), dim)).astype(np.float32)
        self.vectors += self.coarse[rng.integers(0, 8, len(self.vectors))]
        for a in (self.codebooks, self.coarse, self.rotation, self.vectors):
            a.setflags(write=False)
        self.wanted = {}

    def quantizers(self, ivf, opq):
        return dict(coarse=self.coarse if ivf else None, rotation=self.rotation if opq else None)

    def want(self, po, n, ivf, opq, sum_mode):
        key = (ivf, opq, sum_mode)
        if key not in self.wanted:
            longest = self.V + 1 if ivf or opq else len(self.vectors)
            self.wanted[key] = e16.encode16(po, self.codebooks, self.vectors[:longest], sum_mode=sum_mode, **self.quantizers(ivf, opq))
        a, c = self.wanted[key]
        return (None if a is None else a[:n]), c[:n]


_data = {}


def data(shape):
    if shape not in _data:
        _data[shape] = Data(*shape)
    return _data[shape]


def assert_encoding(got, want, what=""):
    (ga, gc), (wa, wc) = got, want
    assert gc.dtype == np.uint16 and gc.shape == wc.shape, what
    bad = np.argwhere(gc != wc)
    assert len(bad) == 0, "%s: %d of %d codes differ, first at %s: got %d, expected %d" % (
        what, len(bad), gc.size, bad[0], gc[tuple(bad[0])], wc[tuple(bad[0])])
    if wa is None:
        assert ga is None, what
    else:
        assert ga.dtype == np.int32 and np.array_equal(ga, wa), "%s: assign differs" % what


# ---- 1. random vectors ------------------------------------------------------------------------------------------------------

RANDOM = [(s, n, ivf, opq, sm) for s in SHAPES for sm in (1, 0) for ivf, opq in ((0, 0), (1, 0), (0, 1), (1, 1))
          for n in ("1", "V+1", "1000") if not (n == "1000" and (ivf or opq))]


@path_independent
@pytest.mark.parametrize("shape,n,ivf,opq,sum_mode", RANDOM,
                         ids=["%s-n%s-%s-%s-sum%d" % (shape_id(s), n, "ivf" if i else "flat", "opq" if o else "pq", sm) for s, n, i, o, sm in RANDOM])
def test_random_vectors(po, shape, n, ivf, opq, sum_mode):
    d = data(shape)
    n = {"1": 1, "V+1": d.V + 1, "1000": 1000}[n]
    want = d.want(po, n, ivf, opq, sum_mode)
    got = pyqadc.adc_encode16(d.codebooks, d.vectors[:n], sum_mode=sum_mode, **d.quantizers(ivf, opq))
    assert_encoding(got, want)
    assert (got[1] >= 256).any(), "no code uses its high byte"


@path_independent
@pytest.mark.parametrize("n,ivf,opq,sum_mode", [("1", 0, 0, 1), ("V+1", 0, 0, 1), ("V+1", 0, 0, 0), ("V+1", 1, 1, 1)],
                         ids=["n1", "nV+1", "nV+1-sum0", "nV+1-ivf-opq"])
def test_random_vectors_sub_vectors_of_64(po, n, ivf, opq, sum_mode):
    test_random_vectors(po, WIDE, n, ivf, opq, sum_mode)


@path_independent
def test_codes_are_little_endian_bytes(po):
    """the raw call: 2 * sq_count bytes per vector, low byte first — the rows add_partitions takes on a create16 index"""
    d = data((2, 16))
    n = 1000
    raw = np.zeros((n, 2 * d.nsq), np.uint8)
    f32p = C.POINTER(C.c_float)
    v = np.ascontiguousarray(d.vectors[:n])
    rc = pyqadc.lib().qadc_adc_encode16_host(d.nsq, d.dim, d.codebooks.ctypes.data_as(f32p), None, 0, None, v.ctypes.data_as(f32p), n, 1,
                                             None, raw.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
    assert rc == 0
    want = d.want(po, n, 0, 0, 1)[1]
    assert np.array_equal(raw[:, 0::2], (want & 0xff).astype(np.uint8)) and np.array_equal(raw[:, 1::2], (want >> 8).astype(np.uint8))
    assert (raw[:, 1::2] != 0).any()


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(2, 16), (8, 16)], ids=shape_id)
def test_the_first_of_equal_centroids_wins(po, shape):
    """codebooks and vectors from {-1, 0, 1}: at most 3^ds distinct rows among 65536, so every pick is a tie over lanes, waves,
    tiles and centroid runs (n = 3: 64 runs; n = V + 1: 64 runs at 2x16, 16 at 8x16)"""
    nsq, dim = shape
    rng = np.random.default_rng(1700 + nsq)
    cb = rng.integers(-1, 2, (nsq, 65536, dim // nsq)).astype(np.float32)
    v = rng.integers(-1, 2, (wg_vectors(nsq, dim) + 1, dim)).astype(np.float32)
    want = e16.encode16(po, cb, v)
    for n in (3, len(v)):
        assert_encoding(pyqadc.adc_encode16(cb, v[:n]), (None, want[1][:n]), "n %d" % n)
    cb[:, 32768:] = cb[:, :32768]
    _, codes = pyqadc.adc_encode16(cb, v)
    assert (codes < 32768).all(), "a centroid of the duplicated half won"
    assert_encoding((None, codes), e16.encode16(po, cb, v), "duplicated halves")


# ---- 3. NaN -----------------------------------------------------------------------------------------------------------------

NAN_ROWS = [[0], [63], [64], [255], [256], [32767, 32768], [65534], [65535], [300, 40000], list(range(65536))]
# both sides of every place the kernel may cut the centroids of a sub-quantizer
NAN_ROWS += [[k * MIN_SLICE - 1] for k in range(1, 65536 // MIN_SLICE)] + [[k * MIN_SLICE] for k in range(1, 65536 // MIN_SLICE)]


@path_independent
@pytest.mark.parametrize("shape", [(8, 16), (4, 32)], ids=shape_id)
def test_nan_codebook_rows(po, shape):
    """Every launch carries one clean sub-quantizer (the last) and a NaN pattern in each of the others"""
    nsq, dim = shape
    ds = dim // nsq
    rng = np.random.default_rng(1800 + nsq)
    clean = rng.standard_normal((nsq, 65536, ds), dtype=np.float32)
    v = rng.normal(size=(8, dim)).astype(np.float32)
    for first in range(0, len(NAN_ROWS), nsq - 1):
        patterns = NAN_ROWS[first:first + nsq - 1]
        cb = clean.copy()
        for m, rows in enumerate(patterns):
            cb[m, rows, rng.integers(0, ds)] = np.nan
        want = e16.encode16(po, cb, v)
        got = pyqadc.adc_encode16(cb, v)
        assert_encoding(got, want, "NaN rows %s" % [p if len(p) < 4 else "all" for p in patterns])
        for m, rows in enumerate(patterns):
            if rows[-1] >= 65534:
                assert (got[1][:, m] == 65535).all(), rows[-1]


@path_independent
@pytest.mark.parametrize("shape", [(2, 16), (8, 16)], ids=shape_id)
def test_nan_and_infinite_vectors(po, shape):
    nsq, dim = shape
    d = data(shape)
    v = d.vectors[:7].copy()
    v[0, 3] = np.nan
    v[1, dim - 1] = np.inf
    v[2, :] = -np.inf
    v[3, 0] = np.inf
    v[3, dim // nsq] = -np.inf
    v[4, :] = np.nan
    assert_encoding(pyqadc.adc_encode16(d.codebooks, v), e16.encode16(po, d.codebooks, v))
    assert_encoding(pyqadc.adc_encode16(d.codebooks, v, coarse=d.coarse), e16.encode16(po, d.codebooks, v, coarse=d.coarse), "ivf")


# ---- 4. a code is the first argmin of the table the engine builds for that vector ------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(2, 16), (4, 64)], ids=shape_id)
def test_codes_are_the_argmin_of_the_engines_own_tables(shape):
    nsq, dim = shape
    d = data(shape)
    idx = pyqadc.AdcIndex.create16(nsq)
    try:
        idx.add_partitions([np.zeros((1, nsq), np.uint16)])
        idx.set_pq(d.codebooks)
        _, tables = idx.search_tables(d.vectors[:5], 1, table_form=1)
        first_min = np.argmin(tables.reshape(5, nsq, 65536), axis=2)
        _, codes = pyqadc.adc_encode16(d.codebooks, d.vectors[:5])
        assert np.array_equal(codes, first_min.astype(np.uint16))
    finally:
        idx.close()


# ---- 5. the pass size shows in no result ------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("ivf", [0, 1], ids=["flat", "ivf"])
def test_chunk_independence(po, ivf):
    d = data((2, 16))
    rng = np.random.default_rng(1900 + ivf)
    n = CHUNK + 3
    v = rng.standard_normal((n, d.dim), dtype=np.float32)
    coarse = d.coarse if ivf else None
    got = pyqadc.adc_encode16(d.codebooks, v, coarse=coarse)
    rows = np.unique(np.concatenate([[0, CHUNK - 1, CHUNK, CHUNK + 2], rng.choice(n, 296, replace=False)]))
    want = e16.encode16(po, d.codebooks, v[rows], coarse=coarse)
    assert_encoding((None if got[0] is None else got[0][rows], got[1][rows]), want, "sampled rows")
    alone = pyqadc.adc_encode16(d.codebooks, v[:1000], coarse=coarse)
    assert_encoding((None if got[0] is None else got[0][:1000], got[1][:1000]), alone, "the first 1000 rows, encoded alone")


# ---- 6. end to end: encode, index, search -----------------------------------------------------------------------------------

@path_independent
def test_search_over_a_database_encoded_on_the_gpu(po):
    rng = np.random.default_rng(2000)
    n, nq, nsq, dim, K, ma, R = 70000, 5, 2, 16, 8, 3, 100
    centers = (rng.normal(size=(200, dim)) * 3).astype(np.float32)
    vectors = (centers[rng.integers(0, 200, n)] + rng.normal(size=(n, dim))).astype(np.float32)
    queries = (centers[rng.integers(0, 200, nq)] + rng.normal(size=(nq, dim))).astype(np.float32)
    coarse, _ = pyqadc.kmeans_iterations(vectors[:20000], vectors[rng.choice(n, K, replace=False)], 5)
    sample = vectors[rng.choice(n, 65536, replace=False)]
    sa = ac.assign(po, sample, coarse, 1)[:, 0]
    codebooks = np.ascontiguousarray((sample - coarse[sa]).reshape(65536, nsq, dim // nsq).transpose(1, 0, 2), np.float32)
    a, codes = pyqadc.adc_encode16(codebooks, vectors, coarse)
    check = rng.choice(n, 300, replace=False)
    assert_encoding((a[check], codes[check]), e16.encode16(po, codebooks, vectors[check], coarse), "sampled rows")
    order = np.argsort(a, kind="stable")
    bounds = np.searchsorted(a[order], np.arange(K + 1))
    parts = [codes[order[bounds[k]:bounds[k + 1]]] for k in range(K)]
    labels = [order[bounds[k]:bounds[k + 1]].astype(np.uint32) for k in range(K)]
    idx = pyqadc.AdcIndex.create16(nsq)
    try:
        idx.add_partitions(parts, labels)
        idx.set_pq(codebooks)
        idx.set_coarse(coarse)
        keys, vals, sizes, got_a = idx.search(queries, ma, R, table_form=1)
    finally:
        idx.close()
    want_a = ac.assign(po, queries, coarse, ma)
    assert np.array_equal(got_a, want_a)
    res = ac.residuals(queries, coarse, want_a).reshape(nq * ma, dim)
    tables = np.zeros((nq * ma, nsq, 65536), np.float32)
    for m in range(nsq):
        tables[:, m, :] = po.cross_dists(codebooks[m], res[:, m * (dim // nsq):(m + 1) * (dim // nsq)], 1)
    tables = tables.reshape(nq, ma, nsq * 65536)
    hits = 0
    for q in range(nq):
        want = a16.heap(po, nsq, [parts[k] for k in want_a[q]], [labels[k] for k in want_a[q]], tables[q], R)
        a16.assert_heap((keys, vals, sizes), want, q, "encoded database")
        exact = np.argsort(((vectors - queries[q]) ** 2).sum(axis=1))[:R]
        hits += len(np.intersect1d(exact, keys[q, :sizes[q]]))
    print("recall@%d against exact float L2 over %d queries: %.3f" % (R, nq, hits / float(nq * R)))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

@path_independent
def test_a_refused_call_is_followed_by_a_good_one(po):
    d = data((2, 16))
    with pytest.raises(pyqadc.QadcError, match="2, 4 or 8"):
        pyqadc.adc_encode16(np.zeros((16, 65536, 1), np.float32), d.vectors[:4])
    with pytest.raises(pyqadc.QadcError, match="2, 4 or 8"):
        pyqadc.adc_encode16(d.codebooks, d.vectors[:4], sum_mode=2)
    assert_encoding(pyqadc.adc_encode16(d.codebooks, d.vectors[:4]), d.want(po, 4, 0, 0, 1))
