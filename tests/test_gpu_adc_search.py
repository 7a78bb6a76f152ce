"""The float-ADC engine fed with query vectors (pyqadc.AdcIndex.search / search_tables, pyqadc.adc_encode): coarse assignment,
residual, OPQ rotation, the distance tables of every (query, probe) and the 8-bit encoder run on the GPU.  Everything is compared
bit for bit with the composition of the oracle's functions in tests/adc_compose.py, and the heaps with the reference's own
scanner_simple (oracle/_ref) where that build exists."""
import zlib

import numpy as np
import pytest

import adc_compose as ac
import pyqadc
from helpers import path_independent
from test_gpu_adc import assert_heap, expected, ivf_db

pytestmark = pytest.mark.gpu

DIM = 128          # sq_dim 32, 16, 8 for 4x8, 8x8, 16x8: the table kernel's register paths
K = 64


def seed_of(*parts):
    return zlib.crc32(" ".join(str(p) for p in parts).encode())


class Case:
    """One database (flat: one partition; IVF: K = 64 partitions of skewed sizes, six of them empty, labelled), its quantizers and
    its GPU index."""

    def __init__(self, rng, nsq, dim=DIM, ivf=True, opq=False, n=30000):
        self.nsq, self.dim = nsq, dim
        self.codebooks = rng.normal(size=(nsq, 256, dim // nsq)).astype(np.float32)
        self.rotation = ac.random_rotation(rng, dim) if opq else None
        if ivf:
            self.coarse = (rng.normal(size=(K, dim)) * 2).astype(np.float32)
            self.parts, self.labels = ivf_db(rng, nsq, K, n)
        else:
            self.coarse = None
            self.parts, self.labels = [rng.integers(0, 256, (n // 4, nsq), dtype=np.uint8)], None
        self.idx = pyqadc.AdcIndex(nsq, 8)
        self.idx.add_partitions(self.parts, self.labels)
        self.idx.set_pq(self.codebooks)
        self.idx.set_rotation(self.rotation)
        self.idx.set_coarse(self.coarse)

    def queries(self, rng, nq):
        q = rng.normal(size=(nq, self.dim)).astype(np.float32)
        if self.coarse is not None:
            q += self.coarse[rng.integers(0, K, nq)]
        return q

    def compose(self, po, queries, ma, table_form, sum_mode=1):
        a = ac.assign(po, queries, self.coarse, ma, sum_mode)
        res = ac.residuals(queries, self.coarse, a, self.rotation)
        return a, ac.tables(po, self.codebooks, res, table_form, sum_mode), res

    def heaps(self, po, a, tables, q, R, sum_mode=1):
        labels = None if self.labels is None else [self.labels[k] for k in a[q]]
        return expected(po, self.nsq, [self.parts[k] for k in a[q]], labels, tables[q], R, sum_mode)

    def close(self):
        self.idx.close()


def check_tables(po, case, queries, ma, table_form, sum_mode=1, what=""):
    want_a, want_t, res = case.compose(po, queries, ma, table_form, sum_mode)
    got_a, got_t = case.idx.search_tables(queries, ma, table_form, sum_mode)
    assert np.array_equal(got_a, want_a), "%s: assign differs" % what
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)), \
        "%s: %d table entries differ" % (what, int((got_t.view(np.uint32) != want_t.view(np.uint32)).sum()))
    return res


# ---- 3. search_tables: assign and tables equal the composition -------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
def test_tables_equal_the_composition(po, nsq, ivf, opq):
    rng = np.random.default_rng(seed_of("tables", nsq, ivf, opq))
    case = Case(rng, nsq, ivf=ivf, opq=opq)
    queries = case.queries(rng, 3)
    pinned = False
    for table_form in (0, 1, 2):
        for ma in (1, 8, 24, K):
            res = check_tables(po, case, queries, ma, table_form, what="form %d ma %d" % (table_form, ma))
            if not pinned:
                ac.pin_to_reference(po, case.codebooks, res.reshape(-1, DIM)[:4])
                pinned = True
    case.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
def test_tables_in_source_order_sums(po, nsq, ivf, opq):
    rng = np.random.default_rng(seed_of("sum0", nsq, ivf, opq))
    case = Case(rng, nsq, ivf=ivf, opq=opq)
    queries = case.queries(rng, 3)
    for table_form in (0, 1, 2):
        for ma in (1, 8):
            check_tables(po, case, queries, ma, table_form, sum_mode=0, what="sum_mode 0 form %d ma %d" % (table_form, ma))
    case.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("sq_dim", [12, 5, 30])     # as compiled with a remainder of 4 and of 6, and one sequential sum
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
def test_tables_for_any_sub_vector_size(po, nsq, sq_dim, opq):
    rng = np.random.default_rng(seed_of("general", nsq, sq_dim, opq))
    case = Case(rng, nsq, dim=nsq * sq_dim, ivf=True, opq=opq)
    queries = case.queries(rng, 3)
    for table_form in (0, 1):
        for sum_mode in (1, 0):
            for ma in (1, 24):
                check_tables(po, case, queries, ma, table_form, sum_mode, "sq_dim %d form %d sum_mode %d ma %d" % (sq_dim, table_form, sum_mode, ma))
    case.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("nq", [1, 257])
def test_tables_of_one_query_and_of_a_batch(po, nsq, nq):
    rng = np.random.default_rng(seed_of("nq", nsq, nq))
    case = Case(rng, nsq, ivf=True, opq=nsq == 8)
    queries = case.queries(rng, nq)
    for table_form, ma in ((0, 1), (1, 24), (0, 24), (2, 8)):
        check_tables(po, case, queries, ma, table_form, what="nq %d form %d ma %d" % (nq, table_form, ma))
    case.close()


# ---- 4. search: the reference's heaps on those tables, and the caller-tables path of the same index ------------------------

@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
def test_search_heaps_equal_the_reference_scan(po, nsq, ivf, opq):
    rng = np.random.default_rng(seed_of("search", nsq, ivf, opq))
    case = Case(rng, nsq, ivf=ivf, opq=opq)
    nq = 5
    queries = case.queries(rng, nq)
    for table_form, ma, sum_mode in ((2, 1, 1), (2, 8, 1), (0, 24, 1), (1, 24, 1), (1, 8, 0)):
        want_a, want_t, _ = case.compose(po, queries, ma, table_form, sum_mode)
        got_a, got_t = case.idx.search_tables(queries, ma, table_form, sum_mode)
        for R in (1, 100, 1000):
            keys, vals, sizes, a = case.idx.search(queries, ma, R, table_form, sum_mode)
            assert np.array_equal(a, want_a)
            for q in range(nq):
                assert_heap((keys, vals, sizes), case.heaps(po, want_a, want_t, q, R, sum_mode), q,
                            "form %d ma %d R %d sum_mode %d" % (table_form, ma, R, sum_mode))
            old = case.idx.query_scan(got_a, got_t, R, sum_mode)        # the old path, fed with the fetched tables
            for got, ref in zip((keys, vals.view(np.uint32), sizes), (old[0], old[1].view(np.uint32), old[2])):
                assert np.array_equal(got, ref), "search and query_scan(assign, tables) differ"
    # the ordered stream replays to the same arrays
    ma, R = 8, 64
    keys, vals, sizes, a = case.idx.search(queries, ma, R)
    ck, cv, off, ca = case.idx.search_candidates(queries, ma, R)
    assert np.array_equal(a, ca) and off[0] == 0 and off[-1] == len(ck)
    sk = np.zeros(R, np.uint32)
    sv = (np.float32(np.finfo(np.float32).max) - np.arange(R, dtype=np.float32)).astype(np.float32)
    for q in range(nq):
        lo, hi = int(off[q]), int(off[q + 1])
        want = po.heap_replay_f32(np.concatenate([sk, ck[lo:hi]]), np.concatenate([sv, cv[lo:hi]]), R)
        assert_heap((keys, vals, sizes), want, q, "stream replay")
    case.close()


# ---- 5. sub-batches and the re-run of an overflowing region ----------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
def test_results_do_not_depend_on_the_table_budget(po, nsq):
    rng = np.random.default_rng(seed_of("budget", nsq))
    case = Case(rng, nsq, ivf=True, opq=nsq == 4)
    nq, ma, R = 10, 8, 100
    queries = case.queries(rng, nq)
    whole = case.idx.search(queries, ma, R)
    whole_t = case.idx.search_tables(queries, ma)
    whole_c = case.idx.search_candidates(queries, ma, R)
    want_a, want_t, _ = case.compose(po, queries, ma, 2)
    for q in range(nq):
        assert_heap(whole[:3], case.heaps(po, want_a, want_t, q, R), q, "unbudgeted")
    per_query = ma * nsq * 256 * 4
    for per in (1, 3):
        case.idx.set_table_budget(per * per_query)
        for got, ref in ((case.idx.search(queries, ma, R), whole), (case.idx.search_tables(queries, ma), whole_t),
                         (case.idx.search_candidates(queries, ma, R), whole_c)):
            for g, r in zip(got, ref):
                assert g.dtype == r.dtype and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                                             r.view(np.uint32) if r.dtype == np.float32 else r), \
                    "%d queries per sub-batch" % per
    case.idx.set_table_budget(0)
    assert all(np.array_equal(g, r) for g, r in zip(case.idx.search(queries, ma, R)[:1], whole[:1]))
    case.close()


def descending_case(rng, n):
    """A flat 4x8 database over 4-d vectors (sq_dim 1) whose candidates strictly decrease in scan order for the query 0: code i
    stands for v = n - i through c0 = v >> 8, c1 = v & 255, with codebook entries sqrt(512 c) and sqrt(c), so that the direct
    table entries are about 512 c0 and c1 and every candidate is below the one before it; c2 and c3 look up zeros."""
    v = np.arange(n, 0, -1, dtype=np.int64)
    assert n < 256 * 256
    codes = np.stack([v >> 8, v & 255, rng.integers(0, 256, n), rng.integers(0, 256, n)], axis=1).astype(np.uint8)
    c = np.arange(256, dtype=np.float64)
    codebooks = np.zeros((4, 256, 1), np.float32)
    codebooks[0, :, 0] = np.sqrt(512 * c)
    codebooks[1, :, 0] = np.sqrt(c)
    return codes, codebooks


@path_independent
@pytest.mark.parametrize("n", [20000, 60000])
def test_search_reruns_an_overflowing_region(po, n):
    rng = np.random.default_rng(n)
    codes, codebooks = descending_case(rng, n)
    idx = pyqadc.AdcIndex(4, 8)
    idx.add_partitions([codes])
    idx.set_pq(codebooks)
    queries = rng.normal(size=(5, 4)).astype(np.float32)
    queries[2] = 0                                              # the descending one
    a, tables = idx.search_tables(queries, 1, 0)
    want_t = ac.tables(po, codebooks, ac.residuals(queries, None, a), 0)
    assert np.array_equal(tables.view(np.uint32), want_t.view(np.uint32))
    for R in (1, 100):
        runs = idx.reruns()
        got = idx.search(queries, 1, R, 0)
        for q in range(5):
            assert_heap(got[:3], expected(po, 4, [codes], None, tables[q], R), q, "descending n=%d R=%d" % (n, R))
        assert idx.reruns() > runs, "the candidate region did not overflow: the re-run path was not taken"
        ck, cv, off, _ = idx.search_candidates(queries[2:3], 1, R, 0)
        assert int(off[1]) == n and (np.diff(cv) < 0).all()     # every code is a push of the reference
    idx.close()


# ---- 6. exact coarse ties, NaN and infinities ------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
def test_exact_coarse_ties(po, nsq):
    rng = np.random.default_rng(seed_of("ties", nsq))
    case = Case(rng, nsq, ivf=True)
    case.coarse = rng.integers(-1, 2, (K, DIM)).astype(np.float32)          # grid-valued: many exactly equal distances
    case.coarse[10] = case.coarse[3]
    case.coarse[40] = case.coarse[3]
    case.idx.set_coarse(case.coarse)
    queries = rng.integers(-1, 2, (9, DIM)).astype(np.float32)
    d = po.cross_dists(case.coarse, queries, 1)
    assert any(len(np.unique(row)) < K for row in d)
    for ma in (1, 8, 24, K):
        want_a, want_t, _ = case.compose(po, queries, ma, 2)
        got_a, got_t = case.idx.search_tables(queries, ma)
        assert np.array_equal(got_a, want_a), "ma %d" % ma
        assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
        got = case.idx.search(queries, ma, 100)
        for q in range(len(queries)):
            assert_heap(got[:3], case.heaps(po, want_a, want_t, q, 100), q, "ties ma %d" % ma)
    case.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
def test_nan_and_infinities_in_queries_and_centroids(po, nsq, opq):
    rng = np.random.default_rng(seed_of("nonfinite", nsq, opq))
    case = Case(rng, nsq, ivf=True, opq=opq)
    case.coarse[5, 7] = np.nan
    case.coarse[20, 0] = np.inf
    case.coarse[33, 100] = -np.inf
    case.idx.set_coarse(case.coarse)
    queries = case.queries(rng, 8)
    queries[1, 3] = np.nan
    queries[2, 50] = np.inf
    queries[3, 51] = -np.inf
    queries[4, :] = np.nan
    for table_form, ma in ((0, 1), (1, 8), (0, 24), (1, K)):
        with np.errstate(all="ignore"):
            want_a, want_t, _ = case.compose(po, queries, ma, table_form)
        got_a, got_t = case.idx.search_tables(queries, ma, table_form)
        assert np.array_equal(got_a, want_a), "form %d ma %d" % (table_form, ma)
        ac.assert_same_floats(got_t, want_t, "form %d ma %d" % (table_form, ma))
        for R in (1, 100):
            got = case.idx.search(queries, ma, R, table_form)
            for q in range(len(queries)):
                assert_heap(got[:3], case.heaps(po, want_a, want_t, q, R), q, "non-finite form %d ma %d R %d" % (table_form, ma, R))
    case.close()


@path_independent
def test_a_nan_row_with_more_than_256_probes_is_refused(po):
    rng = np.random.default_rng(256)
    nsq, dim, k = 8, 32, 300
    idx = pyqadc.AdcIndex(nsq, 8)
    parts = [rng.integers(0, 256, (20, nsq), dtype=np.uint8) for _ in range(k)]
    idx.add_partitions(parts)
    codebooks = rng.normal(size=(nsq, 256, dim // nsq)).astype(np.float32)
    coarse = rng.normal(size=(k, dim)).astype(np.float32)
    idx.set_pq(codebooks)
    idx.set_coarse(coarse)
    queries = rng.normal(size=(4, dim)).astype(np.float32)
    clean = idx.search(queries, 257, 10)
    bad = queries.copy()
    bad[2, 1] = np.nan
    with pytest.raises(pyqadc.QadcError, match="NaN"):
        idx.search(bad, 257, 10)
    with pytest.raises(pyqadc.QadcError, match="NaN"):
        idx.search_tables(bad, 257)
    again = idx.search(queries, 257, 10)                        # the index stays usable
    assert all(np.array_equal(g, r) for g, r in zip(again, clean))
    got = idx.search(bad, 256, 10)                              # 256 probes: the reference's heap replay decides
    with np.errstate(all="ignore"):
        want_a = ac.assign(po, bad, coarse, 256)
    assert np.array_equal(got[3], want_a)
    idx.close()


# ---- 7. adc_encode ---------------------------------------------------------------------------------------------------------

def check_encode(po, codebooks, vectors, coarse=None, rotation=None, sum_mode=1, what=""):
    with np.errstate(all="ignore"):
        want_a, want_c = ac.encode(po, codebooks, vectors, coarse, rotation, sum_mode)
    got_a, got_c = pyqadc.adc_encode(codebooks, vectors, coarse, rotation, sum_mode=sum_mode)
    if coarse is None:
        assert got_a is None
    else:
        assert np.array_equal(got_a, want_a), "%s: assign differs" % what
    bad = np.argwhere(got_c != want_c)
    assert len(bad) == 0, "%s: %d codes differ, first (vector, sub-quantizer) %s" % (what, len(bad), bad[0])
    return got_c


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("n", [1, 255, 100003])
def test_encode_random_vectors(po, nsq, n):
    rng = np.random.default_rng(seed_of("encode", nsq, n))
    codebooks = rng.normal(size=(nsq, 256, DIM // nsq)).astype(np.float32)
    vectors = rng.normal(size=(n, DIM)).astype(np.float32)
    check_encode(po, codebooks, vectors, what="plain")
    check_encode(po, codebooks, vectors, sum_mode=0, what="sum_mode 0")
    if n <= 255:
        coarse = (rng.normal(size=(K, DIM)) * 2).astype(np.float32)
        rotation = ac.random_rotation(rng, DIM)
        check_encode(po, codebooks, vectors, coarse, None, what="ivf")
        check_encode(po, codebooks, vectors, None, rotation, what="opq")
        check_encode(po, codebooks, vectors, coarse, rotation, what="ivf + opq")


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
def test_encode_with_coarse_and_rotation_at_size(po, nsq):
    rng = np.random.default_rng(seed_of("encode ivf", nsq))
    dim = 64
    codebooks = rng.normal(size=(nsq, 256, dim // nsq)).astype(np.float32)
    coarse = (rng.normal(size=(K, dim)) * 2).astype(np.float32)
    rotation = ac.random_rotation(rng, dim)
    vectors = (rng.normal(size=(40001, dim)) + coarse[rng.integers(0, K, 40001)]).astype(np.float32)
    check_encode(po, codebooks, vectors, coarse, rotation, what="ivf + opq")


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("sq_dim", [8, 12, 5])
def test_encode_ties_duplicates_and_nan(po, nsq, sq_dim):
    rng = np.random.default_rng(seed_of("encode special", nsq, sq_dim))
    dim = nsq * sq_dim
    n = 3000
    # grid data: exact distance ties between different centroids
    grid_cb = rng.integers(-1, 2, (nsq, 256, sq_dim)).astype(np.float32)
    grid_v = rng.integers(-1, 2, (n, dim)).astype(np.float32)
    got = check_encode(po, grid_cb, grid_v, what="grid")
    d = po.cross_dists(grid_cb[0], grid_v[:50, :sq_dim], 1)
    assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).any(), "no exact tie in the grid case"
    # duplicate centroids: the first of them is picked
    dup_cb = rng.normal(size=(nsq, 256, sq_dim)).astype(np.float32)
    dup_cb[:, 128:] = dup_cb[:, :128]
    vectors = rng.normal(size=(n, dim)).astype(np.float32)
    got = check_encode(po, dup_cb, vectors, what="duplicates")
    assert got.max() < 128
    # NaN centroids: at 0, inside a wave, at a wave's last lane, at 255, and several
    for where in ([0], [37], [63], [127, 128], [255], [0, 64, 200], [191, 255], list(range(0, 256))):
        cb = rng.normal(size=(nsq, 256, sq_dim)).astype(np.float32)
        for m in range(nsq):
            if m % 2 == 0 or len(where) == 1:
                cb[m, where, rng.integers(0, sq_dim)] = np.nan
        got = check_encode(po, cb, vectors[:500], what="NaN centroids at %s" % where)
        if where == [255]:
            assert (got == 255).all()
    # NaN and infinities in the vectors
    bad = vectors[:64].copy()
    bad[1, 0] = np.nan
    bad[2, dim - 1] = np.inf
    bad[3, :] = -np.inf
    check_encode(po, dup_cb, bad, what="non-finite vectors")


# ---- 8. real encodings -----------------------------------------------------------------------------------------------------

@path_independent
def test_search_over_a_database_encoded_on_the_gpu(po):
    rng = np.random.default_rng(8)
    n, nq, nsq, ma, R = 200000, 64, 8, 8, 100
    centers = (rng.normal(size=(500, DIM)) * 3).astype(np.float32)
    vectors = (centers[rng.integers(0, 500, n)] + rng.normal(size=(n, DIM))).astype(np.float32)
    queries = (centers[rng.integers(0, 500, nq)] + rng.normal(size=(nq, DIM))).astype(np.float32)
    coarse, _ = pyqadc.kmeans_iterations(vectors[:20000], vectors[rng.choice(n, K, replace=False)], 5)
    sample = vectors[rng.choice(n, 256, replace=False)]
    sa = ac.assign(po, sample, coarse, 1)[:, 0]
    codebooks = np.ascontiguousarray((sample - coarse[sa]).reshape(256, nsq, DIM // nsq).transpose(1, 0, 2), np.float32)
    a, codes = pyqadc.adc_encode(codebooks, vectors, coarse)
    check = rng.choice(n, 2000, replace=False)
    want_a, want_c = ac.encode(po, codebooks, vectors[check], coarse)
    assert np.array_equal(a[check], want_a) and np.array_equal(codes[check], want_c)
    order = np.argsort(a, kind="stable")
    bounds = np.searchsorted(a[order], np.arange(K + 1))
    parts = [codes[order[bounds[k]:bounds[k + 1]]] for k in range(K)]
    labels = [order[bounds[k]:bounds[k + 1]].astype(np.uint32) for k in range(K)]
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    idx.set_pq(codebooks)
    idx.set_coarse(coarse)
    keys, vals, sizes, got_a = idx.search(queries, ma, R)
    want_qa = ac.assign(po, queries, coarse, ma)
    assert np.array_equal(got_a, want_qa)
    want_t = ac.tables(po, codebooks, ac.residuals(queries, coarse, want_qa), 2)
    hits = 0
    for q in range(nq):
        want = expected(po, nsq, [parts[k] for k in want_qa[q]], [labels[k] for k in want_qa[q]], want_t[q], R)
        assert_heap((keys, vals, sizes), want, q, "encoded database")
        exact = np.argsort(((vectors - queries[q]) ** 2).sum(axis=1))[:R]
        hits += len(np.intersect1d(exact, keys[q, :sizes[q]]))
    print("recall@%d against exact float L2 over %d queries: %.3f" % (R, nq, hits / float(nq * R)))
    idx.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------

@path_independent
def test_search_refusals_leave_the_index_usable(po):
    rng = np.random.default_rng(9)
    nsq, dim = 8, 64
    parts, labels = ivf_db(rng, nsq, K, 5000)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    codebooks = rng.normal(size=(nsq, 256, dim // nsq)).astype(np.float32)
    coarse = rng.normal(size=(K, dim)).astype(np.float32)
    queries = rng.normal(size=(3, dim)).astype(np.float32)

    def refused(match, f, *args):
        with pytest.raises(pyqadc.QadcError, match=match) as e:
            f(*args)
        assert "qadc error %d:" % pyqadc.QADC_E_ARG in str(e.value)

    refused("set_pq", idx.search, queries, 4, 10)                          # search before set_pq
    refused("set_pq", idx.search_tables, queries, 4)
    refused("set_pq", idx.set_coarse, coarse)
    refused("multiple", idx.set_pq_raw, 60, np.zeros(nsq * 256 * 8, np.float32))   # dim % sq_count != 0
    refused("set_pq", idx.search, queries, 4, 10)
    idx.set_pq(codebooks)
    idx.set_coarse(coarse[:K - 1])                                         # K != partition count
    refused("partitions", idx.search, queries, 4, 10)
    refused("partitions", idx.search_tables, queries, 4)
    idx.set_coarse(coarse)
    refused("exceeds", idx.search, queries, K + 1, 10)                     # ma > K
    refused("table_form", idx.search, queries, 4, 10, 3)
    refused("sum_mode", idx.search, queries, 4, 10, 2, 2)
    refused("R must", idx.search, queries, 4, 0)
    keys, vals, sizes, a = idx.search(queries, 4, 10)                      # still usable, and right
    want_a = ac.assign(po, queries, coarse, 4)
    want_t = ac.tables(po, codebooks, ac.residuals(queries, coarse, want_a), 2)
    assert np.array_equal(a, want_a)
    for q in range(3):
        want = expected(po, nsq, [parts[k] for k in want_a[q]], [labels[k] for k in want_a[q]], want_t[q], 10)
        assert_heap((keys, vals, sizes), want, q, "after the refusals")
    idx.close()
    empty = pyqadc.AdcIndex(nsq, 8)                                        # a flat index needs its partition
    empty.set_pq(codebooks)
    refused("partition", empty.search, queries, 1, 10)
    empty.close()
    with pytest.raises(pyqadc.QadcError):
        pyqadc.adc_encode(codebooks[:, :, :7].copy().reshape(7, 256, 8), queries[:, :56].copy())   # sq_count 7
