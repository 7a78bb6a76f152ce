"""qadc_adc_search* on a float-ADC view of a 4-bit index (pyqadc.AdcIndex.view_of): the source index's quantizers — codebooks
[M][16][ds], OPQ rotation, coarse centroids — run on the GPU (coarse assignment, residual, rotation, both table forms), then
the nibble scan.  search_tables must equal the oracle's composition bit for bit (tests/adc_compose.py for assign and
residuals, po.tables_direct / po.tables_expansion on the 16-centroid codebooks); the heaps are then scan_4's on those tables
(tests/adc4_compose.py)."""
import zlib

import numpy as np
import pytest

import adc_compose as ac
import pyqadc
from adc4_compose import assert_heap, expected, replay
from helpers import path_independent

pytestmark = pytest.mark.gpu

K = 64


def seed_of(*what):
    return zlib.crc32(" ".join(str(w) for w in what).encode())


class Case:
    """a 4-bit index with quantizers, and a view of it"""

    def __init__(self, rng, M, ivf, opq=False, ds=8, n=30000):
        self.M, self.dim = M, M * ds
        self.codebooks = rng.normal(size=(M, 16, ds)).astype(np.float32)
        self.coarse = (rng.normal(size=(K, self.dim)) * 2).astype(np.float32) if ivf else None
        self.rotation = ac.random_rotation(rng, self.dim) if opq else None
        if ivf:
            w = rng.pareto(1.2, K) + 0.05
            w[rng.choice(K, 4, replace=False)] = 0                     # empty partitions
            sizes = np.floor(w / w.sum() * n).astype(np.int64)
            perm = rng.permutation(int(sizes.sum())).astype(np.uint32)
            self.parts = [rng.integers(0, 256, (int(s), M // 2), dtype=np.uint8) for s in sizes]
            self.labels, o = [], 0
            for s in sizes:
                self.labels.append(perm[o:o + s].copy())
                o += s
        else:
            self.parts = [rng.integers(0, 256, (n, M // 2), dtype=np.uint8)]
            self.labels = None
        self.src = pyqadc.Index(M)
        self.src.add_partitions(self.parts, self.labels)
        self.src.finalize(0.01)
        self.src.set_pq(self.codebooks)
        if opq:
            self.src.set_rotation(self.rotation)
        if ivf:
            self.src.set_coarse(self.coarse)
        self.view = pyqadc.AdcIndex.view_of(self.src)

    def queries(self, rng, nq):
        q = rng.normal(size=(nq, self.dim)).astype(np.float32)
        if self.coarse is not None:
            q = (q + self.coarse[rng.integers(0, K, nq)]).astype(np.float32)
        return q

    def compose(self, po, queries, ma, table_form, sum_mode=1):
        """-> (assign [nq][ma], tables [nq][ma][M*16]) as the reference's feeders compute them"""
        a = ac.assign(po, queries, self.coarse, ma, sum_mode)
        res = ac.residuals(queries, self.coarse, a, self.rotation)
        nq = len(queries)
        flat = res.reshape(nq * ma, self.dim)
        if ac.expansion_used(table_form, ma):
            t = po.tables_expansion(self.codebooks, flat, sum_mode)
        else:
            t = np.stack([po.tables_direct(self.codebooks, v, sum_mode) for v in flat])
        return a, np.ascontiguousarray(t.reshape(nq, ma, self.M * 16), np.float32)

    def heaps(self, po, a, tables, q, R, sum_mode=1):
        labels = None if self.labels is None else [self.labels[k] for k in a[q]]
        return expected(po, self.M, [self.parts[k] for k in a[q]], labels, tables[q], R, sum_mode)

    def close(self):
        self.view.close()
        self.src.close()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@path_independent
@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
def test_search_matches_the_composition(po, M, ivf, opq):
    rng = np.random.default_rng(seed_of("search", M, ivf, opq))
    case = Case(rng, M, ivf, opq)
    queries = case.queries(rng, 5)
    for ma in ((1, 8, 24) if ivf else (1,)):
        for table_form in (0, 1, 2):
            for sum_mode in ((1, 0) if table_form == 2 else (1,)):
                what = "M %d ma %d form %d sum_mode %d" % (M, ma, table_form, sum_mode)
                want_a, want_t = case.compose(po, queries, ma, table_form, sum_mode)
                got_a, got_t = case.view.search_tables(queries, ma, table_form, sum_mode)
                assert np.array_equal(got_a, want_a), what
                assert got_t.shape == (5, ma, M * 16)
                ac.assert_same_floats(got_t, want_t, what)
                for R in (1, 100):
                    got = case.view.search(queries, ma, R, table_form, sum_mode)
                    assert np.array_equal(got[3], want_a), what
                    for q in range(len(queries)):
                        assert_heap(got[:3], case.heaps(po, want_a, want_t, q, R, sum_mode), q, what + " R %d" % R)
    case.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
def test_candidates_and_device_entry_points_agree(po, M):
    import torch
    rng = np.random.default_rng(seed_of("entry points", M))
    case = Case(rng, M, ivf=True, opq=True)
    nq, ma, R = 9, 8, 64
    queries = case.queries(rng, nq)
    want_a, want_t = case.compose(po, queries, ma, 2)
    direct = case.view.search(queries, ma, R)
    for q in range(nq):
        assert_heap(direct[:3], case.heaps(po, want_a, want_t, q, R), q, "search")
    keys, vals, offsets, a = case.view.search_candidates(queries, ma, R)
    assert np.array_equal(a, want_a) and offsets[0] == 0 and offsets[-1] == len(keys)
    for q in range(nq):
        lo, hi = int(offsets[q]), int(offsets[q + 1])
        assert_heap(direct[:3], replay(po, keys[lo:hi], vals[lo:hi], R), q, "search_candidates")
    dq = torch.from_numpy(queries).cuda()
    torch.cuda.synchronize()
    dk, dv, dsz = case.view.search_device(dq, ma, R)
    assert dk.is_cuda and dv.is_cuda and dsz.is_cuda
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), direct[0]) and same_bits(dv.cpu().numpy(), direct[1])
    assert np.array_equal(dsz.cpu().numpy(), direct[2])
    dt = torch.from_numpy(want_t).cuda()                   # the tables in device memory
    torch.cuda.synchronize()
    dk, dv, dsz = case.view.query_scan_device(want_a, dt, R)
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), direct[0]) and same_bits(dv.cpu().numpy(), direct[1])
    assert np.array_equal(dsz.cpu().numpy(), direct[2])
    with pytest.raises(pyqadc.QadcError, match="shape"):   # tables of the whole-byte engine's size
        case.view.query_scan_device(want_a, torch.zeros((nq, ma, M * 256), dtype=torch.float32, device="cuda"), R)
    case.view.set_finish(1)                                # the device finish under search()
    dev = case.view.search(queries, ma, R)
    assert all(same_bits(x, y) for x, y in zip(dev[:3], direct[:3])) and case.view.host_finishes() == 0
    case.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("per_pass", [1, 3])
def test_table_budget_splits_the_batch(po, M, per_pass):
    """the budget counts M * 16 * 4 bytes per (query, probe): a budget of per_pass queries' tables runs the batch in passes"""
    rng = np.random.default_rng(seed_of("budget", M, per_pass))
    case = Case(rng, M, ivf=True)
    nq, ma, R = 7, 8, 50
    queries = case.queries(rng, nq)
    whole = case.view.search(queries, ma, R)
    whole_t = case.view.search_tables(queries, ma)
    whole_c = case.view.search_candidates(queries, ma, R)
    case.view.set_table_budget(per_pass * ma * M * 16 * 4)
    for finish in (0, 1):
        case.view.set_finish(finish)
        got = case.view.search(queries, ma, R)
        assert all(same_bits(x, y) for x, y in zip(got, whole)), "finish %d" % finish
    got_t = case.view.search_tables(queries, ma)
    assert np.array_equal(got_t[0], whole_t[0]) and same_bits(got_t[1], whole_t[1])
    got_c = case.view.search_candidates(queries, ma, R)
    assert all(same_bits(x, y) for x, y in zip(got_c[:2], whole_c[:2])) and np.array_equal(got_c[2], whole_c[2])
    want_a, want_t = case.compose(po, queries, ma, 2)
    for q in range(nq):
        assert_heap(got[:3], case.heaps(po, want_a, want_t, q, R), q, "budget of %d queries" % per_pass)
    case.view.set_table_budget(0)
    case.close()


@path_independent
def test_the_source_quantizers_are_read_at_the_call(po):
    """a view has no quantizer of its own: what qadc_index_set_* put on the source when the call is made is what runs"""
    rng = np.random.default_rng(5)
    M = 16
    case = Case(rng, M, ivf=True)
    queries = case.queries(rng, 4)
    first = case.view.search_tables(queries, 8)
    case.coarse = (rng.normal(size=(K, case.dim)) * 2).astype(np.float32)
    case.src.set_coarse(case.coarse)
    case.codebooks = rng.normal(size=(M, 16, 8)).astype(np.float32)
    case.src.set_pq(case.codebooks)
    want_a, want_t = case.compose(po, queries, 8, 2)
    got_a, got_t = case.view.search_tables(queries, 8)
    assert np.array_equal(got_a, want_a) and not np.array_equal(got_a, first[0])
    ac.assert_same_floats(got_t, want_t, "after the source's set_coarse / set_pq")
    case.close()


@path_independent
def test_a_nan_row_with_more_than_256_probes_is_refused(po):
    rng = np.random.default_rng(256)
    M, dim, k = 16, 32, 300
    src = pyqadc.Index(M)
    src.add_partitions([rng.integers(0, 256, (20, M // 2), dtype=np.uint8) for _ in range(k)])
    src.finalize(0.01)
    coarse = rng.normal(size=(k, dim)).astype(np.float32)
    src.set_pq(rng.normal(size=(M, 16, dim // M)).astype(np.float32))
    src.set_coarse(coarse)
    view = pyqadc.AdcIndex.view_of(src)
    queries = rng.normal(size=(4, dim)).astype(np.float32)
    clean = view.search(queries, 257, 10)
    bad = queries.copy()
    bad[2, 1] = np.nan
    with pytest.raises(pyqadc.QadcError, match="NaN"):
        view.search(bad, 257, 10)
    with pytest.raises(pyqadc.QadcError, match="NaN"):
        view.search_tables(bad, 257)
    again = view.search(queries, 257, 10)                      # the view stays usable
    assert all(np.array_equal(g, r) for g, r in zip(again, clean))
    got = view.search(bad, 256, 10)                            # 256 probes: the reference's heap replay decides
    with np.errstate(all="ignore"):
        want_a = ac.assign(po, bad, coarse, 256)
    assert np.array_equal(got[3], want_a)
    with pytest.raises(pyqadc.QadcError, match="exceeds"):
        view.search(queries, k + 1, 10)
    view.close()
    src.close()
