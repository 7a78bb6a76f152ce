"""The float-ADC engine's device-memory entry points (AdcIndex.search_device / query_scan_device: torch tensors in, torch tensors
out, nothing but assign crosses the bus): the heaps equal the reference's scan on the oracle's composition of the feeders
(tests/adc_compose.py), on the shapes of test_gpu_adc_search.py, bit for bit on keys, values and sizes."""
import numpy as np
import pytest

import pyqadc
from helpers import path_independent
from test_gpu_adc import assert_heap, expected, ivf_db, rand_tables
from test_gpu_adc_search import Case, K, seed_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def to_numpy(out):
    """(keys int32 carrying the uint32 bits, vals, sizes) tensors -> the arrays assert_heap takes"""
    keys, vals, sizes = out
    return keys.cpu().numpy().view(np.uint32), vals.cpu().numpy(), sizes.cpu().numpy()


def check_outputs(out, nq, R, device=0):
    keys, vals, sizes = out
    for t, dtype, shape in ((keys, torch.int32, (nq, R)), (vals, torch.float32, (nq, R)), (sizes, torch.int32, (nq,))):
        assert isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape
        assert t.device.type == "cuda" and t.device.index == device and t.is_contiguous()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
def test_search_device_equals_the_composition(po, nsq, ivf, opq):
    rng = np.random.default_rng(seed_of("search_device", nsq, ivf, opq))
    case = Case(rng, nsq, ivf=ivf, opq=opq)
    nq = 5
    queries = case.queries(rng, nq)
    dq = torch.from_numpy(queries).cuda()
    for table_form, ma, sum_mode in ((2, 1, 1), (2, 8, 1), (0, 24, 1), (1, 24, 1), (1, 8, 0)):
        want_a, want_t, _ = case.compose(po, queries, ma, table_form, sum_mode)
        for R in (1, 100, 1000):
            out = case.idx.search_device(dq, ma, R, table_form, sum_mode)
            check_outputs(out, nq, R)
            got = to_numpy(out)
            for q in range(nq):
                assert_heap(got, case.heaps(po, want_a, want_t, q, R, sum_mode), q,
                            "form %d ma %d R %d sum_mode %d" % (table_form, ma, R, sum_mode))
    assert case.idx.host_finishes() == 0
    case.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
def test_search_device_does_not_depend_on_the_table_budget(po, nsq):
    rng = np.random.default_rng(seed_of("budget_device", nsq))
    case = Case(rng, nsq, ivf=True, opq=nsq == 4)
    nq, ma, R = 10, 8, 100
    queries = case.queries(rng, nq)
    dq = torch.from_numpy(queries).cuda()
    want_a, want_t, _ = case.compose(po, queries, ma, 2)
    per_query = ma * nsq * 256 * 4
    for per in (0, 1, 3):                                      # 0: the default budget, the whole batch in one pass
        case.idx.set_table_budget(per * per_query)
        got = to_numpy(case.idx.search_device(dq, ma, R))
        for q in range(nq):
            assert_heap(got, case.heaps(po, want_a, want_t, q, R), q, "%d queries per pass" % per)
    case.idx.set_table_budget(0)
    assert case.idx.host_finishes() == 0
    case.close()


@path_independent
@pytest.mark.parametrize("nsq", [4, 8, 16])
def test_query_scan_device_on_tables_left_in_device_memory(po, nsq):
    rng = np.random.default_rng(seed_of("query_scan_device", nsq))
    case = Case(rng, nsq, ivf=True, opq=nsq == 16)
    nq, ma = 7, 8
    queries = case.queries(rng, nq)
    assign, tables = case.idx.search_tables(queries, ma)
    want_a, want_t, _ = case.compose(po, queries, ma, 2)
    assert np.array_equal(assign, want_a) and np.array_equal(tables.view(np.uint32), want_t.view(np.uint32))
    dt = torch.from_numpy(tables).cuda()
    for R in (1, 100, 1000):
        out = case.idx.query_scan_device(assign, dt, R)
        check_outputs(out, nq, R)
        got = to_numpy(out)
        host = case.idx.query_scan(assign, tables, R)
        for q in range(nq):
            assert_heap(got, case.heaps(po, want_a, want_t, q, R), q, "R %d" % R)
        for g, h in zip(got, host):
            assert np.array_equal(g.view(np.uint32), h.view(np.uint32)), "query_scan_device and query_scan differ"
    assert case.idx.host_finishes() == 0
    case.close()


@path_independent
def test_query_scan_device_on_special_tables(po):
    """caller-made tables with ties, negative entries and non-finite entries, labelled partitions, duplicate probes"""
    rng = np.random.default_rng(77)
    nsq, nq, ma, R = 8, 6, 8, 100
    parts, labels = ivf_db(rng, nsq)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    assign[0, 1] = assign[0, 0]
    for kind in ("ties", "negative", "nonfinite"):
        tables = rand_tables(rng, nq, ma, nsq, kind)
        got = to_numpy(idx.query_scan_device(assign, torch.from_numpy(tables).cuda(), R))
        for q in range(nq):
            want = expected(po, nsq, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
            assert_heap(got, want, q, kind)
    assert idx.host_finishes() == 0
    idx.close()


@path_independent
def test_a_heap_too_large_for_lds_is_uploaded_into_the_outputs(po):
    rng = np.random.default_rng(5000)
    nsq, n, R = 8, 30000, 5000
    codes = rng.integers(0, 256, (n, nsq), dtype=np.uint8)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions([codes])
    tables = rand_tables(rng, 2, 1, nsq)
    out = idx.query_scan_device(np.zeros((2, 1), np.int32), torch.from_numpy(tables).cuda(), R)
    check_outputs(out, 2, R)
    got = to_numpy(out)
    for q in range(2):
        assert_heap(got, expected(po, nsq, [codes], None, tables[q], R), q, "R=%d" % R)
    print("host_finishes after 2 queries at R = %d through query_scan_device: %d" % (R, idx.host_finishes()))
    assert idx.host_finishes() in (0, 2)
    idx.close()


@path_independent
def test_wrong_tensors_are_refused_before_any_launch(po):
    rng = np.random.default_rng(11)
    case = Case(rng, 8, ivf=True)
    nq, ma, R = 4, 8, 10
    queries = case.queries(rng, nq)
    good = torch.from_numpy(queries).cuda()
    assign, tables = case.idx.search_tables(queries, ma)
    good_t = torch.from_numpy(tables).cuda()
    refusals = (pyqadc.QadcError, TypeError)
    wide = torch.zeros((nq, 2 * case.dim), dtype=torch.float32, device="cuda")
    for bad in (torch.from_numpy(queries),                     # a CPU tensor
                good.double(),                                 # float64
                wide[:, ::2],                                  # not contiguous
                queries):                                      # no tensor at all
        with pytest.raises(refusals):
            case.idx.search_device(bad, ma, R)
    wide_t = torch.zeros((nq, ma, 2 * 8 * 256), dtype=torch.float32, device="cuda")
    for bad in (torch.from_numpy(tables), good_t.double(), wide_t[:, :, ::2], good_t[:, :, :-1].contiguous()):
        with pytest.raises(refusals):
            case.idx.query_scan_device(assign, bad, R)
    # the C entry points refuse like their host twins
    with pytest.raises(pyqadc.QadcError, match="R must"):
        case.idx.search_device(good, ma, 0)
    with pytest.raises(pyqadc.QadcError, match="sum_mode"):
        case.idx.search_device(good, ma, R, 2, 2)
    with pytest.raises(pyqadc.QadcError, match="exceeds"):
        case.idx.search_device(good, K + 1, R)
    with pytest.raises(pyqadc.QadcError, match="partition"):
        case.idx.query_scan_device(np.full((nq, ma), K, np.int32), good_t, R)
    got = to_numpy(case.idx.search_device(good, ma, R))        # still usable, and right
    want_a, want_t, _ = case.compose(po, queries, ma, 2)
    for q in range(nq):
        assert_heap(got, case.heaps(po, want_a, want_t, q, R), q, "after the refusals")
    case.close()


@path_independent
def test_a_nan_row_with_more_than_256_probes_is_refused_by_search_device(po):
    rng = np.random.default_rng(256)
    nsq, dim, k = 8, 32, 300
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions([rng.integers(0, 256, (20, nsq), dtype=np.uint8) for _ in range(k)])
    idx.set_pq(rng.normal(size=(nsq, 256, dim // nsq)).astype(np.float32))
    idx.set_coarse(rng.normal(size=(k, dim)).astype(np.float32))
    queries = rng.normal(size=(4, dim)).astype(np.float32)
    clean = to_numpy(idx.search_device(torch.from_numpy(queries).cuda(), 257, 10))
    host = idx.search(queries, 257, 10)
    for g, h in zip(clean, host[:3]):
        assert np.array_equal(g.view(np.uint32), h.view(np.uint32))
    bad = queries.copy()
    bad[2, 1] = np.nan
    with pytest.raises(pyqadc.QadcError, match="NaN"):
        idx.search_device(torch.from_numpy(bad).cuda(), 257, 10)
    idx.close()
