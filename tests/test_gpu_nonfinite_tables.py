"""GPU: the float front of the 4-bit engine (pre-scan, qmin / clamp, QuantizerMAX) on NaN, +-inf and +-FLT_MAX tables.

The reference is compiled with -ffast-math, so what it does with a NaN is what its instructions do (oracle/qadc_oracle.c:
orc_min_element_compiled, orc_quantize_tables; the start scan never pushes a NaN sum, nor +inf, nor FLT_MAX itself):
  * qmax   = the R-th smallest pre-scan sum BELOW FLT_MAX, FLT_MAX (status 1) when there are fewer than R of them;
  * qmin   = the build's min reduction, in which a NaN makes a lane forget what it saw before: NaN when the table's last entry is
             NaN (then nothing is clamped), possibly above the true minimum otherwise;
  * int8   = 127 for a NaN entry (the worst score), the low byte of the truncation otherwise.
Expected values: tests/golden/ref_query_scan_nonfinite_cases.npz (outputs of the reference build, oracle/gen_golden_float.py) and
the oracle, which tests/test_oracle_float_ref.py pins to that build on these input families.  Every comparison is bit for bit:
status, sizes, qmin and qmax as bits, the int8 tables, the heap arrays, sort_keys of them, the caller's tables after the call.

Negative int8 tables.  Where a NaN makes the build's qmin overshoot finite entries (a NaN late in their lane, or in the two entries
before the table's end), those entries quantize BELOW 0.  The streaming int8 scan kernels are exact for entries in [0, 127] only
(without a NaN, qmin is the minimum and nothing is negative), so the library answers such a query from
candidates_i8_signed_kernel — scan_avx_4's saturating signed chains for every code — replayed on the host by the reference's
block-wise push rule.  The heaps of these queries are compared like all others; test_heaps_under_negative_int8_tables makes sure
the fixture holds such a case and that the oracle's int8 scan of it is the reference build's."""
import numpy as np
import pytest

import golden_cases
from helpers import float_tables, path_independent, rand_codes

pytestmark = pytest.mark.gpu

NAN_POS, NAN_NEG, INF_POS, INF_NEG = 0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000


def f32(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


_FIXTURE = {}


def fixture_cases(po):
    """The fixture's cases by database id, each with the oracle's result beside the reference's (computed once per session)."""
    if not _FIXTURE:
        for c in golden_cases.nonfinite_cases(po):
            c["tables_after"] = c["tables"].copy()
            c["want"] = po.query_scan(c["M"], c["parts"], c["labels"], c["keep"], c["assign"], c["tables_after"], c["R"])
            w = c["want"]
            # the oracle IS the reference build on these cases (also asserted on the CPU, where the build is live)
            assert w["rc"] == c["exit"] and w["qmax_bits"] == int(bits(c["qmax"])[0]), c["cid"]
            if not c["exit"]:
                assert np.array_equal(w["keys"], c["keys"]) and np.array_equal(w["values"], c["vals"]), c["cid"]
                assert np.array_equal(bits(c["tables_after"]), c["after"].reshape(-1)), c["cid"]
            _FIXTURE.setdefault(c["dbi"], []).append(c)
    return _FIXTURE


def check_query(po, pyqadc, got, q, want, t_dev, t_orc, tag, sorted_keys=None):
    """One query of a query_scan result against the oracle's dict; t_dev / t_orc: the caller's tables after the two calls."""
    assert int(got["status"][q]) == want["rc"], tag
    assert int(bits(got["qmax"][q:q + 1])[0]) == want["qmax_bits"], (tag, got["qmax"][q], want["qmax"])
    if want["rc"]:
        return
    assert int(bits(got["qmin"][q:q + 1])[0]) == want["qmin_bits"], (tag, got["qmin"][q], want["qmin"])
    if got.get("qtables") is not None:
        bad = np.nonzero(got["qtables"][q].reshape(-1) != want["qtables"].reshape(-1))[0]
        assert not len(bad), (tag, bad[:8], got["qtables"][q].reshape(-1)[bad[:8]], want["qtables"].reshape(-1)[bad[:8]])
    keys, vals = got["heaps"][q]
    assert int(got["sizes"][q]) == len(want["keys"]), tag
    assert np.array_equal(keys, want["keys"]) and np.array_equal(vals, want["values"]), tag
    sk = po.sort_keys_i8(want["keys"], want["values"])
    assert np.array_equal(pyqadc.sort_keys_i8(keys, vals), sk), tag
    if sorted_keys is not None:
        assert np.array_equal(sk, sorted_keys), tag
    assert np.array_equal(bits(t_dev), bits(t_orc)), tag           # clamped only when qmin < 0; NaN entries keep their bits


def open_index(pyqadc, M, parts, labels, keep, profile=1, **options):
    idx = pyqadc.Index(M)
    idx.add_partitions(parts, labels)
    idx.finalize(float(keep))
    if profile:
        idx.set_option("profile", 1)
    for k, v in options.items():
        idx.set_option(k, v)
    return idx


def path_taken(prof, scan_path):
    """The scan path the test asked for is the one that ran (profile() counters)."""
    if scan_path == "wgq":
        return prof["wgq_launches"] > 0
    if scan_path == "levels_head":
        return prof["head_launches"] > 0
    return prof["scan_launches"] + prof["small_launches"] + prof["mq_launches"] > 0


@pytest.mark.parametrize("dbi", [0, 1, 2])
def test_query_scan_on_the_reference_builds_nonfinite_cases(pyqadc, po, scan_path, dbi):
    """Every case of the fixture through query_scan, one query per call and then all cases of one R in one batch: 16x4 and 32x4 on
    a flat partition of 20 000 codes (keep 0.05), and the IVF cases with ma = 4 where one probe's table holds the NaN."""
    cs = fixture_cases(po)[dbi]
    c0 = cs[0]
    idx = open_index(pyqadc, c0["M"], c0["parts"], c0["labels"], c0["keep"])
    for c in cs:
        t = c["tables"].copy().reshape(1, len(c["assign"]), -1)
        got = idx.query_scan(c["assign"][None, :], t, c["R"], want_qtables=True)
        check_query(po, pyqadc, got, 0, c["want"], t, c["tables_after"], (c["cid"], c["family"]), c.get("sorted"))
    same = [c for c in cs if c["R"] == 100]
    t = np.ascontiguousarray(np.stack([c["tables"] for c in same]))
    got = idx.query_scan(np.stack([c["assign"] for c in same]), t, 100, want_qtables=True)
    for q, c in enumerate(same):
        check_query(po, pyqadc, got, q, c["want"], t[q], c["tables_after"], ("batch", c["cid"], c["family"]))
    prof = idx.profile()
    idx.close()
    assert path_taken(prof, scan_path), prof
    assert len(same) >= 2 and sum(c["exit"] for c in cs) >= (1 if dbi < 2 else 0)


@path_independent
def test_heaps_under_negative_int8_tables(pyqadc, po):
    """The fixture's cases whose int8 tables (the reference build's, through the oracle) hold negative entries — case n36: 32x4, a
    NaN in the entry before the table's end, 3 % negative entries, qmin = the last entry, 171 entries below 0 — on the library's
    default path: the heap after the whole query_scan is the reference's (before the signed replay existed the device's heap held
    2 entries where the reference's holds 100)."""
    n = 0
    for dbi, cs in fixture_cases(po).items():
        neg = [c for c in cs if not c["exit"] and c["want"]["qtables"].min() < 0]
        if not neg:
            continue
        idx = open_index(pyqadc, cs[0]["M"], cs[0]["parts"], cs[0]["labels"], cs[0]["keep"])
        for c in neg:
            got = idx.query_scan(c["assign"][None, :], c["tables"].copy().reshape(1, len(c["assign"]), -1), c["R"])
            assert np.array_equal(got["heaps"][0][0], c["keys"]) and np.array_equal(got["heaps"][0][1], c["vals"]), (c["cid"], c["family"])
            n += 1
        idx.close()
    assert n >= 1


@pytest.mark.parametrize("dbi", [0, 1, 2])
def test_scan_start_alone_on_nonfinite_tables(pyqadc, po, scan_path, dbi):
    """qadc_scan_start: qmax alone = the top of the reference's float heap after query_scan_start, as bits — FLT_MAX where NaN
    sums, +inf sums and FLT_MAX sums leave fewer than R pushable starts, however many starts there are."""
    cs = [c for c in fixture_cases(po)[dbi] if c["R"] == 100]
    idx = open_index(pyqadc, cs[0]["M"], cs[0]["parts"], cs[0]["labels"], cs[0]["keep"])
    for c in cs:
        qmax = idx.scan_start(c["assign"][None, :], c["tables"].copy(), 100)
        assert int(bits(qmax)[0]) == int(bits(c["qmax"])[0]), (c["cid"], c["family"], qmax, c["qmax"])
    qmax = idx.scan_start(np.stack([c["assign"] for c in cs]), np.stack([c["tables"] for c in cs]), 100)
    assert np.array_equal(bits(qmax), bits(np.array([c["qmax"] for c in cs]))), [c["cid"] for c in cs]
    idx.close()


def nonfinite_families(rng, M, ma=1):
    """(name, tables [ma][M*16]) on fresh random tables: the families of the fixture, for fronts the fixture's shapes do not reach."""
    last = ma * M * 16 - 1

    def base(neg=False):
        return float_tables(rng, 1, ma, M, negatives=neg)[0]

    def put(t, where, vals):
        flat = t.reshape(-1)
        for i, w in enumerate(np.atleast_1d(where)):
            flat[int(w)] = f32(vals[i % len(vals)])
        return t
    out = [("nan_first", put(base(), 0, [NAN_POS])), ("nan_middle", put(base(), 87, [NAN_NEG])),
           ("nan_row_end", put(base(), 63, [NAN_POS])), ("nan_table_end", put(base(), last, [NAN_NEG])),
           ("nan_before_end_negatives", put(base(True), last - 1, [NAN_POS])), ("nan_middle_negatives", put(base(True), 87, [NAN_NEG])),
           ("nan_row", put(base(), np.arange(48, 64), [NAN_POS, NAN_NEG])),
           ("nan_sparse", put(base(), rng.choice(last, 12, replace=False), [NAN_POS, NAN_NEG, 0x7fffffff, 0xffffffff])),
           ("inf_middle", put(base(), [87, 200], [INF_POS, INF_NEG])), ("fmax_sparse", put(base(), rng.choice(last, 8, replace=False), [0x7f7fffff, 0xff7fffff])),
           ("inf_minus_inf_sums", put(put(base(), np.arange(32, 40), [INF_POS]), np.arange(80, 86), [INF_NEG])),
           ("most_sums_nan", put(base(), np.arange(15), [NAN_POS, NAN_NEG])),
           ("all_nan", put(base(), np.arange(last + 1), [NAN_NEG, NAN_POS])), ("all_pinf", put(base(), np.arange(last + 1), [INF_POS]))]
    t = base()
    out.append(("nan_argmin", put(t, int(np.argmin(t)), [NAN_POS])))
    out.append(("nan_ties", put(np.round(base() * 2) / 2, 130, [NAN_NEG])))
    return out


@path_independent
@pytest.mark.parametrize("M", [16, 32])
def test_sliced_lone_front_on_nonfinite_tables(pyqadc, po, M):
    """lone_front_kernel (wgq = 1, one query, 300 000 codes, keep 0.05: 15 000 starts in slices): every slice's R smallest keys,
    the last workgroup's select over their union, qmin / clamp / QuantizerMAX there.  R = 100 and 1."""
    rng = np.random.default_rng(1700 + M)
    n, keep = 300000, np.float32(0.05)
    parts = [rand_codes(rng, n, M)]
    idx = open_index(pyqadc, M, parts, None, keep, profile=0, wgq=1)     # (the timed launches of "profile" take the walk's own front)
    a = np.zeros((1, 1), np.int32)
    nexit = 0
    for name, tb in nonfinite_families(rng, M):
        for R in ((100, 1) if name in ("nan_middle", "most_sums_nan") else (100,)):
            t_dev, t_orc = tb.copy().reshape(1, 1, -1), tb.copy()
            got = idx.query_scan(a, t_dev, R, want_qtables=True)
            want = po.query_scan(M, parts, None, keep, a[0], t_orc, R)
            check_query(po, pyqadc, got, 0, want, t_dev, t_orc, (name, R))
            nexit += want["rc"]
    sliced = idx.profile()["lone_front_launches"]
    idx.close()
    assert sliced >= 3 and nexit >= 2, (sliced, nexit)


@pytest.mark.parametrize("M", [16, 32])
def test_prescanned_submit_on_nonfinite_tables(pyqadc, po, scan_path, M):
    """The sharded pre-scan: each slice exports its R smallest values (NaN sums are none of them), and the submit that takes the
    gathered values selects qmax among them: heaps and exit statuses of the whole query_scan."""
    rng = np.random.default_rng(2300 + M)
    W, R, keep = 3, 100, np.float32(0.05)
    parts = [rand_codes(rng, 40000, M)]
    idx = open_index(pyqadc, M, parts, None, keep)
    fam = nonfinite_families(rng, M)
    nq = len(fam)
    assign = np.zeros((nq, 1), np.int32)
    tables = np.ascontiguousarray(np.stack([t for _, t in fam]))
    gathered = []
    for r in range(W):
        idx.prescan_submit(r % 2, assign, tables.copy(), R, r, W)
        gathered.append(idx.prescan_collect(r % 2))
    gathered = np.concatenate(gathered, axis=1)
    assert not np.isnan(gathered).any()
    t_dev = tables.copy()
    idx.submit(0, assign, t_dev, R, prescan=gathered)
    got = idx.collect(0)
    nexit = 0
    for q, (name, _) in enumerate(fam):
        t_orc = tables[q].copy()
        want = po.query_scan(M, parts, None, keep, assign[q], t_orc, R)
        assert int(got["status"][q]) == want["rc"], name
        nexit += want["rc"]
        if want["rc"]:
            continue
        assert np.array_equal(bits(t_dev[q]), bits(t_orc)), name
        sz = int(got["sizes"][q])
        assert sz == len(want["keys"]) and np.array_equal(got["keys"][q, :sz], want["keys"]) and np.array_equal(got["values"][q, :sz], want["values"]), name
        assert np.array_equal(bits(t_dev[q]), bits(t_orc)), name
    idx.close()
    assert nexit >= 2


def ivf_database(rng, M, sizes):
    parts = [rand_codes(rng, s, M) for s in sizes]
    perm = rng.permutation(sum(sizes)).astype(np.uint32) + 5
    return parts, list(np.split(perm, np.cumsum(sizes)[:-1]))


@pytest.mark.parametrize("M", [16, 32])
def test_one_nonfinite_query_in_a_batch_of_eight(pyqadc, po, scan_path, M):
    """Eight IVF queries with ma = 4 share the pre-scan passes; query 3's tables are non-finite (in one probe's table in most
    families, a whole probe's table for all_nan / all_pinf), the others come out exactly as in the all-finite batch, and query 3 as the oracle has it."""
    rng = np.random.default_rng(3100 + M)
    keep, R, ma = np.float32(0.05), 100, 4
    parts, labels = ivf_database(rng, M, [3000, 2500, 17, 3500, 900, 4100])
    idx = open_index(pyqadc, M, parts, labels, keep)
    assign = np.stack([rng.permutation(len(parts))[:ma] for _ in range(8)]).astype(np.int32)
    finite = float_tables(rng, 8, ma, M, negatives=True)
    t_fin = finite.copy()
    ref = idx.query_scan(assign, t_fin, R, want_qtables=True)
    assert (ref["status"] == 0).all()
    for name, tb in nonfinite_families(rng, M, ma):
        if name.startswith("all_"):
            tb = finite[3].copy()
            tb[2, :] = f32(NAN_NEG if name == "all_nan" else INF_POS)   # the whole table of probe 2, and only that one
        tables = finite.copy()
        tables[3] = tb
        t_dev = tables.copy()
        got = idx.query_scan(assign, t_dev, R, want_qtables=True)
        for q in range(8):
            if q == 3:
                t_orc = tables[3].copy()
                want = po.query_scan(M, parts, labels, keep, assign[3], t_orc, R)
                check_query(po, pyqadc, got, 3, want, t_dev[3], t_orc, name)
                continue
            assert got["status"][q] == 0 and got["sizes"][q] == ref["sizes"][q], (name, q)
            assert np.array_equal(bits(got["qmin"][q:q + 1]), bits(ref["qmin"][q:q + 1])), (name, q)
            assert np.array_equal(bits(got["qmax"][q:q + 1]), bits(ref["qmax"][q:q + 1])), (name, q)
            assert np.array_equal(got["qtables"][q], ref["qtables"][q]), (name, q)
            assert np.array_equal(got["heaps"][q][0], ref["heaps"][q][0]) and np.array_equal(got["heaps"][q][1], ref["heaps"][q][1]), (name, q)
            assert np.array_equal(bits(t_dev[q]), bits(t_fin[q])), (name, q)
    prof = idx.profile()
    idx.close()
    assert path_taken(prof, scan_path), prof


def test_partition_major_batch_with_nonfinite_queries(pyqadc, po):
    """The 256-thread select_kth_kernel in front of a partition-major batch (wgq_group = 2: head launch, grouped second phase):
    96 queries x 8 probes, every eighth query non-finite in one probe's table."""
    M, nq, ma, head = 16, 96, 8, 2
    rng = np.random.default_rng(7000 + M + nq + ma)
    sizes = [int(x) for x in rng.integers(1, 3000, 37)] + [0, 15, 16, 17, 40001, 0, 129, 30000, 25013, 36000]
    parts, labels = ivf_database(rng, M, sizes)
    keep, R = np.float32(0.05), 100
    idx = open_index(pyqadc, M, parts, labels, keep, wgq=2, wgq_group=2, wgq_group_head=head, device_replay_alone_nq=0)
    K, big = len(sizes), [41, 44, 45, 46]
    assign = np.stack([rng.permutation(K)[:ma] for _ in range(nq)]).astype(np.int32)
    for q in range(nq):
        b = big[q % 4]
        assign[q] = [b] + [p for p in assign[q] if p != b][:ma - 1]
    tables = float_tables(rng, nq, ma, M)
    tables = np.ascontiguousarray(tables + np.float32(0.6) * np.arange(ma, dtype=np.float32)[None, :, None])
    fam = nonfinite_families(rng, M)
    hit = {}
    for i, q in enumerate(range(3, nq, 8)):
        name, tb = fam[i % len(fam)]
        src = tb.reshape(-1)
        tables[q, i % ma][~np.isfinite(src)] = src[~np.isfinite(src)]   # the family's non-finite entries, in one probe's table only
        hit[q] = name
    t_dev = tables.copy()
    got = idx.query_scan(assign, t_dev, R, want_qtables=True)
    prof = idx.profile()
    idx.close()
    assert prof["group_launches"] >= 1, prof
    nexit = 0
    for q in range(nq):
        t_orc = tables[q].copy()
        want = po.query_scan(M, parts, labels, keep, assign[q], t_orc, R)
        check_query(po, pyqadc, got, q, want, t_dev[q], t_orc, (q, hit.get(q)))
        nexit += want["rc"]
    assert len(hit) == 12


@pytest.mark.parametrize("M", [16, 32])
def test_search_with_one_nan_query_vector(pyqadc, po, scan_path, M):
    """qadc_search on a batch in which one query vector is NaN: its tables are NaN, every pre-scan sum is NaN, so its status is 1
    (the reference's exit); its neighbours in the batch come out exactly as in the batch without it."""
    rng = np.random.default_rng(4400 + M)
    K, ma, nq, dim, R = 12, 4, 9, 4 * M, 100
    parts, labels = ivf_database(rng, M, [int(x) for x in rng.integers(1500, 5000, K)])
    idx = open_index(pyqadc, M, parts, labels, np.float32(0.05))
    idx.set_pq(rng.normal(size=(M, 16, dim // M)).astype(np.float32))
    idx.set_coarse(rng.normal(size=(K, dim)).astype(np.float32))
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    ref = idx.search(queries, ma, R)
    assert (ref["status"] == 0).all()
    for bad, value in ((4, NAN_POS), (0, NAN_NEG), (nq - 1, NAN_POS)):
        qn = queries.copy()
        qn[bad] = f32(value)
        got = idx.search(qn, ma, R)
        assert got["status"][bad] == 1 and ((got["assign"][bad] >= 0) & (got["assign"][bad] < K)).all(), bad
        for q in range(nq):
            if q == bad:
                continue
            assert got["status"][q] == 0 and np.array_equal(got["assign"][q], ref["assign"][q]), (bad, q)
            assert np.array_equal(got["heaps"][q][0], ref["heaps"][q][0]) and np.array_equal(got["heaps"][q][1], ref["heaps"][q][1]), (bad, q)
    prof = idx.profile()
    idx.close()
    assert path_taken(prof, scan_path), prof
