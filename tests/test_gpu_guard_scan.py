"""GPU: the memory behaviour of the float-ADC query entry points at the C-ABI, on guard-band arenas
(tests/guard_arena.py): qadc_adc_query_scan_device, qadc_adc_search_device, their _filtered forms, qadc_adc_range_scan_device,
_range_search_device and _range_collect_device through raw ctypes calls on windows of a larger device buffer, and the host forms
with a capacity (qadc_adc_range_collect, qadc_adc_query_scan_candidates, qadc_adc_search_candidates) on the numpy arena.

W  every byte outside the declared outputs is unchanged by the call (guard bands and inputs);
R  the outputs under the two guard poisons are bit-identical, and equal the same call made through the pyqadc wrapper and the host form;
F  no output element the header documents keeps either output poison (0xFF.. / 0x5A..): follows from R, since the wrappers hand in zeros;
A  every buffer at the smallest alignment include/qadc.h allows (d_tables 16 bytes, everything else its element's 4), and at 256.

Every compare is for equality.  The shapes are the smallest that reach each scan instantiation: 8x8, 16x8, 2x16 and the 16x4 view."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = (301, 257, 199)                                      # odd, more than one workgroup's codes, no multiple of a tile
NQ, MA = 3, 2
ASSIGN = np.array([[0, 1], [2, 0], [1, 1]], np.int32)        # a duplicate probe in the last query
ALIGNS = ["min", 256]


def al(align, minimum):
    return minimum if align == "min" else align


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


class Db:
    """one small database per shape, built once per module, with a filter set that really drops rows"""

    def __init__(self, pyqadc, shape):
        rng = np.random.default_rng(sum(map(ord, shape)))
        self.shape, self.src = shape, None
        if shape == "16x4v":
            self.src = pyqadc.Index(16)
            self.src.add_partitions([rng.integers(0, 256, (n, 8), dtype=np.uint8) for n in SIZES])
            self.src.finalize(0.5)
            self.idx = pyqadc.AdcIndex.view_of(self.src)
            keys = np.arange(0, 120, dtype=np.uint32)                        # positions
        else:
            nsq, wide = int(shape.split("x")[0]), shape.endswith("x16")
            self.idx = pyqadc.AdcIndex.create16(nsq) if wide else pyqadc.AdcIndex(nsq, 8)
            codes = [rng.integers(0, 65536 if wide else 256, (n, nsq)).astype(np.uint16 if wide else np.uint8) for n in SIZES]
            labels = None
            keys = np.arange(0, 120, dtype=np.uint32)
            if shape == "8x8":                                               # one labelled database
                perm = rng.permutation(sum(SIZES)).astype(np.uint32) + 1000
                labels = np.split(perm, np.cumsum(SIZES)[:-1])
                keys = perm[::3].copy()
            self.idx.add_partitions(codes, labels)
        self.filter = pyqadc.AdcFilter(keys, "exclude")
        self.tables = rng.normal(size=(NQ, MA, self.idx.table_dim)).astype(np.float32) ** 2

    def close(self):
        self.idx.close()
        self.filter.close()
        if self.src is not None:
            self.src.close()


@pytest.fixture(scope="module")
def dbs(pyqadc):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Db(pyqadc, shape)
        return made[shape]
    yield get
    for db in made.values():
        db.close()


def heaps_of(out):
    keys, vals, sizes = out
    if isinstance(keys, torch.Tensor):
        keys, vals, sizes = keys.cpu().numpy().view(np.uint32), vals.cpu().numpy(), sizes.cpu().numpy()
    return dict(keys=keys, vals=vals, sizes=sizes)


def place_heaps(a, nq, R, align):
    return (a.place(np.empty((nq, R), np.uint32), al(align, 4), "out", name="d_keys"),
            a.place(np.empty((nq, R), np.float32), al(align, 4), "out", name="d_values"),
            a.place(np.empty(nq, np.int32), al(align, 4), "out", name="d_sizes"))


def scan_call(pyqadc, db, fl, R, tables_ptr, k, v, s):
    L, p = pyqadc.lib(), ASSIGN.ctypes.data_as(C.POINTER(C.c_int32))
    if fl is None:
        return L.qadc_adc_query_scan_device(db.idx._h, NQ, MA, p, tables_ptr, R, 1, k, v, s)
    return L.qadc_adc_query_scan_device_filtered(db.idx._h, NQ, MA, p, tables_ptr, R, 1, k, v, s, fl)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])
@pytest.mark.parametrize("R", [1, 100, 4097])
@pytest.mark.parametrize("shape", ["8x8", "16x8", "2x16", "16x4v"])
def test_query_scan_device(pyqadc, dbs, shape, R, filtered, align):
    db = dbs(shape)
    filters = [db.filter, None, db.filter] if filtered else None

    def call(a):
        t = a.place(db.tables, al(align, 16), "in", name="d_tables")
        k, v, s = place_heaps(a, NQ, R, align)
        a.snapshot()
        rc = scan_call(pyqadc, db, db.idx._filters(filters, NQ), R, a.ptr(t), a.ptr(k), a.ptr(v), a.ptr(s))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([k, v, s])
        return heaps_of((a.host(k), a.host(v), a.host(s)))

    got = ga.under_both_poisons(call, backend="torch", capacity=db.tables.nbytes + (1 << 20))
    assert (got["sizes"] == R).all()                                         # the sentinels fill every heap
    wrapper = heaps_of(db.idx.query_scan_device(ASSIGN, torch.from_numpy(db.tables).cuda(), R, filters=filters))
    assert ga.same(got, wrapper) is None, "%s differs from the wrapper's call" % ga.same(got, wrapper)
    host = heaps_of(db.idx.query_scan(ASSIGN, db.tables, R, filters=filters))
    assert ga.same(got, host) is None, "%s differs from the host form" % ga.same(got, host)
    if filtered and R > 1:
        plain = heaps_of(db.idx.query_scan(ASSIGN, db.tables, R))
        assert ga.same(plain, host) == "keys"                                # (the filter drops rows that would have entered)


@path_independent
@pytest.mark.parametrize("shape", ["8x8", "16x4v"])
def test_query_scan_device_refuses_pointers_below_the_stated_alignment(pyqadc, dbs, shape):
    """d_tables at 4 (mod 8) bytes, then each output two bytes off: QADC_E_ARG before any HIP call, nothing written, the index as before"""
    db, R = dbs(shape), 100
    before = heaps_of(db.idx.query_scan(ASSIGN, db.tables, R))
    for poison in ga.POISONS:
        a = ga.Arena(poison, backend="torch", capacity=1 << 20)
        low = a.place(db.tables, 4, "in", name="d_tables at 4 bytes")
        good = a.place(db.tables, 16, "in", name="d_tables")
        k, v, s = place_heaps(a, NQ, R, "min")
        assert a.ptr(low) % 16 in (4, 12) and a.ptr(good) % 32 == 16
        for fl in (None, db.idx._filters([db.filter, None, None], NQ)):
            for off in ((1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2)):
                a.snapshot()
                rc = scan_call(pyqadc, db, fl, R, a.ptr(low) if off[0] else a.ptr(good), a.ptr(k) + off[1], a.ptr(v) + off[2], a.ptr(s) + off[3])
                assert rc == pyqadc.QADC_E_ARG and b"aligned" in pyqadc.lib().qadc_last_error(), off
                a.check_untouched([])
        a.snapshot()
        assert scan_call(pyqadc, db, None, R, a.ptr(good), a.ptr(k), a.ptr(v), a.ptr(s)) == 0
        a.check_untouched([k, v, s])
        assert ga.same(heaps_of((a.host(k), a.host(v), a.host(s))), before) is None
    with pytest.raises(pyqadc.QadcError, match="d_tables must be 16-byte aligned"):      # the wrapper: the same C check
        db.idx.query_scan_device(ASSIGN, torch.zeros(db.tables.size + 1, device="cuda")[1:].view(NQ, MA, -1), R)


# ---- from query vectors: qadc_adc_search_device ----

class SearchDb:
    """an IVF database with K = 3 and its quantizers; budget: the tables of two queries, so five queries run in passes of 2, 2 and 1"""

    def __init__(self, pyqadc, shape, ds, opq):
        rng = np.random.default_rng(1000 + ds)
        nsq, wide = int(shape.split("x")[0]), shape.endswith("x16")
        self.dim, self.ma, self.nq = nsq * ds, 2, 5
        self.idx = pyqadc.AdcIndex.create16(nsq) if wide else pyqadc.AdcIndex(nsq, 8)
        self.idx.add_partitions([rng.integers(0, 65536 if wide else 256, (n, nsq)).astype(np.uint16 if wide else np.uint8) for n in SIZES])
        self.idx.set_pq(rng.normal(size=(nsq, self.idx.centroids, ds)).astype(np.float32))
        if opq:
            self.idx.set_rotation(np.linalg.qr(rng.normal(size=(self.dim, self.dim)))[0].astype(np.float32))
        self.idx.set_coarse(rng.normal(size=(len(SIZES), self.dim)).astype(np.float32))
        self.idx.set_table_budget(2 * self.ma * self.idx.table_dim * 4)
        self.queries = rng.normal(size=(self.nq, self.dim)).astype(np.float32)
        self.filter = pyqadc.AdcFilter(np.arange(0, 150, dtype=np.uint32), "exclude")

    def close(self):
        self.idx.close()
        self.filter.close()


SEARCH = [("8x8", 8, True), ("8x8", 16, True), ("8x8", 5, True), ("4x16", 8, False)]       # sub-vectors of 8, of 16, and the any-size feeder


@pytest.fixture(scope="module", params=SEARCH, ids=["%s-ds%d" % s[:2] for s in SEARCH])
def sdb(request, pyqadc):
    db = SearchDb(pyqadc, *request.param)
    yield db
    db.close()


def search_call(pyqadc, db, fl, R, q_ptr, k, v, s):
    L = pyqadc.lib()
    if fl is None:
        return L.qadc_adc_search_device(db.idx._h, db.nq, q_ptr, db.ma, R, 2, 1, k, v, s)
    return L.qadc_adc_search_device_filtered(db.idx._h, db.nq, q_ptr, db.ma, R, 2, 1, k, v, s, fl)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])
@pytest.mark.parametrize("R", [1, 100, 4097])
def test_search_device(pyqadc, sdb, R, filtered, align):
    db = sdb
    filters = [None, db.filter, db.filter, None, db.filter] if filtered else None

    def call(a):
        q = a.place(db.queries, al(align, 4), "in", name="d_queries")
        k, v, s = place_heaps(a, db.nq, R, align)
        a.snapshot()
        rc = search_call(pyqadc, db, db.idx._filters(filters, db.nq), R, a.ptr(q), a.ptr(k), a.ptr(v), a.ptr(s))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([k, v, s])
        return heaps_of((a.host(k), a.host(v), a.host(s)))

    got = ga.under_both_poisons(call, backend="torch", capacity=1 << 20)
    wrapper = heaps_of(db.idx.search_device(torch.from_numpy(db.queries).cuda(), db.ma, R, filters=filters))
    assert ga.same(got, wrapper) is None, "%s differs from the wrapper's call" % ga.same(got, wrapper)
    host = heaps_of(db.idx.search(db.queries, db.ma, R, filters=filters)[:3])
    assert ga.same(got, host) is None, "%s differs from the host form" % ga.same(got, host)


@path_independent
def test_search_device_refuses_pointers_below_the_stated_alignment(pyqadc, sdb):
    db, R = sdb, 100
    before = heaps_of(db.idx.search(db.queries, db.ma, R)[:3])
    a = ga.Arena(ga.P2, backend="torch", capacity=1 << 20)
    q = a.place(db.queries, 4, "in", name="d_queries")
    k, v, s = place_heaps(a, db.nq, R, "min")
    for off in ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2)):
        a.snapshot()
        rc = search_call(pyqadc, db, None, R, a.ptr(q) + off[0], a.ptr(k) + off[1], a.ptr(v) + off[2], a.ptr(s) + off[3])
        assert rc == pyqadc.QADC_E_ARG and b"aligned" in pyqadc.lib().qadc_last_error(), off
        a.check_untouched([])
    a.snapshot()
    assert search_call(pyqadc, db, None, R, a.ptr(q), a.ptr(k), a.ptr(v), a.ptr(s)) == 0
    a.check_untouched([k, v, s])
    assert ga.same(heaps_of((a.host(k), a.host(v), a.host(s))), before) is None


# ---- range search: the held result and its collectors ----

class RangeDb:
    """8x8 with quantizers, flat over partition 0 for the search form; query 0 keeps every row of its probes (5001 + 301, above
    QADC_ADC_RANGE_SORT_LDS: the radix path's output copy), the others a part of theirs"""

    def __init__(self, pyqadc):
        rng = np.random.default_rng(77)
        self.sizes = (5001, 301, 199)
        self.idx = pyqadc.AdcIndex(8, 8)
        self.idx.add_partitions([rng.integers(0, 256, (n, 8), dtype=np.uint8) for n in self.sizes])
        self.idx.set_pq(rng.normal(size=(8, 256, 8)).astype(np.float32))
        self.tables = rng.normal(size=(NQ, MA, 2048)).astype(np.float32) ** 2
        self.radius = np.array([np.inf, 6.0, 5.0], np.float32)
        self.queries = rng.normal(size=(NQ, 64)).astype(np.float32)
        self.sradius = np.array([np.inf, 120.0, 100.0], np.float32)          # flat: every query probes partition 0


@pytest.fixture(scope="module")
def rdb(pyqadc):
    db = RangeDb(pyqadc)
    yield db
    db.idx.close()


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def range_scan_raw(pyqadc, db, tables_ptr):
    lims = np.zeros(NQ + 1, np.uint64)
    rc = pyqadc.lib().qadc_adc_range_scan_device(db.idx._h, NQ, MA, ASSIGN.ctypes.data_as(C.POINTER(C.c_int32)), tables_ptr, fp(db.radius), 1,
                                                 None, lims.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, lims


def range_search_raw(pyqadc, db, q_ptr):
    lims = np.zeros(NQ + 1, np.uint64)
    rc = pyqadc.lib().qadc_adc_range_search_device(db.idx._h, NQ, q_ptr, 1, fp(db.sradius), 2, 1, None, None,
                                                   lims.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, lims


def collect_cases(pyqadc, db, a, rows, align, backend, want):
    """capacity exact, 7 over and 1 short, from one held result, into fresh windows of the arena `a`"""
    L = pyqadc.lib()
    out = {}
    for name, cap in (("exact", rows), ("over", rows + 7), ("short", rows - 1)):
        k = a.place(np.empty(cap, np.uint32), al(align, 4), "out", name="keys (%s)" % name)
        v = a.place(np.empty(cap, np.float32), al(align, 4), "out", name="values (%s)" % name)
        a.snapshot()
        if backend == "torch":
            rc = L.qadc_adc_range_collect_device(db.idx._h, cap, a.ptr(k), a.ptr(v))
        else:
            rc = L.qadc_adc_range_collect(db.idx._h, cap, C.cast(a.ptr(k), C.POINTER(C.c_uint32)), C.cast(a.ptr(v), C.POINTER(C.c_float)))
        if name == "short":
            assert rc == pyqadc.QADC_E_CAPACITY
            a.check_untouched([])                                            # nothing is copied ...
        else:
            assert rc == 0, L.qadc_last_error()
            a.check_untouched([(k, rows), (v, rows)])                        # ... and the 7 trailing entries stay
            out[name + " keys"], out[name + " values"] = a.host(k)[:rows], a.host(v)[:rows]
            assert ga.same(dict(keys=out[name + " keys"], values=out[name + " values"]), want) is None, name
    rc, keys, vals = db.idx.range_collect_raw(rows)                          # ... and the result is still held
    assert rc == 0 and ga.same(dict(keys=keys[:rows], values=vals[:rows]), want) is None
    return out


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("form", ["scan", "search"])
def test_range_device_and_collect_device(pyqadc, rdb, form, align):
    db = rdb
    if form == "scan":
        wl, wk, wv = db.idx.range_scan(ASSIGN, db.tables, db.radius)
    else:
        wl, wk, wv = db.idx.range_search(db.queries, 1, db.sradius)
    rows = int(wl[-1])
    want = dict(keys=wk, values=wv)
    assert wl[1] - wl[0] > pyqadc.ADC_RANGE_SORT_LDS and 0 < wl[2] - wl[1] < 4096 and rows > 7

    def call(a):
        if form == "scan":
            t = a.place(db.tables, al(align, 16), "in", name="d_tables")
            a.snapshot()
            rc, lims = range_scan_raw(pyqadc, db, a.ptr(t))
        else:
            q = a.place(db.queries, al(align, 4), "in", name="d_queries")
            a.snapshot()
            rc, lims = range_search_raw(pyqadc, db, a.ptr(q))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([])                                                # the result is held on the index: no caller buffer is written
        assert np.array_equal(lims.astype(np.int64), wl)
        return collect_cases(pyqadc, db, a, rows, align, "torch", want)

    ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    if form == "scan":
        wrapper = db.idx.range_scan_device(ASSIGN, torch.from_numpy(db.tables).cuda(), db.radius)
        got = dict(keys=wrapper[1].cpu().numpy().view(np.uint32), values=wrapper[2].cpu().numpy())
        assert np.array_equal(wrapper[0], wl) and ga.same(got, want) is None


@path_independent
def test_range_calls_refuse_pointers_below_the_stated_alignment(pyqadc, rdb):
    db = rdb
    wl, wk, wv = db.idx.range_scan(ASSIGN, db.tables, db.radius)
    rows, want = int(wl[-1]), dict(keys=wk, values=wv)
    a = ga.Arena(ga.P1, backend="torch", capacity=1 << 20)
    t = a.place(db.tables, 4, "in", name="d_tables at 4 bytes")
    q = a.place(db.queries, 4, "in", name="d_queries")
    k = a.place(np.empty(rows, np.uint32), 4, "out", name="d_keys")
    v = a.place(np.empty(rows, np.float32), 4, "out", name="d_values")
    L = pyqadc.lib()
    a.snapshot()
    assert range_scan_raw(pyqadc, db, a.ptr(t))[0] == pyqadc.QADC_E_ARG and b"d_tables must be 16-byte aligned" in L.qadc_last_error()
    assert range_search_raw(pyqadc, db, a.ptr(q) + 2)[0] == pyqadc.QADC_E_ARG and b"aligned" in L.qadc_last_error()
    assert L.qadc_adc_range_collect_device(db.idx._h, rows, a.ptr(k) + 2, a.ptr(v)) == pyqadc.QADC_E_ARG
    assert L.qadc_adc_range_collect_device(db.idx._h, rows, a.ptr(k), a.ptr(v) + 2) == pyqadc.QADC_E_ARG
    a.check_untouched([])
    assert L.qadc_adc_range_collect_device(db.idx._h, rows, a.ptr(k), a.ptr(v)) == 0      # the refusals dropped nothing
    a.check_untouched([k, v])
    assert ga.same(dict(keys=a.host(k), values=a.host(v)), want) is None


# ---- host pointers with a capacity, on the numpy arena ----

@path_independent
@pytest.mark.parametrize("align", ALIGNS)
def test_range_collect_into_host_windows(pyqadc, rdb, align):
    db = rdb
    wl, wk, wv = db.idx.range_scan(ASSIGN, db.tables, db.radius)
    ga.under_both_poisons(lambda a: collect_cases(pyqadc, db, a, int(wl[-1]), align, "numpy", dict(keys=wk, values=wv)), capacity=2 << 20)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("form", ["query_scan", "search"])
def test_candidate_streams_into_host_windows(pyqadc, dbs, sdb, form, align):
    """qadc_adc_query_scan_candidates and qadc_adc_search_candidates with cand_capacity one short, exact and seven over"""
    L, R = pyqadc.lib(), 10
    if form == "query_scan":
        db, nq = dbs("8x8"), NQ
        wk, wv, wo = db.idx.query_scan_candidates(ASSIGN, db.tables, R)
    else:
        db, nq = sdb, sdb.nq
        wk, wv, wo, _ = db.idx.search_candidates(db.queries, db.ma, R)
    n = int(wo[-1])
    assert n > 7
    u32p, f32p, u64p, i32p = (C.POINTER(t) for t in (C.c_uint32, C.c_float, C.c_uint64, C.c_int32))

    def call(a):
        out = {}
        for name, cap in (("short", n - 1), ("exact", n), ("over", n + 7)):
            k = a.place(np.empty(cap, np.uint32), al(align, 4), "out", name="cand_keys (%s)" % name)
            v = a.place(np.empty(cap, np.float32), al(align, 4), "out", name="cand_vals (%s)" % name)
            o = a.place(np.empty(nq + 1, np.uint64), al(align, 8), "out", name="offsets (%s)" % name)
            ptrs = (cap, C.cast(a.ptr(k), u32p), C.cast(a.ptr(v), f32p), C.cast(a.ptr(o), u64p))
            a.snapshot()
            if form == "query_scan":
                rc = L.qadc_adc_query_scan_candidates(db.idx._h, nq, MA, ASSIGN.ctypes.data_as(i32p), fp(db.tables), R, 1, *ptrs)
            else:
                rc = L.qadc_adc_search_candidates(db.idx._h, nq, fp(db.queries), db.ma, R, 2, 1, *ptrs, None)
            if name == "short":
                assert rc == pyqadc.QADC_E_CAPACITY
                a.check_untouched([o])                                       # offsets is filled, offsets[nq] = the entries needed
            else:
                assert rc == 0, L.qadc_last_error()
                a.check_untouched([(k, n), (v, n), o])
                assert np.array_equal(a.host(k)[:n], wk) and np.array_equal(ga.bits(a.host(v)[:n]), ga.bits(wv))
                out[name + " keys"], out[name + " vals"] = a.host(k)[:n], a.host(v)[:n]
            assert np.array_equal(a.host(o), wo)
        return out

    ga.under_both_poisons(call, capacity=2 << 20)
