"""GPU: the 4-bit index's host forms with a capacity — qadc_query_scan_candidates, qadc_scan_i8_candidates and
qadc_query_scan_collect_candidates — writing into windows of a numpy guard-band arena (tests/guard_arena.py),
with cand_capacity one short, exact and seven over.

One short: QADC_E_CAPACITY, offsets filled with offsets[nq] = the entries needed, and not one byte of cand_keys / cand_vals /
cand_slots written; the collect form keeps its result.  Exact and over: the stream of the plain call, the tail behind it untouched.
Both guard poisons, every buffer at its element's alignment and at 256."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
from helpers import float_tables, path_independent, rand_codes, rand_qtables

pytestmark = pytest.mark.gpu

M, NQ, MA, R = 16, 3, 2, 10
ASSIGN = np.array([[0, 1], [1, 0], [1, 1]], np.int32)
PTR = {t: C.POINTER(t) for t in (C.c_uint32, C.c_int8, C.c_uint16, C.c_uint64, C.c_int32, C.c_float)}


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def db(pyqadc):
    rng = np.random.default_rng(16)
    idx = pyqadc.Index(M)
    idx.add_partitions([rand_codes(rng, 2001, M), rand_codes(rng, 1501, M)])
    idx.finalize(0.5)
    yield idx, float_tables(rng, NQ, MA, M), rand_qtables(rng, (NQ, MA), M, 7)         # (sums stay below the 127 of the sentinel)
    idx.close()


def p(a, t):
    return a.ctypes.data_as(PTR[t])


@path_independent
@pytest.mark.parametrize("align", ["min", 256])
@pytest.mark.parametrize("form", ["query_scan", "scan_i8", "collect"])
def test_candidate_streams_of_the_4bit_index_into_host_windows(pyqadc, db, form, align):
    idx, tables, qtables = db
    L = pyqadc.lib()
    if form == "query_scan":
        streams = idx.query_scan_candidates(ASSIGN, tables.copy(), R)["streams"]
    elif form == "scan_i8":
        streams = idx.scan_i8_candidates(ASSIGN, qtables, R)
    else:
        whole = idx.query_scan_shard_streams(ASSIGN, tables.copy(), R)
        streams = [(whole["keys"][a:b], whole["vals"][a:b]) for a, b in zip(whole["offsets"][:-1], whole["offsets"][1:])]
    wk, wv = np.concatenate([s[0] for s in streams]), np.concatenate([s[1] for s in streams])
    wo = np.concatenate([[0], np.cumsum([len(s[0]) for s in streams])]).astype(np.uint64)
    n = int(wo[-1])
    assert n > 7 and all(len(s[0]) for s in streams)
    status, qmin, qmax = np.zeros(NQ, np.int32), np.zeros(NQ, np.float32), np.zeros(NQ, np.float32)

    def call(a):
        out, held = {}, None
        for name, cap in (("short", n - 1), ("exact", n), ("over", n + 7)):
            k = a.place(np.empty(cap, np.uint32), 4 if align == "min" else align, "out", name="cand_keys (%s)" % name)
            v = a.place(np.empty(cap, np.int8), 1 if align == "min" else align, "out", name="cand_vals (%s)" % name)
            s = a.place(np.empty(cap, np.uint16), 2 if align == "min" else align, "out", name="cand_slots (%s)" % name)
            o = a.place(np.empty(NQ + 1, np.uint64), 8 if align == "min" else align, "out", name="offsets (%s)" % name)
            ptrs = (cap, C.cast(a.ptr(k), PTR[C.c_uint32]), C.cast(a.ptr(v), PTR[C.c_int8]))
            off = C.cast(a.ptr(o), PTR[C.c_uint64])
            written = [(k, n), (v, n), o]
            if form == "collect" and name != "exact":                        # (a short call keeps the result: the exact one collects it)
                held = idx.submit(0, ASSIGN, tables.copy(), R) or idx._pending.pop(0)   # (its tables stay alive until the collect)
            a.snapshot()
            if form == "query_scan":
                t = tables.copy()
                rc = L.qadc_query_scan_candidates(idx._h, NQ, MA, p(ASSIGN, C.c_int32), p(t, C.c_float), R, *ptrs, off, p(status, C.c_int32),
                                                  p(qmin, C.c_float), p(qmax, C.c_float))
            elif form == "scan_i8":
                rc = L.qadc_scan_i8_candidates(idx._h, NQ, MA, p(ASSIGN, C.c_int32), p(qtables, C.c_int8), R, *ptrs, off)
            else:
                rc = L.qadc_query_scan_collect_candidates(idx._h, 0, *ptrs, C.cast(a.ptr(s), PTR[C.c_uint16]), off, p(status, C.c_int32),
                                                          p(qmin, C.c_float), p(qmax, C.c_float))
                written.append((s, n))
            if name == "short":
                assert rc == pyqadc.QADC_E_CAPACITY
                a.check_untouched([o])
            else:
                assert rc == 0, L.qadc_last_error()
                a.check_untouched(written)
                assert np.array_equal(a.host(k)[:n], wk) and np.array_equal(a.host(v)[:n], wv)
                out[name + " keys"], out[name + " vals"] = a.host(k)[:n], a.host(v)[:n]
                if form == "collect":
                    out[name + " slots"] = a.host(s)[:n]
                    assert np.array_equal(out[name + " slots"], whole["slots"])
            assert np.array_equal(a.host(o), wo) and (status == 0).all()
        del held
        return out

    ga.under_both_poisons(call, capacity=2 << 20)
