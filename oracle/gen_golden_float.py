"""TEST INFRASTRUCTURE — generates tests/golden/ref_query_scan_cases.npz: fixtures for the float -> int8 boundary of
scanner_4::query_scan (db_query_4.cpp:230-309), every output produced by the REFERENCE'S OWN CODE as compiled here:

    oracle/_ref/libqadc_ref_float.so   scanner_4 (whole), QuantizerMAX, scan_4 — line ranges of the reference's files
                                       (oracle/ref_extract.sh, oracle/ref_float_harness.cpp)
    oracle/_ref/libqadc_ref.so         scan_avx_4 + kv_binheap (oracle/ref_harness.cpp)

Run in the build container only:   make -C oracle && python oracle/gen_golden_float.py
(it also writes tests/golden/ref_query_scan_nonfinite_cases.npz: see main_nonfinite.  QADC_GOLDEN_OUT names the first file; the
second goes beside it.)

Per case the file holds the inputs (the database it runs on — row-major partitions, or the seed of the counter-based
generator for the larger flat ones —, labels, keep, R, assign, float tables BEFORE the in-place clamp) and the
reference's results:
    exit     exit status of query_scan in a child process (1 = "Max quantization bound too high", db_query_4.cpp:271-274)
    starts   scanner_4::starts_sizes of the probed partitions (prepare_database, db_query_4.cpp:125-126)
    qmax     tmp_bh.max() after scanner_4::query_scan_start (230-242, 259)
    qmin     min of all tables clamped at 0 (258-263) — a comparison, no arithmetic: evaluated here in numpy
    qt       QuantizerMAX<int8_t>(qmin, qmax).quantize_tables of the CLAMPED tables (277-284)        [exit == 0]
    keys / vals / sorted   the int8 heap after the WHOLE scanner_4::query_scan, and sort_keys of it   [exit == 0]
and, as a cross-check made at generation time, the heap from scan_avx_4 fed with `qt` equals keys / vals.
Four small cases also carry per-code arrays: `fcand` = scan_4's float sum of every start code (read out of a float heap
with room for all of them) and `cand` = scan_avx_4's int8 value of every code of the first probed partition (read out
of an int8 heap with room for all; codes the scan never pushes have cand = 127).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyoracle as po  # noqa: E402

OUT = os.environ.get("QADC_GOLDEN_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                        "ref_query_scan_cases.npz")
# the second fixture (NaN / infinite / FLT_MAX tables, see main_nonfinite) is written beside the first, under its own name
NF_OUT = os.path.join(os.path.dirname(OUT), "ref_query_scan_nonfinite_cases.npz")
OUT = os.path.join(os.path.dirname(OUT), "ref_query_scan_cases.npz")


def dist_tables(rng, ma, M, scale=1.0, negatives=0.0, levels=0):
    """[ma][M*16] float32 distance-table-like values; `negatives` = fraction of slightly negative entries (what the BLAS
    expansion form produces); `levels` > 0 = that many distinct values only (ties everywhere)."""
    d = 8
    q = rng.normal(size=(ma, M, 1, d)).astype(np.float32)
    c = rng.normal(size=(1, M, 16, d)).astype(np.float32)
    t = ((q - c) ** 2).sum(-1).astype(np.float32) * np.float32(scale)
    if levels:
        t = (np.floor(t / t.max() * levels) * np.float32(scale / levels)).astype(np.float32)
    if negatives:
        neg = rng.random(t.shape) < negatives
        t = np.where(neg, -np.float32(0.03 * scale) * rng.random(t.shape).astype(np.float32), t).astype(np.float32)
    return np.ascontiguousarray(t.reshape(ma, M * 16), np.float32)


def synth_codes(n, M, seed):
    cs = M // 2
    return po.fill_codes(0, (n * cs + 7) // 8, seed)[:n * cs].reshape(n, cs).copy()


def main():
    assert po.have_ref() and po.have_ref_float(), "build oracle/_ref first (make -C oracle)"
    rng = np.random.default_rng(20175)
    d, cases = {}, []

    dbs = []

    def store_db(parts, labels, synth=None):
        """-> database id; partitions are stored once however many cases query them (synth = (n, seed): only that)."""
        dbi = len(dbs)
        if synth is not None:
            d["db%d_synth" % dbi] = np.array(synth, np.int64)
        else:
            for i, p in enumerate(parts):
                d["db%d_codes%d" % (dbi, i)] = np.ascontiguousarray(p, np.uint8)
        if labels is not None:
            for i, l in enumerate(labels):
                d["db%d_labels%d" % (dbi, i)] = np.ascontiguousarray(l, np.uint32)
        dbs.append((len(parts), int(labels is not None), int(synth is not None)))
        return dbi

    def add(M, parts, labels, keep, R, assign, tables, per_code=False, dbi=None, synth=None):
        cid = "q%02d" % len(cases)
        if dbi is None:
            dbi = store_db(parts, labels, synth)
        assign = np.asarray(assign, np.int32)
        ma = len(assign)
        tables = np.ascontiguousarray(tables, np.float32).reshape(ma, M * 16)
        sc = po.RefScanner4(M, parts, labels, keep)
        starts, psizes, has_labels = sc.sizes()
        assert has_labels == (labels is not None)
        fk, fv = sc.query_start(assign, tables, R)
        qmax = fv[0]
        qmin = np.float32(0) if tables.min() < 0 else tables.min()
        clamped = np.where(tables < 0, np.float32(0), tables).astype(np.float32)
        code = sc.try_query(assign, tables, R)
        assert code == (1 if float(qmax) > 1e30 else 0), (cid, code, qmax)
        d[cid + "_assign"] = assign
        d[cid + "_tables"] = tables.copy()
        d[cid + "_exit"] = np.array(code)
        d[cid + "_starts"] = starts[assign].copy()
        d[cid + "_qmax"] = np.array(qmax, np.float32)
        d[cid + "_qmin"] = np.array(qmin, np.float32)
        if code == 0:
            qt = po.reff_quantize_tables(clamped.reshape(ma, M, 16), float(qmin), float(qmax))
            tb = tables.copy()
            keys, vals, skeys = sc.query_scan(assign, tb, R, want_sorted=True)
            assert np.array_equal(tb, clamped), cid                    # the in-place clamp (262-269)
            # cross-check: the integer half alone (scan_avx_4 + kv_binheap of libqadc_ref.so) on those int8 tables
            live = [a for a in range(ma) if parts[assign[a]].shape[0] > 0]
            k2, v2 = po.ref_scan(M, [parts[assign[a]] for a in live],
                                 None if labels is None else [labels[assign[a]] for a in live], qt[live], R)
            assert np.array_equal(k2, keys) and np.array_equal(v2, vals), cid
            d[cid + "_qt"], d[cid + "_keys"], d[cid + "_vals"], d[cid + "_sorted"] = qt, keys, vals, skeys
            if per_code:
                p0 = parts[assign[0]]
                n0, s0 = p0.shape[0], int(starts[assign[0]])
                pk, pv = po.reff_scan4_start(M, [p0[:s0]], None, tables[:1], s0 + 2)       # room for all: nothing evicted
                fc = np.full(s0, np.nan, np.float32)
                fc[pk[1:]] = pv[1:]                                    # (entry 0 is the (0, FLT_MAX) seed, never moved: it is the max)
                assert pk[0] == 0 and pv[0] == np.finfo(np.float32).max and not np.isnan(fc).any(), cid
                d[cid + "_fcand"] = fc
                ck, cv = po.ref_scan(M, [p0], None, qt[:1], n0 + 32)   # room for all, incl. the padding lanes' replays
                cand = np.full(n0, 127, np.int8)
                cand[ck[1:]] = cv[1:]
                d[cid + "_cand"] = cand
        cases.append((cid, M, R, dbi, int(labels is not None), int(per_code), float(keep)))
        sc.close()

    def codes(n, M):
        return rng.integers(0, 256, (n, M // 2), dtype=np.uint8)

    R = 100
    # ---- flat: scales, negatives, ties; per-code arrays on the small ones ------------------------------------------
    for M in (16, 32):
        add(M, [codes(1800, M)], None, 0.08, R, [0], dist_tables(rng, 1, M), per_code=True)
        add(M, [codes(2101, M)], None, 0.06, R, [0], dist_tables(rng, 1, M, negatives=0.03), per_code=True)
        add(M, [synth_codes(40003, M, 21 + M)], None, 0.01, R, [0], dist_tables(rng, 1, M, scale=1000.0), synth=(40003, 21 + M))
        add(M, [synth_codes(30000, M, 22 + M)], None, 0.01, R, [0], dist_tables(rng, 1, M, scale=1e-3, negatives=0.01),
            synth=(30000, 22 + M))
        add(M, [synth_codes(9000, M, 23 + M)], None, 0.05, R, [0], dist_tables(rng, 1, M, levels=6), synth=(9000, 23 + M))
    # ---- start sizes 1 ... R + 50 around the "heap not full -> FLT_MAX -> exit" edge (db_query_4.cpp:271-274) -----
    for s in (1, R - 1, R, R + 1, R + 50):
        n = 1000
        add(16, [codes(n, 16)], None, (s + 0.5) / n, R, [0], dist_tables(rng, 1, 16))
    add(16, [codes(900, 16)], None, 0.5, 1000, [0], dist_tables(rng, 1, 16))          # R > N
    add(16, [codes(5000, 16)], None, 0.05, 10, [0], dist_tables(rng, 1, 16, negatives=0.02))   # small R
    # ---- IVF: labels, one (qmin, qmax) for all probes, ragged sizes, an empty probed partition ----------------------
    for M, keep in ((16, 0.05), (32, 0.04), (16, 0.02)):
        sizes = [3333, 17, 0, 2048, 1, 4999, 777, 1600]
        parts = [codes(s, M) for s in sizes]
        perm = rng.permutation(sum(sizes)).astype(np.uint32) + 11
        labels = list(np.split(perm, np.cumsum(sizes)[:-1]))
        dbi = store_db(parts, labels)
        for assign in ([5, 0, 3, 7], [2, 1, 4, 6, 0], [7, 6, 5, 4, 3, 2, 1, 0]):
            add(M, parts, labels, keep, R, assign, dist_tables(rng, len(assign), M, negatives=0.02 if M == 16 else 0.0), dbi=dbi)
    d["cases"] = np.array([c[0] for c in cases])
    d["case_meta"] = np.array([c[1:6] for c in cases], np.int64)          # M, R, database id, has_labels, per_code
    d["db_meta"] = np.array(dbs, np.int64)                                # nparts, has_labels, synthetic
    d["case_keep"] = np.array([c[6] for c in cases], np.float32)
    np.savez_compressed(OUT, **d)
    nexit = sum(int(d[c[0] + "_exit"]) for c in cases)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(cases), "query_scan cases,", nexit, "of them exit(1)")


def f32_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


NAN_POS, NAN_NEG = 0x7fc00000, 0xffc00000
INF_POS, INF_NEG = 0x7f800000, 0xff800000
FMAX_POS, FMAX_NEG = 0x7f7fffff, 0xff7fffff


def main_nonfinite():
    """tests/golden/ref_query_scan_nonfinite_cases.npz: scanner_4::query_scan of the reference build on tables that hold NaN of
    both signs, +-inf and +-FLT_MAX.  Inputs (tables as uint32 bit patterns: NaN signs and payloads are part of the input) and
    the reference's outputs only:
        exit                       exit status of query_scan in a child process
        start_keys / start_vals    the float heap after scanner_4::query_scan_start (values as bits; qmax = vals[0])
        keys / vals / sorted       the int8 heap after the whole query_scan and its sort_keys                    [exit == 0]
        after                      the caller's tables after the call, as bits (the in-place clamp, 262-269)      [exit == 0]
    The reference keeps qmin and its int8 tables to itself: they are pinned through the final heap.
    Databases: one flat partition of 20 000 generated codes per M (only the seed is stored), keep 0.05, and one small
    labelled IVF database shared by its cases."""
    assert po.have_ref() and po.have_ref_float(), "build oracle/_ref first (make -C oracle)"
    rng = np.random.default_rng(20176)
    d, cases, dbs = {}, [], []

    def store_db(M, parts, labels, synth=None):
        dbi = len(dbs)
        if synth is not None:
            d["db%d_synth" % dbi] = np.array(synth, np.int64)
        else:
            for i, p in enumerate(parts):
                d["db%d_codes%d" % (dbi, i)] = np.ascontiguousarray(p, np.uint8)
        if labels is not None:
            for i, l in enumerate(labels):
                d["db%d_labels%d" % (dbi, i)] = np.ascontiguousarray(l, np.uint32)
        dbs.append((len(parts), int(labels is not None), int(synth is not None)))
        return dict(dbi=dbi, M=M, parts=parts, labels=labels)

    def add(db, keep, R, assign, tables, family):
        cid = "n%02d" % len(cases)
        M, parts, labels = db["M"], db["parts"], db["labels"]
        assign = np.asarray(assign, np.int32)
        ma = len(assign)
        tables = np.ascontiguousarray(tables, np.float32).reshape(ma, M * 16)
        sc = po.RefScanner4(M, parts, labels, keep)
        fk, fv = sc.query_start(assign, tables.copy(), R)
        code = sc.try_query(assign, tables, R)
        assert code == (1 if float(fv[0]) > 1e30 else 0), (cid, code, fv[0])
        assert not np.isnan(fv).any(), cid                        # (the binary never pushes a NaN candidate)
        d[cid + "_assign"] = assign
        d[cid + "_tables"] = tables.view(np.uint32).copy()
        d[cid + "_exit"] = np.array(code)
        d[cid + "_start_keys"], d[cid + "_start_vals"] = fk, fv.view(np.uint32).copy()
        if code == 0:
            tb = tables.copy()
            keys, vals, skeys = sc.query_scan(assign, tb, R, want_sorted=True)
            d[cid + "_keys"], d[cid + "_vals"], d[cid + "_sorted"] = keys, vals, skeys
            d[cid + "_after"] = tb.view(np.uint32).copy()
        cases.append((cid, M, R, db["dbi"], int(labels is not None), float(keep), family))
        sc.close()

    def put(t, where, bits):
        t = t.copy()
        flat = t.reshape(-1)
        for i, w in enumerate(np.atleast_1d(where)):
            flat[int(w)] = f32_bits(bits[i % len(bits)] if isinstance(bits, (tuple, list)) else bits)
        return t

    def pushed(db, keep, tables):
        """how many start candidates of partition 0 the reference's float heap takes (cand < FLT_MAX): read off a heap with room for all"""
        s0 = po.start_size(db["parts"][0].shape[0], keep)
        pk, pv = po.reff_scan4_start(db["M"], [db["parts"][0][:s0]], None, tables.reshape(1, -1), s0 + 2)
        return len(pk) - 1

    def tune(db, keep, base, extra_rows, bits, targets):
        """tables = base + a few more entries of `bits` in random rows >= extra_rows[0], one table per target count of pushed starts"""
        M, found = db["M"], {}
        for _ in range(20000):
            k = int(rng.integers(0, 7))
            where = [int(rng.integers(extra_rows[0], extra_rows[1])) * 16 + int(rng.integers(0, 16)) for _ in range(k)]
            t = put(base, where, bits) if k else base.copy()
            c = pushed(db, keep, t)
            if c in targets and c not in found:
                found[c] = t
                if len(found) == len(targets):
                    break
        assert len(found) == len(targets), sorted(found)
        return [found[c] for c in targets]

    keep, R, n = np.float32(0.05), 100, 20000
    flat = {M: store_db(M, [synth_codes(n, M, 61 + M)], None, synth=(n, 61 + M)) for M in (16, 32)}
    for M in (16, 32):
        db, last = flat[M], M * 16 - 1
        base = dist_tables(rng, 1, M)
        negs = dist_tables(rng, 1, M, negatives=0.03)
        amin = int(np.argmin(base))
        spots = (("first", 0), ("middle", 87), ("row_end", 63), ("table_end", last), ("argmin", amin)) if M == 16 else \
                (("first", 0), ("table_end", last), ("argmin", amin))
        for name, at in spots:                                     # one NaN of each sign
            for sign, bits in (("pos", NAN_POS), ("neg", NAN_NEG)):
                add(db, keep, R, [0], put(base, at, bits), "nan_%s_%s" % (name, sign))
        add(db, keep, R, [0], put(base, np.arange(48, 64), (NAN_POS, NAN_NEG)), "nan_row")
        add(db, keep, R, [0], put(negs, last - 1, NAN_NEG), "nan_tail_negatives")          # a NaN qmin: nothing is clamped
        add(db, keep, R, [0], put(np.round(base * 2) / 2, 130, NAN_POS), "nan_ties")
        if M == 16:
            add(db, keep, R, [0], put(base, rng.choice(M * 16 - 3, 12, replace=False), (NAN_POS, NAN_NEG, 0x7fffffff, 0xffffffff)), "nan_sparse")
            add(db, keep, R, [0], put(negs, 87, NAN_POS), "nan_middle_negatives")           # qmin < 0: the clamp runs, the NaN keeps its bits
            add(db, keep, 1, [0], put(base, 87, NAN_NEG), "nan_middle_R1")
            for name, bits in (("pinf", INF_POS), ("ninf", INF_NEG), ("pfmax", FMAX_POS), ("nfmax", FMAX_NEG)):
                add(db, keep, R, [0], put(base, 87, bits), name + "_middle")
            add(db, keep, R, [0], put(base, np.arange(32, 48), INF_POS), "pinf_row")
            add(db, keep, R, [0], put(base, rng.choice(M * 16, 12, replace=False), (INF_NEG, FMAX_NEG)), "ninf_nfmax_sparse")
            add(db, keep, R, [0], put(put(base, np.arange(32, 40), INF_POS), np.arange(80, 86), INF_NEG), "inf_minus_inf_sums")
            add(db, keep, R, [0], put(base, np.arange(M * 16), (NAN_POS, NAN_NEG)), "all_nan")
            add(db, keep, R, [0], put(base, np.arange(M * 16), INF_POS), "all_pinf")
            add(db, keep, R, [0], put(base, np.arange(M * 16), INF_NEG), "all_ninf")
            # NaN sums on either side of starts - R: 14 of row 0's 16 entries NaN, then single entries until 101 / 100 / 99 starts are left
            coarse = put(base, np.arange(14), (NAN_POS, NAN_NEG))
            for c, t in zip((101, 100, 99), tune(db, keep, coarse, (1, M), (NAN_NEG, NAN_POS), (101, 100, 99))):
                add(db, keep, R, [0], t, "nan_sums_leave_%d" % c)
        else:
            # the same edge made by +inf and -inf: +inf alone is not pushed either, -inf alone is, both give a NaN sum
            coarse = put(put(base, [r * 16 + e for r in (2, 3, 4) for e in range(8)], INF_POS), np.arange(80, 84), INF_NEG)
            for c, t in zip((101, 100, 99), tune(db, keep, coarse, (6, M), INF_POS, (101, 100, 99))):
                add(db, keep, R, [0], t, "inf_sums_leave_%d" % c)
    # IVF, ma = 4: the NaN sits in one probe's table only; qmin spans all four tables
    M, sizes = 16, [3000, 2500, 1, 3500, 900]
    parts = [rng.integers(0, 256, (s, M // 2), dtype=np.uint8) for s in sizes]
    perm = rng.permutation(sum(sizes)).astype(np.uint32) + 7
    ivf = store_db(M, parts, list(np.split(perm, np.cumsum(sizes)[:-1])))
    tb4 = dist_tables(rng, 4, M, negatives=0.01)
    add(ivf, keep, R, [3, 0, 2, 1], put(tb4, 2 * 256 + 87, NAN_NEG), "ivf_nan_probe2")
    add(ivf, keep, R, [1, 4, 0, 3], put(tb4, 4 * 256 - 1, NAN_POS), "ivf_nan_table_end")
    d["cases"] = np.array([c[0] for c in cases])
    d["case_meta"] = np.array([c[1:5] for c in cases], np.int64)          # M, R, database id, has_labels
    d["case_keep"] = np.array([c[5] for c in cases], np.float32)
    d["case_family"] = np.array([c[6] for c in cases])
    d["db_meta"] = np.array(dbs, np.int64)                                # nparts, has_labels, synthetic
    np.savez_compressed(NF_OUT, **d)
    nexit = sum(int(d[c[0] + "_exit"]) for c in cases)
    print("wrote", NF_OUT, os.path.getsize(NF_OUT), "bytes,", len(cases), "non-finite query_scan cases,", nexit, "of them exit(1)")


if __name__ == "__main__":
    main()
    main_nonfinite()
