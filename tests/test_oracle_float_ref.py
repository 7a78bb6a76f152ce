"""CPU: the FLOAT half of the oracle (oracle/qadc_oracle.c: scan_4's sum, QuantizerMAX, the query_scan glue, start sizes,
the direct table form, scan_standard, the 4-bit packer) against

  * tests/golden/ref_query_scan_cases.npz — outputs of the reference's own scanner_4 / QuantizerMAX / scan_4 / scan_avx_4
    as compiled by oracle/Makefile (generator: oracle/gen_golden_float.py); runs everywhere, and
  * the live build oracle/_ref/libqadc_ref_float.so (line ranges of the reference's files compiled with its flags,
    oracle/ref_extract.sh + oracle/ref_float_harness.cpp) on seeded random inputs; skipped where that build is absent.

SURVEY.md section 8 rows A5 / A6 / A7 / A8 / A10 (direct form) and (c).  Everything compared is bit-exact: float heaps entry by
entry (so qmax = values[0]), int8 tables, int8 heaps, start sizes, exit statuses."""
import numpy as np
import pytest

import golden_cases
from helpers import rand_codes

FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def g():
    return golden_cases.load_query_scan()


PINNED_GXX = "11.4.0"      # the groupings of the float sums were read off THIS compiler's build of the reference (-O3 -ffast-math -mavx2 -mfma)


def _need_ref_float(po):
    if not po.have_ref_float():
        pytest.skip("oracle/_ref/libqadc_ref_float.so not built (no /root/reference here)")
    import os
    import subprocess
    if os.path.isdir("/root/reference"):                        # (a live build: made by the local g++; the GPU box runs the prebuilt file)
        v = subprocess.run(["g++", "-dumpfullversion"], stdout=subprocess.PIPE).stdout.decode().strip()
        if v != PINNED_GXX:
            pytest.skip("oracle/_ref was built by g++ %s; the as-compiled groupings (sum_mode / quant_mode / div_mode 1) are pinned to g++ %s: "
                        "another compiler may group the reference's -ffast-math sums differently — not a failure of this repository" % (v, PINNED_GXX))


def rand_tables(rng, ma, M, negatives=False):
    """[ma][M*16] float32: squared distances of N(0,1) sub-vectors at a random scale, optionally a few small negatives."""
    q = rng.normal(size=(ma, M, 1, 8)).astype(np.float32)
    c = rng.normal(size=(1, M, 16, 8)).astype(np.float32)
    t = ((q - c) ** 2).sum(-1).astype(np.float32) * np.float32(rng.choice([1e-3, 1.0, 1.0, 37.5, 1e4]))
    if negatives:
        t = np.where(rng.random(t.shape) < 0.02, -np.float32(0.01) * t, t).astype(np.float32)
    return np.ascontiguousarray(t.reshape(ma, M * 16), np.float32)


# ------------------------------------------------------------------------------------------------ golden (runs everywhere)
def test_query_scan_matches_reference_golden(po, g):
    n = nexit = 0
    for c in golden_cases.query_scan_cases(g, po):
        M, R, assign = c["M"], c["R"], c["assign"]
        for a, p in enumerate(assign):
            assert po.start_size(c["parts"][p].shape[0], c["keep"]) == c["starts"][a], c["cid"]
        tb = c["tables"].copy()
        o = po.query_scan(M, c["parts"], c["labels"], c["keep"], assign, tb, R)
        assert o["rc"] == c["exit"], c["cid"]
        assert np.float32(o["qmax"]) == c["qmax"] and np.float32(o["qmin"]) == c["qmin"], c["cid"]
        if c["exit"]:
            nexit += 1
            continue
        assert np.array_equal(o["qtables"], c["qt"]), c["cid"]
        assert np.array_equal(o["keys"], c["keys"]) and np.array_equal(o["values"], c["vals"]), c["cid"]
        assert np.array_equal(po.sort_keys_i8(o["keys"], o["values"]), c["sorted"]), c["cid"]
        assert np.array_equal(tb, np.where(c["tables"] < 0, np.float32(0), c["tables"])), c["cid"]   # the in-place clamp
        if "fcand" in c:
            p0 = c["parts"][assign[0]]
            assert np.array_equal(po.candidates_f32(M, p0[:c["starts"][0]], c["tables"][0]), c["fcand"]), c["cid"]
            assert np.array_equal(po.candidates_i8(M, p0, c["qt"][0]), c["cand"]), c["cid"]
        n += 1
    assert n >= 20 and nexit >= 3


def test_source_order_sum_is_not_what_the_reference_binary_computes(po, g):
    """The pin is not vacuous: scan_4's sum in SOURCE order (sum_mode 0) disagrees with the reference as compiled on these
    fixtures (its -ffast-math re-associates the sum) — in the per-code values and in qmax."""
    dcand = dqmax = 0
    for c in golden_cases.query_scan_cases(g, po):
        if "fcand" in c:
            p0 = c["parts"][c["assign"][0]]
            seq = po.candidates_f32(c["M"], p0[:c["starts"][0]], c["tables"][0], sum_mode=0)
            dcand += int((seq != c["fcand"]).sum())
        if c["exit"] == 0:
            o = po.query_scan(c["M"], c["parts"], c["labels"], c["keep"], c["assign"], c["tables"].copy(), c["R"], sum_mode=0)
            dqmax += int(np.float32(o["qmax"]) != c["qmax"])
    assert dcand > 0 and dqmax > 0


# ------------------------------------------------------------------------------------------------ live reference build
@pytest.mark.parametrize("M", [16, 32])
def test_scan4_start_heap_matches_the_reference_as_compiled(po, M):
    """A7: push(0, FLT_MAX) + scan_4<M> over 1..4 runs, each with its own table: the WHOLE float heap, entry by entry."""
    _need_ref_float(po)
    rng = np.random.default_rng(700 + M)
    for t in range(400):
        nparts = int(rng.integers(1, 5))
        parts = [rand_codes(rng, int(rng.integers(1, 3000)), M) for _ in range(nparts)]
        labels = None
        if t % 3 == 0:
            labels = [rng.integers(0, 2 ** 32, p.shape[0], dtype=np.uint64).astype(np.uint32) for p in parts]
        tables = rand_tables(rng, nparts, M, negatives=(t % 4 == 1))
        R = int(rng.choice([1, 10, 100, 1000]))
        rk, rv = po.reff_scan4_start(M, parts, labels, tables, R)
        ok, ov = po.scan4_start(M, parts, labels, tables, R)
        assert np.array_equal(rk, ok) and np.array_equal(rv, ov), t


def test_quantizer_matches_the_reference_as_compiled(po):
    """A5: QuantizerMAX<int8_t>::quantize_tables on 1.6 M entries: random, exactly on bucket edges (k * delta + qmin and its
    float neighbours), at / above qmax, and with qmin > 0."""
    _need_ref_float(po)
    rng = np.random.default_rng(55)
    total = 0
    for t in range(100):
        qmin = np.float32(0) if t % 2 == 0 else np.float32(rng.random() * 3)
        qmax = np.float32(qmin + np.float32(rng.choice([1e-3, 0.5, 7.25, 127.0, 3e4])) * np.float32(0.5 + rng.random()))
        vals = (qmin + rng.random(16000).astype(np.float32) * np.float32(1.1) * (qmax - qmin)).astype(np.float32)
        k = rng.integers(0, 128, 4000).astype(np.float32)
        edge = (qmin + k * ((qmax - qmin) / np.float32(127))).astype(np.float32)
        edges = np.concatenate([edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))])
        edges = np.maximum(edges, qmin).astype(np.float32)       # the caller never hands values below qmin (it is the min)
        allv = np.concatenate([vals, edges[:15984], np.array([qmax, np.nextafter(qmax, np.float32(0)), qmin] * 5 + [qmax], np.float32)])
        allv = np.ascontiguousarray(allv[:(allv.size // 16) * 16].reshape(-1, 16))
        want = po.reff_quantize_tables(allv, float(qmin), float(qmax))
        got = po.quantize_tables(allv, float(qmin), float(qmax), mode=1)
        assert np.array_equal(want, got), t
        assert want.min() >= 0
        total += allv.size
    assert total >= 1_500_000


@pytest.mark.parametrize("M", [16, 32])
def test_query_scan_whole_matches_the_reference_as_compiled(po, M):
    """A6 / A8: the reference's scanner_4, WHOLE (prepare_database + query_scan as compiled), against orc_query_scan on
    5 000 random queries per M — flat and IVF with labels, keep 1 % / 0.2 % / larger, ragged and empty partitions, negative
    table entries: start sizes, qmax (the float heap of query_scan_start), int8 tables (QuantizerMAX of the build on the
    clamped tables) and the final int8 heap."""
    _need_ref_float(po)
    rng = np.random.default_rng(9100 + M)
    nq = 0
    for db in range(20):
        ivf = db % 2 == 1
        if ivf:
            K = int(rng.integers(4, 12))
            sizes = [int(s) for s in rng.integers(0, 9000, K)]
            sizes[int(rng.integers(1, K))] = 0                       # (an empty partition 0 is refused: see the exit paths' test)
            sizes[0] = max(sizes[0], 1)
            keep = np.float32(rng.choice([0.01, 0.02, 0.05]))
            perm = rng.permutation(sum(sizes)).astype(np.uint32) + 3
            labels = list(np.split(perm, np.cumsum(sizes)[:-1]))
        else:
            sizes = [int(rng.integers(20000, 70000))]
            keep = np.float32(rng.choice([0.01, 0.002 if sizes[0] > 55000 else 0.01, 0.1]))
            labels = None
        parts = [rand_codes(rng, s, M) for s in sizes]
        sc = po.RefScanner4(M, parts, labels, keep)
        starts, psizes, has_labels = sc.sizes()
        assert list(psizes) == sizes and has_labels == ivf
        assert [po.start_size(s, keep) for s in sizes] == list(starts)
        for q in range(250):
            ma = int(rng.integers(2, min(8, len(sizes)) + 1)) if ivf else 1
            assign = rng.permutation(len(sizes))[:ma].astype(np.int32)
            R = 100 if q % 5 else int(rng.choice([10, 50, 100]))
            if int(starts[assign].sum()) < R:
                continue                                             # qmax = FLT_MAX: the exit path has its own test
            tables = rand_tables(rng, ma, M, negatives=(q % 3 == 0))
            fk, fv = sc.query_start(assign, tables, R)
            assert fv[0] < FMAX
            want = po.query_scan(M, parts, labels, keep, assign, tables.copy(), R)
            assert want["rc"] == 0 and np.float32(want["qmax"]) == fv[0], (db, q)
            tb = tables.copy()
            hk, hv = sc.query_scan(assign, tb, R)
            assert np.array_equal(hk, want["keys"]) and np.array_equal(hv, want["values"]), (db, q)
            if q % 10 == 0:
                qt = po.reff_quantize_tables(tb.reshape(ma, M, 16), want["qmin"], float(fv[0]))
                assert np.array_equal(qt, want["qtables"]), (db, q)
            nq += 1
        sc.close()
    assert nq >= 4500


# ---- NaN, +-inf and +-FLT_MAX tables: the float front as the reference BUILD runs it (oracle/qadc_oracle.c: orc_min_element_compiled,
# orc_quantize_tables; the start scan needs no special rule: cand < top never holds for a NaN)
def _bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


NF_NAN = (0x7fc00000, 0xffc00000)
NF_VALUES = NF_NAN + (0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7fffffff, 0xffffffff)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _aligned_copy(tables, offset_floats):
    """A C-contiguous copy of `tables` that starts `offset_floats` floats past a 64-byte boundary."""
    buf = np.zeros(tables.size + 32, np.float32)
    first = (-(buf.ctypes.data // 4)) % 16 + offset_floats
    out = buf[first:first + tables.size].reshape(tables.shape)
    out[...] = tables
    assert out.flags.c_contiguous and (out.ctypes.data // 4) % 16 == offset_floats % 16
    return out


def _check_whole_against_reference(po, sc, M, parts, labels, keep, assign, tables, R, tag, may_exit=False, offset=0):
    """start heap, exit status, final heap, in-place clamp (as bits) of the reference build == the oracle's; the build's own
    QuantizerMAX instance on the clamped tables with the oracle's (qmin, qmax) == the oracle's int8 tables."""
    starts = [parts[p][:po.start_size(parts[p].shape[0], keep)] for p in assign]
    fk, fv = sc.query_start(assign, tables, R)
    ok, ov = po.scan4_start(M, starts, None if labels is None else [labels[p][:len(s)] for p, s in zip(assign, starts)], tables, R)
    assert np.array_equal(fk, ok) and _same_bits(fv, ov), tag
    assert not np.isnan(fv).any(), tag                            # the binary never pushes a NaN candidate
    ot = _aligned_copy(tables, offset)
    want = po.query_scan(M, parts, labels, keep, assign, ot, R)
    assert want["qmax_bits"] == int(fv[:1].view(np.uint32)[0]), tag
    code = sc.try_query(assign, tables, R) if may_exit else 0
    assert (float(fv[0]) > 1e30) == bool(code) if may_exit else float(fv[0]) <= 1e30, tag
    assert want["rc"] == code, tag
    if code:
        return want
    rt = _aligned_copy(tables, offset)
    hk, hv = sc.query_scan(assign, rt, R)
    assert np.array_equal(hk, want["keys"]) and np.array_equal(hv, want["values"]), tag
    assert _same_bits(rt, ot), tag                                # the clamp: negatives to +0 only when qmin < 0, NaN bits kept
    qt = po.reff_quantize_tables(rt.reshape(len(assign), M, 16), _bits(want["qmin_bits"]), fv[0])
    assert np.array_equal(qt, want["qtables"]), tag
    return want


@pytest.mark.parametrize("M", [16, 32])
def test_one_nan_at_every_table_entry_matches_the_reference_as_compiled(po, M):
    """One NaN swept over EVERY entry of the tables, ma = 1 and 3, both NaN signs, with and without negative entries, the tables at
    two alignments (the build's min reduction uses unaligned loads and has no peel: orc_min_element_compiled is a function of the
    values alone).  The NaN's position decides qmin — a lane of the reduction forgets what it saw before a NaN, a NaN in the last
    entry IS qmin, one in the two entries before it leaves only what follows — and through it the int8 tables and the final heap."""
    _need_ref_float(po)
    rng = np.random.default_rng(4100 + M)
    sizes = [4000, 3500, 4500]
    parts = [rand_codes(rng, s, M) for s in sizes]
    labels = [np.arange(s, dtype=np.uint32) * 3 + i for i, s in enumerate(sizes)]
    keep, R, n = np.float32(0.05), 100, 0
    qmins = set()
    for ma in (1, 3):
        sc = po.RefScanner4(M, parts[:ma], labels[:ma], keep)
        assign = np.arange(ma, dtype=np.int32)
        plain, negs = rand_tables(rng, ma, M), rand_tables(rng, ma, M, negatives=True)
        for bits in NF_NAN:
            for e in range(ma * M * 16):
                for base in ((plain, negs) if e % 4 == 0 or e >= ma * M * 16 - 8 else (plain,)):
                    t = base.copy()
                    t.reshape(-1)[e] = _bits(bits)
                    w = _check_whole_against_reference(po, sc, M, parts[:ma], labels[:ma], keep, assign, t, R, (ma, hex(bits), e),
                                                       offset=(0 if e % 3 else 5))
                    qmins.add(("nan" if np.isnan(w["qmin"]) else "above" if w["qmin"] > max(0, np.nanmin(t)) else "min", base is negs))
                    n += 1
        sc.close()
    assert n >= 2 * 4 * M * 16 * 5 // 4
    # every outcome of the rule was met (a NaN two or three entries before the end hides ALL the negatives: a positive qmin, no clamp)
    assert qmins == {(k, b) for k in ("nan", "above", "min") for b in (False, True)}


@pytest.mark.parametrize("M", [16, 32])
def test_query_scan_on_nonfinite_tables_matches_the_reference_as_compiled(po, M):
    """Random non-finite tables through the reference's scanner_4, whole, and orc_query_scan: single entries, whole rows, sparse
    entries and whole tables of NaN (both signs, two payloads), +-inf and +-FLT_MAX, alone and mixed, with negatives, flat and IVF,
    R = 1 / 10 / 100, tie-rounded tables; rows of +inf and -inf whose sums are NaN, in numbers that leave about R pushable starts,
    so that the "Max quantization bound too high" exit is taken on both sides of its edge."""
    _need_ref_float(po)
    rng = np.random.default_rng(5200 + M)
    nexit = nrun = 0
    for db in range(6):
        ivf = db % 2 == 1
        sizes = [int(s) for s in rng.integers(1500, 5000, 5)] if ivf else [int(rng.integers(15000, 25000))]
        parts = [rand_codes(rng, s, M) for s in sizes]
        labels = [rng.integers(0, 2 ** 32, s, dtype=np.uint64).astype(np.uint32) for s in sizes] if ivf else None
        keep = np.float32(0.05)
        sc = po.RefScanner4(M, parts, labels, keep)
        for q in range(120):
            ma = int(rng.integers(2, 5)) if ivf else 1
            assign = rng.permutation(len(sizes))[:ma].astype(np.int32)
            R = int(rng.choice([1, 10, 100, 100]))
            t = rand_tables(rng, ma, M, negatives=(q % 3 == 0))
            if q % 7 == 0:
                t = (np.round(t / t.max() * 6) * np.float32(0.5)).astype(np.float32)
            flat, kind = t.reshape(-1), q % 6
            vals = [_bits(b) for b in (NF_VALUES if q % 2 else NF_NAN)]
            if kind == 0:
                flat[int(rng.integers(flat.size))] = vals[q % len(vals)]
            elif kind == 1:
                r = int(rng.integers(ma * M))
                flat[r * 16:r * 16 + 16] = [vals[(q + i) % len(vals)] for i in range(16)]
            elif kind == 2:
                for e in rng.choice(flat.size, 12, replace=False):
                    flat[e] = vals[int(rng.integers(len(vals)))]
            elif kind == 3:                                         # NaN sums: +inf in some rows, -inf in others
                for r, v in ((1, 0x7f800000), (2, 0x7f800000), (3, 0x7f800000), (6, 0xff800000)):
                    flat[r * 16:r * 16 + int(rng.integers(4, 12))] = _bits(v)
            elif kind == 4:                                         # most starts NaN: around the exit's edge
                flat[:int(rng.integers(12, 16))] = vals[q % 2]
                for e in rng.choice(np.arange(16, M * 16), int(rng.integers(0, 5)), replace=False):
                    flat[e] = vals[(q + 1) % 2]
            else:
                flat[:] = vals[q % len(vals)] if q % 12 == 5 else flat
                flat[-1 - int(rng.integers(0, 8))] = vals[q % len(vals)]
            w = _check_whole_against_reference(po, sc, M, parts, labels, keep, assign, t, R, (db, q), may_exit=True, offset=q % 4)
            nexit += w["rc"]
            nrun += 1 - w["rc"]
        sc.close()
    assert nexit >= 20 and nrun >= 300


def test_quantizer_on_nonfinite_entries_and_bounds_matches_the_reference_as_compiled(po):
    """QuantizerMAX<int8_t> of the build on NaN / inf / FLT_MAX entries and on the bounds the non-finite rules produce: a NaN qmin,
    qmin above qmax, qmax = -inf, qmax = qmin.  A NaN entry is 127; a product that is NaN or outside int32 is 0; the rest is the
    low byte of the truncation (no saturation)."""
    _need_ref_float(po)
    rng = np.random.default_rng(77)
    seen127 = seen_wrap = 0
    for t in range(400):
        qmin, qmax = np.float32(rng.random() * 2), np.float32(2 + rng.random() * 50)
        if t % 8 == 1:
            qmin = _bits(NF_NAN[t % 2])
        elif t % 8 == 2:
            qmin, qmax = qmax, qmin                                # the reduction forgot the small entries: qmin above qmax
        elif t % 8 == 3:
            qmax = _bits(0xff800000)
        elif t % 8 == 4:
            qmax = np.float32(qmin)
        elif t % 8 == 5:
            qmax = np.nextafter(qmin, np.float32(np.inf))          # scale = 127 / ulp: products far outside int8, some outside int32
        v = (rng.random(1600).astype(np.float32) * np.float32(60) - np.float32(3 if t % 3 == 0 else 0)).astype(np.float32)
        for e in rng.choice(1600, 160, replace=False):
            v[e] = _bits(NF_VALUES[int(rng.integers(len(NF_VALUES)))])
        if t % 8 == 5:
            v[::5] = (qmin - rng.random(320).astype(np.float32) * np.float32([1e-6, 1e-3, 1.0, 1e6][t % 4])).astype(np.float32)
        v = np.ascontiguousarray(v.reshape(-1, 16))
        want = po.reff_quantize_tables(v, qmin, qmax)
        got = po.quantize_tables(v, qmin, qmax, mode=1)
        assert np.array_equal(want, got), t
        assert (got[np.isnan(v)] == 127).all()
        seen127 += int(np.isnan(v).sum())
        seen_wrap += int((got < 0).sum())
    assert seen127 > 1000 and seen_wrap > 100


def test_nonfinite_fixture_is_what_the_oracle_computes(po):
    """tests/golden/ref_query_scan_nonfinite_cases.npz (the reference build's outputs, oracle/gen_golden_float.py) against
    orc_query_scan: runs everywhere.  Start heap and qmax as bits, exit status, final heap, sort_keys, the tables after the call."""
    fam, nexit = set(), 0
    for c in golden_cases.nonfinite_cases(po):
        M, R, assign, keep = c["M"], c["R"], c["assign"], c["keep"]
        starts = [c["parts"][p][:po.start_size(c["parts"][p].shape[0], keep)] for p in assign]
        slab = None if c["labels"] is None else [c["labels"][p][:len(s)] for p, s in zip(assign, starts)]
        ok, ov = po.scan4_start(M, starts, slab, c["tables"], R)
        assert np.array_equal(ok, c["start_keys"]) and _same_bits(ov, c["start_vals"]), c["cid"]
        tb = c["tables"].copy()
        o = po.query_scan(M, c["parts"], c["labels"], keep, assign, tb, R)
        assert o["rc"] == c["exit"] and o["qmax_bits"] == int(c["start_vals"][:1].view(np.uint32)[0]), c["cid"]
        fam.add(c["family"].rstrip("0123456789_"))
        if c["exit"]:
            nexit += 1
            continue
        assert np.array_equal(o["keys"], c["keys"]) and np.array_equal(o["values"], c["vals"]), (c["cid"], c["family"])
        assert np.array_equal(po.sort_keys_i8(o["keys"], o["values"]), c["sorted"]), c["cid"]
        assert np.array_equal(tb.view(np.uint32), c["after"]), c["cid"]
    assert nexit >= 4 and len(fam) >= 25


def test_the_nan_rules_are_not_the_source_text(po):
    """The pin is not vacuous: on the fixture's cases the SOURCE-level expressions (quant_mode 0: the iterator loop of min_element,
    v >= max) give other heaps than the reference build where a NaN entry is in reach of a code's score, and the build's qmin is
    neither the source loop's nor the minimum over the non-NaN entries once a NaN sits in the table's last three entries."""
    differ = ncase = 0
    for c in golden_cases.nonfinite_cases(po):
        nan = np.isnan(c["tables"])
        if c["exit"] or not nan.any():
            continue
        o0 = po.query_scan(c["M"], c["parts"], c["labels"], c["keep"], c["assign"], c["tables"].copy(), c["R"], quant_mode=0)
        o1 = po.query_scan(c["M"], c["parts"], c["labels"], c["keep"], c["assign"], c["tables"].copy(), c["R"], quant_mode=1)
        assert (o1["qtables"].reshape(nan.shape)[nan] == 127).all() and (o0["qtables"].reshape(nan.shape)[nan] == 0).all(), c["cid"]
        differ += int(not (np.array_equal(o0["keys"], c["keys"]) and np.array_equal(o0["values"], c["vals"])))
        ncase += 1
    assert ncase >= 20 and differ >= ncase // 2
    rng = np.random.default_rng(1)
    t = (rng.random(256).astype(np.float32) + np.float32(1))
    for e in (255, 254, 253, 252, 0, 7):
        u = t.copy()
        u[e] = np.nan
        u[(e + 100) % 256] = np.float32(0.5)                        # the true minimum, in another lane than the NaN
        got = po.min_element_compiled(u)
        if e == 255:
            assert np.isnan(got)                                    # the last scalar step: the NaN is the second operand
        elif e >= 253:
            assert got == u[e + 1:].min() > np.float32(0.5)         # a scalar step on a NaN forgets EVERYTHING before it
        else:
            assert got == np.float32(0.5), (e, got)
    u = t.copy()
    u[1 + 8 * 3 + 2] = np.float32(0.25)                             # lane 2 of the 8-lane loop, block 3
    u[1 + 8 * 9 + 2] = np.nan                                       # the same lane, later: the 0.25 is forgotten
    u[200] = np.float32(0.75)                                       # (lane 7)
    assert po.min_element_compiled(u) == np.float32(0.75) and np.nanmin(u) == np.float32(0.25)


def test_reference_exit_paths(po):
    """qmax > 1e30 (fewer than R starts: heap not full, or only the sentinel evicted...) -> the reference prints its warning
    and exit(1)s (db_query_4.cpp:271-274); mixed labelled / unlabelled partitions -> exit(1) in prepare_database (118-124)."""
    _need_ref_float(po)
    rng = np.random.default_rng(8)
    codes = rand_codes(rng, 1000, 16)
    tables = rand_tables(rng, 1, 16)
    for s, code in ((1, 1), (98, 1), (99, 1), (100, 0), (101, 0)):
        keep = np.float32((s + 0.5) / 1000)
        sc = po.RefScanner4(16, [codes], None, keep)
        assert sc.sizes()[0][0] == s == po.start_size(1000, keep)
        assert sc.try_query([0], tables, 100) == code
        assert po.query_scan(16, [codes], None, keep, [0], tables.copy(), 100)["rc"] == code
        sc.close()
    a, b = rand_codes(rng, 50, 16), rand_codes(rng, 60, 16)
    la, lb = np.arange(50, dtype=np.uint32), np.arange(60, dtype=np.uint32)
    assert po.RefScanner4.try_prepare(16, [a, b], [la, lb], 0.5) == 0
    assert po.RefScanner4.try_prepare(16, [a, b], None, 0.5) == 0
    assert po.RefScanner4.try_prepare(16, [a, b], [la, None], 0.5) == 1
    assert po.RefScanner4.try_prepare(16, [a, b], [None, lb], 0.5) == 1
    # has_labels is read off partition 0 even when it is EMPTY (compute_sizes, 105-110), and index_db hands out an empty
    # std::vector's data() = nullptr for it (databases.hpp:237-243): a labelled database whose partition 0 is empty is refused
    e = np.zeros((0, 8), np.uint8)
    assert po.RefScanner4.try_prepare(16, [e, a, b], [None, la, lb], 0.5) == 1
    assert po.RefScanner4.try_prepare(16, [a, e, b], [la, None, lb], 0.5) == 0


def test_start_sizes_match_the_reference_as_compiled(po):
    """A8: starts_sizes = max(1u, unsigned(size * keep)), the product evaluated in float (db_query_4.cpp:125-126), at sizes
    where size * keep lands on or next to an integer."""
    _need_ref_float(po)
    sizes = [1, 2, 99, 100, 101, 199, 200, 1000, 4999, 5000, 5001, 65535, 65536, 100000, 300000, 1000003, 2000000]
    parts = [np.zeros((s, 8), np.uint8) for s in sizes]
    for keep in (0.01, 0.002, 0.0005, 0.1, 0.3, 1.0 / 3.0, 0.999, 1.0):
        sc = po.RefScanner4(16, parts, None, np.float32(keep))
        starts = sc.sizes()[0]
        assert [po.start_size(s, np.float32(keep)) for s in sizes] == list(starts), keep
        sc.close()


def test_direct_tables_match_the_reference_as_compiled(po):
    """A10 (direct form): compute_dists_single_simd_cg<DSQ> -> fmanorm for every sq_dim of the reference's dispatch
    (distances.cpp:50-84); and sq_dims it has no instance of are refused by it (ours take the sequential loop)."""
    _need_ref_float(po)
    rng = np.random.default_rng(31)
    for dsq in (4, 8, 16, 30, 32, 48, 60, 64, 96, 120, 128, 192, 240, 256):
        for t in range(12):
            M = int(rng.choice([16, 32]))
            scale = np.float32(rng.choice([0.01, 1.0, 100.0]))
            cb = (rng.normal(size=(M, 16, dsq)) * scale).astype(np.float32)
            x = (rng.normal(size=M * dsq) * scale).astype(np.float32)
            if t == 0:
                x[:dsq] = cb[0, 3]                                   # an exact zero distance
            assert np.array_equal(po.reff_tables_direct(cb, x), po.tables_direct(cb, x, sum_mode=1)), (dsq, t)
    with pytest.raises(AssertionError):
        po.reff_tables_direct(np.zeros((32, 16, 3), np.float32), np.zeros(96, np.float32))


@pytest.mark.parametrize("NSQ", [4, 8, 16])
def test_scan_standard_matches_the_reference_as_compiled(po, NSQ):
    """BASELINE configs[0]: scanner_simple::query_scan (db_query.cpp:26-45) with scan_standard<uint8_t,NSQ>."""
    _need_ref_float(po)
    rng = np.random.default_rng(NSQ)
    for t in range(60):
        nparts = 1 + t % 3
        parts = [rng.integers(0, 256, (int(rng.integers(1, 4000)), NSQ), dtype=np.uint8) for _ in range(nparts)]
        labels = None if t % 2 else [rng.integers(0, 2 ** 31, p.shape[0]).astype(np.uint32) for p in parts]
        tb = (rng.random((nparts, NSQ * 256), dtype=np.float32) * np.float32(rng.choice([1, 100]))).astype(np.float32)
        R = int(rng.choice([10, 100]))
        rk, rv = po.reff_scan_standard_u8(NSQ, parts, labels, tb, R)
        ok, ov = po.scan_standard_u8(NSQ, parts, labels, tb, R)
        assert np.array_equal(rk, ok) and np.array_equal(rv, ov), t


def test_pack4_and_residuals_match_the_reference(po):
    _need_ref_float(po)
    rng = np.random.default_rng(2)
    for M in (16, 32):
        assign = rng.integers(0, 16, (501, M)).astype(np.int32)
        assert np.array_equal(po.reff_pack4(assign, M), po.pack4(assign, M))
    v = rng.normal(size=96).astype(np.float32)
    base = rng.normal(size=(40, 96)).astype(np.float32)
    a = rng.permutation(40)[:7].astype(np.int32)
    assert np.array_equal(po.reff_substract_from_unique(v, base, a), (v[None, :] - base[a]).astype(np.float32))


def test_coarse_selection_against_the_reference_heaps(po):
    """N1, the selection half of find_k_neighbors (neighbors.cpp:18-28, 47-71: add_candidates_heaps block by block, then
    kv_binheap::sort — compiled from the reference's text; the distance half is cblas_sgemm and is not).  (1) The oracle's
    restatement (orc_select_k_neighbors: the heap's push + libstdc++'s std::sort on the permutation) equals the reference's heaps
    entry for entry, distances AND indices, on tie-free and on tie-heavy inputs, at the shapes of configs[2] / [4], at ragged
    block sizes, with k > neighbours.  (2) On distances WITHOUT exact ties among the kept and the boundary values both equal
    `the k smallest by (distance, index)` — the fast path of the device's selection kernels; WITH exact ties they do not (which
    of several equal maxima sits at the heap's root when a smaller value arrives, and std::sort's order of equal keys, decide),
    which is why the device has coarse_exact_select (GPU: test_coarse_assignment_with_exact_distance_ties_is_find_k_neighbors)."""
    _need_ref_float(po)
    rng = np.random.default_rng(77)

    def rule(d, k):
        return np.stack([np.lexsort((np.arange(d.shape[1]), row))[:k] for row in d]).astype(np.int32)

    for count, K, k in ((40, 4096, 32), (24, 16384, 64), (300, 300, 8), (257, 256, 1), (5, 1000, 16), (3, 513, 64), (2, 70, 64)):
        base = (np.arange(K) * 0.37 + rng.random(K) * 0.2).astype(np.float32)     # K distinct values ...
        assert len(np.unique(base)) == K
        d = np.stack([rng.permutation(base) for _ in range(count)])               # ... in another order for every vector
        a, sd = po.reff_select_k_neighbors(d, k)
        want = rule(d, k)
        assert np.array_equal(a, want), (count, K, k)
        assert np.array_equal(sd, np.take_along_axis(d, want, 1))
        b, sb = po.select_k_neighbors(d, k)
        assert np.array_equal(b, a) and np.array_equal(sb, sd)
        # ties only ABOVE the kept values do not matter either
        d2 = d.copy()
        kth = np.sort(d2, 1)[:, k - 1:k]
        d2[d2 > kth] = np.floor(d2[d2 > kth] / 16.0) * 16.0 + 16.0 + kth.max()
        a2, _ = po.reff_select_k_neighbors(d2, k)
        assert np.array_equal(a2, want), (count, K, k)
    # exact ties among the kept values and across the boundary
    ndiff = 0
    for count, K, k, levels in ((50, 4096, 32, 300), (20, 16384, 64, 2000), (40, 300, 8, 20), (40, 1000, 16, 5), (10, 513, 64, 3),
                                (10, 70, 64, 7), (6, 5000, 200, 100), (4, 64, 256, 9), (6, 2000, 256, 50), (30, 700, 2, 3),
                                (300, 260, 5, 4), (8, 9000, 129, 40)):
        d = np.floor(rng.random((count, K)) * levels).astype(np.float32)
        a, sd = po.reff_select_k_neighbors(d, k)
        b, sb = po.select_k_neighbors(d, k)
        kk = min(k, K)
        assert np.array_equal(a[:, :kk], b[:, :kk]) and np.array_equal(sd[:, :kk], sb[:, :kk]), (count, K, k, levels)
        assert np.array_equal(sd[:, :kk], np.take_along_axis(d, rule(d, kk), 1))    # (the kept DISTANCES are the k smallest either way)
        ndiff += int(not np.array_equal(a[:, :kk], rule(d, kk)))
    assert ndiff >= 10


NAN_BITS = (0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff)       # quiet NaN, its negative, the largest payloads of both signs
K_SELECT = (1, 2, 5, 7, 8, 9, 16, 17, 32, 64, 256)


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def nonfinite_rows(rng, K):
    """Distance rows [n][K] with non-finite entries where selections go wrong: NaN of every bit pattern in NAN_BITS, +inf and
    FLT_MAX, at index 0, in the middle, at K-1 and at the last entry of a 256-block (add_candidates_heaps' block edge); all-NaN
    rows, all-+inf rows, and rows with only a few finite values."""
    special = [_f32(b) for b in NAN_BITS] + [np.float32(np.inf), FMAX]
    rows = []
    spots = sorted({0, K // 2, K - 1, min(K - 1, 255), min(K - 1, 256)})
    for v in special:
        for at in spots:
            r = (rng.random(K) * 10).astype(np.float32)
            r[at] = v
            rows.append(r)
        r = (rng.random(K) * 10).astype(np.float32)
        r[spots] = v
        rows.append(r)
        rows.append(np.full(K, v, np.float32))                                     # the whole row
        r = np.full(K, v, np.float32)
        few = rng.choice(K, size=min(K, 3), replace=False)
        r[few] = rng.random(len(few)).astype(np.float32)                           # fewer finite values than most k
        rows.append(r)
    for frac in (0.05, 0.5, 0.95):                                                 # mixtures of all of them
        r = (rng.random((8, K)) * 10).astype(np.float32)
        m = rng.random((8, K)) < frac
        r[m] = rng.choice(np.array(special, np.float32), size=int(m.sum()))
        rows.extend(r)
    r = np.floor(rng.random((4, K)) * 3).astype(np.float32)                        # exact ties around NaNs
    r[:, ::5] = np.nan
    rows.extend(r)
    return np.stack(rows).astype(np.float32)


def test_coarse_selection_on_non_finite_distances_is_the_reference_binary(po):
    """find_k_neighbors' selection half on NaN, +inf and FLT_MAX distances.  The reference is built with -ffast-math, and its
    replace-top test compiles to !(v >= top) (vcomiss + jae), not to the source's v < top: a NaN always replaces the heap top,
    and the next value always replaces a NaN top.  orc_select_k_neighbors writes that predicate out and must equal the
    reference's heaps entry for entry (indices, and distances bit for bit, NaN payloads included) for every k, with K below
    and above k."""
    _need_ref_float(po)
    rng = np.random.default_rng(2024)
    for K in (1, 3, 7, 16, 70, 255, 256, 257, 513, 1000):
        d = nonfinite_rows(rng, K)
        for k in K_SELECT:
            a, sd = po.reff_select_k_neighbors(d, k)
            b, sb = po.select_k_neighbors(d, k)
            kk = min(k, K)
            assert np.array_equal(b[:, :kk], a[:, :kk]), (K, k)
            assert np.array_equal(sb[:, :kk].view(np.uint32), sd[:, :kk].view(np.uint32)), (K, k)
            assert ((a[:, :kk] >= 0) & (a[:, :kk] < K)).all()
    # the rule, on rows that show it: the result is the first strict minimum after the last NaN (k = 1)
    d = np.full((1, 20), np.nan, np.float32)
    d[0, 7] = 1
    for sel in (po.reff_select_k_neighbors, po.select_k_neighbors):
        assert sel(d, 1)[0].tolist() == [[19]] and sel(d, 4)[0].tolist() == [[17, 18, 2, 19]]
        assert sel(np.full((1, 9), np.inf, np.float32), 3)[0].tolist() == [[0, 1, 2]]
        assert sel(np.array([[np.nan, 3, 2, np.nan, 5, 4, 6]], np.float32), 1)[0].tolist() == [[5]]
        assert sel(np.array([[2, 1, 3, np.nan]], np.float32), 1)[0].tolist() == [[3]]


# ------------------------------------------------------------------------------------------------ N4: the encoder
def _seq_rotate(po, v, rot):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("gen_golden_encode", os.path.join(os.path.dirname(po.__file__), "gen_golden_encode.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.seq_rotate(v, rot)


def test_oracle_encoder_matches_reference_golden(po):
    """orc_pq_encode (find_k_neighbors with k = 1 on the BLAS-expansion distances) writes the codes of
    tests/golden/ref_encode_cases.npz — the chain of the reference's own extract_subvectors, compute_cross_dists_blas up to
    its sgemm, add_candidates_heaps and multiple_set_bits_4 — and orc_cross_dists' norm half is that matrix bit for bit.
    Runs everywhere.  The direct form (what this repository encoded with before round 6) writes OTHER codes on the
    cancellation-dominated and the midpoint cases: the fixtures can tell the forms apart."""
    ncase = direct_differs = 0
    for c in golden_cases.encode_cases():
        M, ds = c["M"], c["dim"] // c["M"]
        assert np.array_equal(po.pq_encode(c["codebooks"], c["vectors"], c["rotation"]), c["codes"]), c["cid"]
        x = c["vectors"] if c["rotation"] is None else _seq_rotate(po, c["vectors"], c["rotation"])
        for m in range(M):
            sub = x[:c["norms"].shape[1], m * ds:(m + 1) * ds]
            assert np.array_equal(po.cross_dists(c["codebooks"][m], sub, with_product=False), c["norms"][m]), (c["cid"], m)
        direct_differs += int((po.pq_encode(c["codebooks"], c["vectors"], c["rotation"], form=0) != c["codes"]).any())
        ncase += 1
    assert ncase == 15 and direct_differs >= 4


def _first_strict_min(d):
    """k = 1 with the source's IEEE test (replace iff v < best): the first strict minimum, a NaN at index 0 never replaced."""
    out = np.zeros(d.shape[0], np.int32)
    for i, r in enumerate(d):
        for c in range(1, d.shape[1]):
            if r[c] < r[out[i]]:
                out[i] = c
    return out


def _reference_encode_chain(po, codebooks, vectors, select=None):
    """base_pq::encode_multiple_vectors as a chain of the reference's compiled pieces: extract_subvectors, compute_cross_dists_blas
    up to its sgemm (the norms), then -2 x.c as one sequential dot added in one rounding (what orc_cross_dists restates for the
    sgemm), find_k_neighbors' selection with k = 1 and multiple_set_bits_4.  (fma(-2, dot, base) of float32s is exact in float64
    up to the final rounding.)"""
    M, _, ds = codebooks.shape
    assign = np.zeros((vectors.shape[0], M), np.int32)
    for m in range(M):
        sub = po.reff_extract_subvectors(vectors, ds, m)
        base = po.reff_cross_norms(codebooks[m], sub)
        dot = np.zeros((sub.shape[0], 16), np.float32)
        for j in range(ds):
            dot = (dot + (sub[:, j:j + 1] * codebooks[m][None, :, j]).astype(np.float32)).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            dist = (base.astype(np.float64) - 2.0 * dot.astype(np.float64)).astype(np.float32)
        assign[:, m] = po.reff_select_k_neighbors(dist, 1)[0][:, 0] if select is None else select(dist)
    return po.reff_pack4(assign, M)


def test_oracle_encoder_on_nan_codebooks_and_vectors_is_the_reference_chain(po):
    """orc_pq_encode (form 1) with NaN codebook centroids at index 0, in the middle and at 15 of a sub-quantizer, NaN vector
    components, +inf and FLT_MAX-scale entries: the codes equal the chain of the reference's own compiled pieces — in particular
    its k = 1 selection, which picks the first strict minimum after the LAST NaN distance, not the first centroid."""
    _need_ref_float(po)
    rng = np.random.default_rng(31)
    nan_differs = 0
    for M, ds, n in ((8, 4, 300), (16, 8, 200), (4, 16, 120)):
        cb = rng.normal(size=(M, 16, ds)).astype(np.float32)
        v = rng.normal(size=(n, M * ds)).astype(np.float32)
        cb[0, 0, 1] = np.nan
        cb[1, 7, :] = _f32(0xffc00000)
        cb[2, 15, 0] = _f32(0x7fffffff)
        cb[3, 0, :] = np.nan
        cb[3, 15, :] = np.nan
        v[::7, 1] = np.nan                                      # one NaN component: all 16 distances of sub-quantizer 0
        v[3::11, M * ds - 1] = np.inf
        v[5::13, ds] = np.float32(3e19)                         # squares overflow to +inf
        got = po.pq_encode(cb, v)
        want = _reference_encode_chain(po, cb, v)
        assert np.array_equal(got, want), (M, ds)
        # the IEEE '<' rule (first strict minimum, a NaN at centroid 0 kept) is what this repository restated before
        ieee = _reference_encode_chain(po, cb, v, select=_first_strict_min)
        nan_differs += int((ieee != got).any())
    assert nan_differs


def test_cross_norms_match_the_reference_as_compiled(po):
    """||v||^2 + ||c||^2 as compute_cross_dists_blas<DSQ> hands it to sgemm, for every DSQ of get_cross_dists_func
    (distances.cpp:87-121) and 16 centroids: the reference's text compiled up to the sgemm call vs orc_cross_dists.  The
    source-order sum (sum_mode 0) is NOT what the binary computes."""
    _need_ref_float(po)
    rng = np.random.default_rng(151)
    for ds in (4, 8, 16, 30, 32, 48, 60, 64, 96, 120, 128, 192, 240, 256):
        c = (rng.normal(size=(16, ds)) * rng.choice([0.01, 1.0, 30.0])).astype(np.float32)
        v = (rng.normal(size=(2000, ds)) * rng.choice([0.01, 1.0, 30.0])).astype(np.float32)
        want = po.reff_cross_norms(c, v)
        assert np.array_equal(po.cross_dists(c, v, with_product=False), want), ds
        assert not np.array_equal(po.cross_dists(c, v, sum_mode=0, with_product=False), want), ds
    assert po.reff_cross_norms(np.zeros((16, 3), np.float32), np.zeros((1, 3), np.float32)) is None   # (no instance: sequential here)


def test_expansion_tables_are_the_cross_dists_per_sub_quantizer(po):
    """orc_tables_expansion (compute_dists_multiple_blas_cg, distances.hpp:277-292) = orc_cross_dists of every
    sub-quantizer's 16 centroids, laid out [count][M*16]; its norm half equals the reference's."""
    rng = np.random.default_rng(9)
    for M, ds in ((16, 8), (32, 4), (32, 3), (16, 30)):
        cb = rng.normal(size=(M, 16, ds)).astype(np.float32)
        v = rng.normal(size=(50, M * ds)).astype(np.float32)
        t = po.tables_expansion(cb, v).reshape(50, M, 16)
        for m in range(M):
            assert np.array_equal(t[:, m], po.cross_dists(cb[m], v[:, m * ds:(m + 1) * ds])), (M, m)
            if po.have_ref_float() and ds != 3:
                assert np.array_equal(po.cross_dists(cb[m], v[:, m * ds:(m + 1) * ds], with_product=False),
                                      po.reff_cross_norms(cb[m], v[:, m * ds:(m + 1) * ds]))


def test_kmeans_centroid_update_as_compiled(po):
    """N4: kmeans_fast_iterations_thread's centroid update (databases.cpp:70-88).  The source divides every component by the member
    count; the reference binary (-ffast-math) multiplies by ONE reciprocal per centroid — a different float in a good part of the
    entries.  The product's default (div_mode 1: device kernel, host twin) is the binary's; this test pins the formula to the
    reference's own loops compiled here with its flags, incl. an empty cluster (NaN) and a one-member cluster."""
    _need_ref_float(po)
    rng = np.random.default_rng(5)
    ndiff = ntot = 0
    for n, dim, K in ((5000, 128, 37), (700, 96, 300), (64, 16, 8), (1200, 33, 7)):
        v = rng.normal(size=(n, dim)).astype(np.float32) * np.float32(3.7)
        a = rng.integers(0, K - 1, n).astype(np.int32)               # (cluster K-1 stays empty)
        a[0] = K - 2 if K > 2 else a[0]
        got = po.reff_kmeans_update(v, a, K)
        s = np.zeros((K, dim), np.float32)
        cnt = np.zeros(K, np.int64)
        for i in range(n):
            s[a[i]] = (s[a[i]] + v[i]).astype(np.float32)
            cnt[a[i]] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            compiled = (s * (np.float32(1.0) / cnt[:, None].astype(np.float32)).astype(np.float32)).astype(np.float32)
            source = (s / cnt[:, None].astype(np.float32)).astype(np.float32)
        assert np.array_equal(got, compiled, equal_nan=True), (n, dim, K)
        assert np.isnan(got[K - 1]).all()
        live = cnt > 0
        ndiff += int((compiled[live] != source[live]).sum())
        ntot += int(live.sum()) * dim
    assert ndiff > ntot // 50                                        # (the two forms really differ)


def test_extraction_refuses_a_drifted_reference(tmp_path):
    """oracle/ref_extract.sh carries the sha256 of every line range it cuts out of the reference: one changed byte inside a
    range stops the build instead of silently compiling something else; the untouched reference passes."""
    import os
    import shutil
    import subprocess
    ref = "/root/reference"
    if not os.path.isdir(ref):
        pytest.skip("no /root/reference here")
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "ref_extract.sh")
    out = tmp_path / "out"
    out.mkdir()
    assert subprocess.run([script, ref, str(out)], stderr=subprocess.PIPE).returncode == 0
    assert sorted(os.listdir(out))[0].startswith("x_") and len(os.listdir(out)) == 21
    drift = tmp_path / "ref"
    drift.mkdir()
    for f in ("quantizers.hpp", "databases.hpp", "query_common.hpp", "db_query_4.cpp", "db_query.cpp", "distances.hpp", "databases.cpp", "quantizers.cpp",
              "neighbors.cpp"):
        shutil.copy(os.path.join(ref, f), drift / f)
    lines = open(drift / "query_common.hpp").read().split("\n")
    lines[69] = lines[69] + " "                                    # one blank appended to line 70 (inside scan_4's range, 59-143)
    open(drift / "query_common.hpp", "w").write("\n".join(lines))
    out2 = tmp_path / "out2"
    out2.mkdir()
    r = subprocess.run([script, str(drift), str(out2)], stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"the reference changed" in r.stderr


@pytest.mark.parametrize("script,committed", [("gen_golden_float.py", "ref_query_scan_cases.npz"), ("gen_golden.py", "ref_scan_cases.npz"),
                                              ("gen_golden_encode.py", "ref_encode_cases.npz"),
                                              ("gen_golden_float.py", "ref_query_scan_nonfinite_cases.npz")])
def test_golden_fixtures_regenerate_from_the_reference_build(po, tmp_path, script, committed):
    """The committed fixtures ARE what the generators produce from the reference build today: every array, bit for bit."""
    import os
    import subprocess
    import sys
    if not (po.have_ref() and po.have_ref_float()):
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / committed)
    subprocess.check_call([sys.executable, os.path.join(root, "oracle", script)], env=dict(os.environ, QADC_GOLDEN_OUT=out),
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    a, b = np.load(out), np.load(os.path.join(root, "tests", "golden", committed))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
