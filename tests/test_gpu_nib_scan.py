"""GPU: the nibble form of the split scan: NS = 8, 9 or 10 of the 16 sub-quantizers are streamed from the
nibble-plane copy; the others (the rows whose entries rise least above their minimum, ties: the highest s; any of the 16) are read
from the row-major codes for the survivors only, and a survivor is a code whose partial sum is below bound - c, c = min(127, the
deferred rows' minima summed).  Every comparison is heaps bit for bit (keys, values, sizes, status): the nibble form forced at small
sizes against the same index with 5 planes and the row-major form, and against the reference build.  A c above the true minimum
would lose candidates (the heaps differ).  The streamed list starts behind the highest deferred sub-quantizer (nib_list), so with
the sixteen windows of consecutive deferred sub-quantizers every sub-quantizer is deferred, streamed in a pair and the single
plane of an odd NS in some query."""
import os
import sys

import numpy as np
import pytest

from helpers import float_tables, heaps_equal

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import split_survivors as ss  # noqa: E402  (the numpy twin of the choice rule: choose_nib, nib_streamed)

pytestmark = pytest.mark.gpu
M = 16
ONE_QUERY_PER_PASS = dict(share_variant=0, mq=0, front_run_max=0, wgq=0)
TINY = dict(head_level=0, small_run=1, level_base=16384)    # lists of a few tiles: every level is a streaming launch on tiles
NSS = (8, 9, 10)
OTHERS = ("split5", "rows")


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def make_index(pyqadc, parts, form, labels=None, keep=0.01, **opts):
    """form: "rows", "split5" or 8 / 9 / 10 (the nibble form with that many streamed sub-quantizers, threshold 1)."""
    idx = pyqadc.Index(M)
    for k, v in dict(ONE_QUERY_PER_PASS, **opts).items():
        idx.set_option(k, v)
    idx.set_split(0, 1) if form == "rows" else idx.set_split(1, 1)
    idx.set_split6(0 if form == "rows" else 1)
    idx.set_split5(0 if form == "rows" else 1)                    # (the nibble form is preferred where both thresholds are met)
    if form in NSS:
        idx.set_split_nib(0 if form == 8 else 1, 1 if form == 8 else 0, 10 if form == 10 else 9)
    idx.add_partitions(parts, labels)
    idx.finalize(keep)
    idx.set_option("profile", 1)
    return idx


def scan_forms(pyqadc, parts, tables, R, labels=None, assign=None, int8=False, nss=NSS, **opts):
    """{form: (result, profile)} of the same query batch: the nibble form per NS, 5 planes, row-major."""
    nq = tables.shape[0]
    assign = np.zeros((nq, 1), np.int32) if assign is None else assign
    out = {}
    for form in tuple(nss) + OTHERS:
        idx = make_index(pyqadc, parts, form, labels, **opts)
        res = idx.scan_i8(assign, tables, R) if int8 else idx.query_scan(assign, tables.copy(), R, want_qtables=True)
        pr = idx.profile()
        assert (pr["split_codes"] > 0) == (form != "rows"), pr
        assert (pr["nib_copy_bytes"] > 0) == (form in NSS), pr
        # every split launch is counted under exactly one form
        assert pr["nib_launches"] + pr["nib8_launches"] + pr["split5_launches"] + pr["split6_launches"] == pr["split_launches"], pr
        assert pr["nib_codes"] + pr["nib8_codes"] + pr["split5_codes"] + pr["split6_codes"] == pr["split_codes"], pr
        assert (pr["nib_launches"] == pr["split_launches"] > 0) == (form in (9, 10)), pr
        assert (pr["nib8_launches"] == pr["split_launches"] > 0) == (form == 8), pr
        assert (pr["split5_launches"] == pr["split_launches"] > 0) == (form == "split5"), pr
        assert pr["nib_survivors"] <= pr["nib_codes"] and pr["nib8_survivors"] <= pr["nib8_codes"], pr
        if form not in (9, 10):
            assert pr["nib_survivors"] == 0, pr
        if form != 8:
            assert pr["nib8_survivors"] == 0, pr
        out[form] = (res, pr)
        idx.close()
    return out


def result_heaps(res, q, int8):
    return res[q] if int8 else res["heaps"][q]


def survivors(pr):
    return pr["nib_survivors"] + pr["nib8_survivors"], pr["nib_codes"] + pr["nib8_codes"]


def assert_same(out, nq, int8, R, nss=NSS):
    """Heaps, sizes and status of every nibble form against the 5-plane and the row-major form."""
    for ns in nss:
        a = out[ns][0]
        for other in OTHERS:
            b = out[other][0]
            for q in range(nq):
                ha, hb = result_heaps(a, q, int8), result_heaps(b, q, int8)
                assert ha[0].shape == hb[0].shape and heaps_equal(ha, hb), (ns, other, q)
            if not int8:
                assert np.array_equal(a["status"], b["status"]), (ns, other)


def assert_reference(po, out, parts, labels, qt, queries, R, int8=True, nss=NSS):
    if not po.have_ref():
        return
    inter = [po.ref_interleave(p) for p in parts]
    for q in queries:
        tab = qt[q] if int8 else out[nss[0]][0]["qtables"][q]
        want = po.ref_scan_interleaved(M, inter, [len(p) for p in parts], labels, tab, R)
        for ns in nss:
            assert heaps_equal(result_heaps(out[ns][0], q, int8), want), (ns, q)


def mask_of(subs):
    return sum(1 << s for s in subs)


def window(k, ns):
    """16 - ns consecutive sub-quantizers from k on, cyclically."""
    return [(k + i) % M for i in range(M - ns)]


def window_tables(rng, ns):
    """16 int8 tables: the rule defers window(k, ns) for table k.  Even k: those rows hold 12..14 (small scores, minima of 12+:
    a large c below the clamp), the others 0..13; odd k: 0..2 (c near 0), the others 8..39."""
    qt = np.empty((M, 1, M, 16), np.int8)
    for k in range(M):
        flat = k % 2 == 0
        qt[k, 0] = rng.integers(0, 14, (M, 16)) if flat else rng.integers(8, 40, (M, 16))
        for s in window(k, ns):
            qt[k, 0, s] = rng.integers(12, 15, 16) if flat else rng.integers(0, 3, 16)
    return qt


def choice_bytes(qt, ns):
    mask, c = ss.choose_nib(qt, ns)
    return [mask & 0xff, mask >> 8, c, 0]


@pytest.mark.parametrize("variant", [0x0d, 0x01])                 # chunked tiles (default), grid-stride tiles
@pytest.mark.parametrize("n", [16383, 3 * 16384, 786_432 + 16 * 7 + 5])   # under a tile; whole tiles; a ragged tile, odd n, n % 16 != 0
def test_nib_matches_the_other_forms_and_reference(pyqadc, po, n, variant):
    rng = np.random.default_rng(n + 1)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 3, 1, M)
    # the last code = the smallest sum query 0's tables allow: a sure candidate, emitted by the ragged end of a run together
    # with its padding-lane replays
    best = tables[0, 0].reshape(M, 16).argmin(axis=1).astype(np.uint8)
    codes[-1] = best[0::2] | (best[1::2] << 4)
    R = 100
    out = scan_forms(pyqadc, [codes], tables, R, variant=variant, **(TINY if n < 100_000 else {}))
    for ns in NSS:
        a, pr = out[ns]
        got, of = survivors(pr)
        assert 0 < got <= of, pr
        reps = (16 - n % 16) % 16
        assert np.count_nonzero(a["heaps"][0][0] == n - 1) == 1 + reps
    assert_same(out, 3, False, R)
    assert_reference(po, out, [codes], None, None, range(3), R, int8=False)


@pytest.mark.parametrize("ns", NSS)
def test_nib_every_sub_quantizer_in_every_role_in_one_launch(pyqadc, po, ns):
    """16 queries of one launch with 16 different masks: every sub-quantizer is deferred, streamed in a pair, and (NS = 9) the
    single plane for some query.  The device's choice bytes are the numpy twin's."""
    rng = np.random.default_rng(1000 + ns)
    n = 300_007
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = window_tables(rng, ns)
    lists = []
    for k in range(M):
        mask, c = ss.choose_nib(qt[k, 0], ns)
        assert mask == mask_of(window(k, ns)) and (12 * (M - ns) <= c < 127 or c <= 16), (k, mask, c)
        lists.append(ss.nib_streamed(mask))
        assert len(lists[-1]) == ns and lists[-1][-1] == (k - 1) % M
    got = pyqadc.nib_choice(qt)
    assert got.tolist() == [[choice_bytes(qt[k, 0], s) for s in NSS] for k in range(M)]
    assert {l[-1] for l in lists} == set(range(M))                               # last of the list: the single plane of an odd NS
    assert {s for l in lists for s in l[:2 * (ns // 2)]} == set(range(M))        # fused in a pair
    assert {s for k in range(M) for s in window(k, ns)} == set(range(M))         # deferred
    R = 150
    out = scan_forms(pyqadc, [codes], qt, R, int8=True, nss=(ns,))
    got, of = survivors(out[ns][1])
    assert 0 < got < of, out[ns][1]
    assert_same(out, M, True, R, nss=(ns,))
    assert_reference(po, out, [codes], None, qt, (0, 5, 10, 15), R, nss=(ns,))


def test_nib_choice_bytes_equal_the_twin(pyqadc):
    rng = np.random.default_rng(77)
    qt = np.concatenate([rng.integers(0, hi, (40, M, 16)) for hi in (2, 5, 30, 128)]).astype(np.int8)
    qt[0] = 0                                                    # all rows equal
    qt[1] = 127
    qt[2, 8:] = qt[2, :8]                                        # pairs of equal rows: ties
    got = pyqadc.nib_choice(qt)
    want = [[choice_bytes(qt[t], ns) for ns in NSS] for t in range(len(qt))]
    assert got.tolist() == want
    assert got[0].tolist() == [[0x00, 0xff, 0, 0], [0x00, 0xfe, 0, 0], [0x00, 0xfc, 0, 0]] and got[1, :, 2].tolist() == [127] * 3


def test_nib_float_tables_choose_different_masks_inside_one_launch(pyqadc, po):
    """Float tables (the quantizer's workgroup makes the choice): seven cheap rows per query, a different window each."""
    rng = np.random.default_rng(32)
    n = 600_011
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    nq = 16
    tables = float_tables(rng, nq, 1, M)
    for q in range(nq):
        for s in window(q, 9):
            tables[q, 0].reshape(M, 16)[s] *= np.float32(0.02)
    R = 50
    out = scan_forms(pyqadc, [codes], tables, R)
    a = out[9][0]
    chosen = [ss.choose_nib(np.asarray(a["qtables"][q]).reshape(-1, M, 16)[0], 9)[0] for q in range(nq)]
    assert len(set(chosen)) >= 8 and {s for m in chosen for s in range(M) if m >> s & 1} == set(range(M)), chosen
    assert_same(out, nq, False, R)
    assert_reference(po, out, [codes], None, None, (1, 9, 15), R, int8=False)


def edge_tables(rng, case):
    """The slack-edge tables; with NS = 9 the rule defers rows 9..15 in every case (8: 8..15, 10: 10..15)."""
    qt = np.zeros((2, 1, M, 16), np.int8)
    if case == "clamp":                 # constant rows (all scores 0: the highest rows are deferred) of 127 there: c clamps, bsurv = 0
        qt[:, :, 0:8, :] = 3
        qt[:, :, 8:16, :] = 127
    elif case == "c0":                  # deferred rows: 0 with a few ones (minimum 0: c = 0); streamed rows spread wide
        qt[:, :, 0:8, :] = rng.integers(0, 60, (2, 1, 8, 16), dtype=np.int8)
        qt[:, :, 8:16, 3] = 1
    elif case == "reach":               # streamed rows 0 but for one entry, deferred rows 2 (the last: some threes): every sum is >= c
        qt[:, :, 0:10, 5] = 50
        qt[:, :, 8:16, :] = 2
        qt[:, :, 8:10, 5] = 52
        qt[:, :, 15, 0:4] = 3
    else:                               # "sat": streamed rows 127, deferred rows 4: min(127, partial) is never below a bound
        qt[:, :, 0:8, :] = 127
        qt[:, :, 8:16, :] = 4
    return qt


@pytest.mark.parametrize("case", ["clamp", "c0", "reach", "sat"])
def test_nib_slack_edges(pyqadc, po, case):
    rng = np.random.default_rng({"clamp": 300, "c0": 301, "reach": 302, "sat": 303}[case])
    n = 500_009
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = edge_tables(rng, case)
    R = 50 if case == "reach" else 300
    for ns in NSS:
        for q in range(2):
            mask, c = ss.choose_nib(qt[q, 0], ns)
            if case != "reach" or ns == 9:
                assert mask == mask_of(range(ns, M)), (ns, hex(mask))
            assert {"clamp": c == 127, "c0": c == 0, "reach": 12 <= c <= 16, "sat": 24 <= c <= 32}[case], (ns, c)
    # "reach": level 0 is a nibble launch too (its bound is 127: most codes survive and become candidates); more than half of the
    # codes have the smallest sum there is (16 = the c of NS = 8: the bound is reached exactly; c = 14 and 12 with 9 and 10 streamed,
    # whose partials are at least 2 and 4), so from level 1 on the bound is 16, bsurv = 0, 2 and 4, and no code survives.  A c one
    # too large would lose candidates (the heaps differ); one too small would keep half of the codes survivors to the end.
    out = scan_forms(pyqadc, [codes], qt, R, int8=True, **(TINY if case == "reach" else {}))
    for ns in NSS:
        pr = out[ns][1]
        got, of = survivors(pr)
        if case in ("clamp", "sat"):
            assert got == 0 and pr["regrows"] == 0, pr       # c >= bound, or no partial below any bound: no survivor
        elif case == "reach":
            assert 0 < got <= 16384 * 2, pr                  # (two queries: level 0's codes at the most)
        else:
            assert 0 < got <= of and pr["regrows"] == 0, pr
    assert_same(out, 2, True, R)
    assert_reference(po, out, [codes], None, qt, range(2), R)


def saturation_tables(rng, where):
    """Entries of 127 in the streamed rows, the deferred rows or both; the deferred rows stay the rule's choice for NS = 9 (one
    127 per row there: the score rises by 127 a row, the others' spread is wider)."""
    deferred = (2, 3, 5, 10, 11, 14, 15)
    qt = rng.integers(8, 48, (2, 1, M, 16), dtype=np.int8)
    for s in deferred:
        qt[:, :, s, :] = rng.integers(0, 4, (2, 1, 16), dtype=np.int8)
    big = rng.random((2, 1, M, 16)) < 0.3
    big[:, :, deferred, :] = False
    if where != "deferred":
        qt[big] = 127
    if where != "streamed":
        for i, s in enumerate(deferred):
            qt[:, :, s, (3 * i + 1) % 16] = 127
    return qt, deferred


@pytest.mark.parametrize("where", ["streamed", "deferred", "both"])
def test_nib_saturation(pyqadc, po, where):
    """Entries of 127: partial sums and full sums above 127, min(127, .) on both sides of the comparison with the bound."""
    rng = np.random.default_rng({"streamed": 51, "deferred": 52, "both": 53}[where])
    n = 700_003
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt, deferred = saturation_tables(rng, where)
    assert all(ss.choose_nib(qt[q, 0], 9)[0] == mask_of(deferred) for q in range(2))
    R = 400
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, 2, True, R)
    assert_reference(po, out, [codes], None, qt, range(2), R)


def test_nib_tie_heavy_tables(pyqadc, po):
    """Two distinct entry values only, and a table whose rows are all equal: thousands of codes share every sum, the heap's
    content is decided by scan order."""
    rng = np.random.default_rng(41)
    n = 800_021
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = (rng.integers(0, 2, (3, 1, M, 16)) * 9).astype(np.int8)
    qt[2, 0, :] = qt[2, 0, 0]
    R = 500
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, 3, True, R)
    assert_reference(po, out, [codes], None, qt, range(3), R)


@pytest.mark.parametrize("R", [1, 9_000, 10_003, 11_000])          # around the number of starts (10 000)
def test_nib_R_around_the_starts(pyqadc, po, R):
    rng = np.random.default_rng(R)
    n = 1_000_003
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    out = scan_forms(pyqadc, [codes], tables, R)
    assert_same(out, 2, False, R)
    a = out[9][0]
    assert np.all((a["status"] == 0) == (R <= 10_000)), a["status"]
    assert_reference(po, out, [codes], None, None, [q for q in range(2) if a["status"][q] == 0], R, int8=False)


def test_nib_with_labels_and_several_partitions(pyqadc, po):
    rng = np.random.default_rng(17)
    sizes = [700_001, 1_600_000, 16384 * 40 + 9]
    parts = [rng.integers(0, 256, (s, M // 2), dtype=np.uint8) for s in sizes]
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    nq, ma = 2, 3
    tables = float_tables(rng, nq, ma, M)
    assign = np.array([[0, 1, 2], [2, 0, 1]], np.int32)
    R = 64
    out = scan_forms(pyqadc, parts, tables, R, labels=labels, assign=assign)
    for ns in NSS:
        assert 0 < survivors(out[ns][1])[1] < out[ns][1]["scan_codes"], out[ns][1]
    assert_same(out, nq, False, R)
    if po.have_ref():
        a = out[9][0]
        for q in range(nq):
            order = [int(p) for p in assign[q]]
            inter = [po.ref_interleave(parts[p]) for p in order]
            want = po.ref_scan_interleaved(M, inter, [len(parts[p]) for p in order], [labels[p] for p in order], a["qtables"][q], R)
            for ns in NSS:
                assert heaps_equal(out[ns][0]["heaps"][q], want), (ns, q)


def test_nib_loose_bounds_and_region_overflow(pyqadc, po):
    """Large R: most codes survive; a small candidate region overflows and the batch is re-run (the existing fallback)."""
    rng = np.random.default_rng(6)
    n = 600_000
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    R = 4000
    out = scan_forms(pyqadc, [codes], tables, R, cand_capacity=256)
    for ns in NSS:
        assert out[ns][1]["regrows"] >= 1, out[ns][1]
    assert_same(out, 2, False, R)
    assert_reference(po, out, [codes], None, None, range(2), R, int8=False)


def test_nib_thresholds_pick_the_form_per_launch(pyqadc):
    """set_split_nib(min_run, min_run8, ns): launches whose runs all have min_run8 codes stream 8, the others with min_run codes ns,
    the rest of this index 5 planes; 0 = never.  A launch is counted under exactly one form."""
    rng = np.random.default_rng(8)
    n = 3_000_000                                            # levels [128 Ki, 512 Ki), [512 Ki, 2 Mi), [2 Mi, n)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    res = {}
    for thr in ((0, 0), (1, 0), (0, 1), (1 << 20, 0), (1, 1 << 20), (1 << 19, 1 << 20), (1 << 40, 1 << 40)):
        idx = make_index(pyqadc, [codes], 9)                 # (the copy is built: thresholds 1, 0 at finalize)
        idx.set_split_nib(thr[0], thr[1], 10)
        res[thr] = (idx.query_scan(np.zeros((2, 1), np.int32), tables.copy(), 100), idx.profile())
        idx.close()
    count = lambda thr: tuple(res[thr][1][k] for k in ("nib_launches", "nib8_launches", "split5_launches"))
    for thr, (_, pr) in res.items():
        assert pr["split_launches"] == 3 == sum(count(thr)) and pr["split6_launches"] == 0, pr
        assert pr["nib_codes"] + pr["nib8_codes"] + pr["split5_codes"] == pr["split_codes"], pr
        for k in ("nib", "nib8", "split5"):
            assert (pr[k + "_survivors"] > 0) == (pr[k + "_launches"] > 0) == (pr[k + "_codes"] > 0), pr
    assert count((0, 0)) == (0, 0, 3) == count((1 << 40, 1 << 40))
    assert count((1, 0)) == (3, 0, 0) and count((0, 1)) == (0, 3, 0)
    # the runs have 393 216, 1 572 864 and 902 848 codes: only the second has 2^20, the first is below 2^19
    assert count((1 << 20, 0)) == (1, 0, 2)
    assert count((1, 1 << 20)) == (2, 1, 0) and count((1 << 19, 1 << 20)) == (1, 1, 1)
    for thr in res:
        for q in range(2):
            assert heaps_equal(res[thr][0]["heaps"][q], res[(0, 0)][0]["heaps"][q]), (thr, q)
