"""GPU: the 5-plane form of the split scan: 5 of the 7 planes of the byte-plane copy are streamed; two
bytes j1 < j2 of 0..6 (the two whose pair entries rise least above their minimum, ties: the highest j) and byte 7 are read from
the row-major codes for the survivors only, and a survivor is a code whose 5-byte partial sum is below bound - c, c = min(127,
the three deferred pair tables' minima summed).  Every comparison is heaps bit for bit (keys, values, sizes, status): the 5-plane
form forced at small sizes against the same index with 6 planes, 7 planes and the row-major form, and against the reference
build.  A c above the true minimum would lose candidates (the heaps differ); a c below it shows in the survivor counts of the
slack-edge cases."""
import numpy as np
import pytest

from helpers import float_tables, heaps_equal

pytestmark = pytest.mark.gpu
M = 16
ONE_QUERY_PER_PASS = dict(share_variant=0, mq=0, front_run_max=0, wgq=0)
FORMS = ("split5", "split6", "split7", "rows")
PAIRS = [(a, b) for a in range(7) for b in range(a + 1, 7)]


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def make_index(pyqadc, parts, form, labels=None, keep=0.01, **opts):
    idx = pyqadc.Index(M)
    for k, v in dict(ONE_QUERY_PER_PASS, **opts).items():
        idx.set_option(k, v)
    idx.set_split(0, 1) if form == "rows" else idx.set_split(1, 1)
    idx.set_split6(1 if form in ("split5", "split6") else 0)     # (5 planes are preferred where both thresholds are met)
    idx.set_split5(1 if form == "split5" else 0)
    idx.add_partitions(parts, labels)
    idx.finalize(keep)
    idx.set_option("profile", 1)
    return idx


def scan_forms(pyqadc, parts, tables, R, labels=None, assign=None, int8=False, **opts):
    """{form: (result, profile)} of the same query batch on four indexes: 5, 6, 7 planes, row-major."""
    nq = tables.shape[0]
    assign = np.zeros((nq, 1), np.int32) if assign is None else assign
    out = {}
    for form in FORMS:
        idx = make_index(pyqadc, parts, form, labels, **opts)
        res = idx.scan_i8(assign, tables, R) if int8 else idx.query_scan(assign, tables.copy(), R, want_qtables=True)
        pr = idx.profile()
        assert (pr["split_codes"] > 0) == (form != "rows"), pr
        assert (pr["split5_codes"] > 0) == (form == "split5") and (pr["split5_launches"] > 0) == (form == "split5"), pr
        assert (pr["split6_codes"] > 0) == (form == "split6") and (pr["split6_launches"] > 0) == (form == "split6"), pr
        assert pr["split5_codes"] + pr["split6_codes"] <= pr["split_codes"], pr
        assert pr["split5_launches"] + pr["split6_launches"] <= pr["split_launches"], pr
        assert pr["split5_survivors"] <= pr["split5_codes"], pr
        if form != "split5":
            assert pr["split5_survivors"] == 0, pr
        if form != "split6":
            assert pr["split_survivors"] == 0, pr
        out[form] = (res, pr)
        idx.close()
    return out


def result_heaps(res, q, int8):
    return res[q] if int8 else res["heaps"][q]


def assert_same(out, nq, int8, R):
    """Heaps, sizes and status of the 5-plane form against the three other forms."""
    a = out["split5"][0]
    for other in FORMS[1:]:
        b = out[other][0]
        for q in range(nq):
            ha, hb = result_heaps(a, q, int8), result_heaps(b, q, int8)
            assert ha[0].shape == hb[0].shape and heaps_equal(ha, hb), (other, q)
        if not int8:
            assert np.array_equal(a["status"], b["status"]), other


def assert_reference(po, out, parts, labels, qt, queries, R, int8=True):
    if not po.have_ref():
        return
    a = out["split5"][0]
    inter = [po.ref_interleave(p) for p in parts]
    for q in queries:
        tab = qt[q] if int8 else a["qtables"][q]
        want = po.ref_scan_interleaved(M, inter, [len(p) for p in parts], labels, tab, R)
        assert heaps_equal(result_heaps(a, q, int8), want), q


def expected_choice5(qt):
    """The rule of DESIGN.md 3.1 on one [M][16] int8 table -> (j1, j2, c): score_j = the two rows' sum - 16 (min row 2j + min
    row 2j+1) for j in 0..6; the smallest score is picked, ties: the highest j, then again among the rest; c = min(127, the sum of
    min P over the two picks and byte 7)."""
    t = qt.reshape(M, 16).astype(np.int64)
    minp = [int(t[2 * j].min() + t[2 * j + 1].min()) for j in range(8)]
    score = [int(t[2 * j].sum() + t[2 * j + 1].sum()) - 16 * minp[j] for j in range(7)]
    a = max(j for j in range(7) if score[j] == min(score))
    rest = [j for j in range(7) if j != a]
    b = max(j for j in rest if score[j] == min(score[r] for r in rest))
    j1, j2 = min(a, b), max(a, b)
    return j1, j2, min(127, minp[j1] + minp[j2] + minp[7])


def pair_tables(rng, nq, pair, flat):
    """int8 tables for which the rule defers the bytes of `pair`.  flat: their four rows hold 18..20 only (almost no spread: small
    scores, and minima of 36+ per pair table, so c is large but stays below the clamp); else 0..2 (c near 0).  The other rows
    spread over 0..13 (flat) or 8..39."""
    qt = rng.integers(0, 14, (nq, 1, M, 16), dtype=np.int8) if flat else rng.integers(8, 40, (nq, 1, M, 16), dtype=np.int8)
    for j in pair:
        qt[:, :, 2 * j:2 * j + 2, :] = rng.integers(18, 21, (nq, 1, 2, 16), dtype=np.int8) if flat else \
            rng.integers(0, 3, (nq, 1, 2, 16), dtype=np.int8)
    if not flat:
        qt[:, :, 14:16, :] = rng.integers(0, 32, (nq, 1, 2, 16), dtype=np.int8)      # byte 7's minimum near 0 as well
    return qt


def saturation_tables(rng, where):
    """Entries of 127 in the streamed rows, the deferred rows (bytes 2, 5 and 7) or both; bytes 2 and 5 stay the rule's choice
    (one 127 per row there: the score rises by 127 a row, the others' spread is wider)."""
    qt = rng.integers(8, 48, (2, 1, M, 16), dtype=np.int8)
    for j in (2, 5):
        qt[:, :, 2 * j:2 * j + 2, :] = rng.integers(0, 4, (2, 1, 2, 16), dtype=np.int8)
    big = rng.random((2, 1, M, 16)) < 0.3
    big[:, :, 4:6, :] = False
    big[:, :, 10:12, :] = False
    if where == "streamed":
        big[:, :, 14:16, :] = False
    elif where == "deferred":
        big[:, :, 0:14, :] = False
    qt[big] = 127
    if where != "streamed":
        for r, i in ((4, 3), (5, 9), (10, 1), (11, 12)):
            qt[:, :, r, i] = 127
    return qt


def edge_tables(rng, case):
    """The slack-edge tables.  All of bytes 0..6 have constant rows (score 0), so the rule defers the two highest: 5 and 6."""
    qt = np.zeros((2, 1, M, 16), np.int8)
    if case == "clamp":                 # deferred rows constant 127: c clamps at 127, bsurv = 0
        qt[:, :, 0:10, :] = 3
        qt[:, :, 10:16, :] = 127
    elif case == "c0":                  # streamed rows 0, every deferred row holds a 0: c = 0, partial 0 < bound always
        qt[:, :, 14:16, :] = rng.integers(1, 60, (2, 1, 2, 16), dtype=np.int8)
        qt[:, :, 14:16, 0] = 0
    elif case == "reach":               # streamed rows 0, deferred minima >= 1: the bound comes down to c and the survivors stop
        qt[:, :, 10:14, :] = 1
        qt[:, :, 14:16, :] = rng.integers(1, 30, (2, 1, 2, 16), dtype=np.int8)
    else:                               # "sat": streamed rows 127: min(127, partial) is never below a bound
        qt[:, :, 0:10, :] = 127
        qt[:, :, 14:16, :] = rng.integers(1, 60, (2, 1, 2, 16), dtype=np.int8)
    return qt


@pytest.mark.parametrize("variant", [0x0d, 0x01])                 # chunked tiles (default), grid-stride tiles
@pytest.mark.parametrize("n", [1_000_003, 786_432 + 16 * 7 + 5])   # a ragged last tile, n % 16 != 0
def test_split5_matches_the_other_forms_and_reference(pyqadc, po, n, variant):
    rng = np.random.default_rng(n + 1)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 3, 1, M)
    # the last code = the smallest sum query 0's tables allow: a sure candidate, emitted by the ragged end of a run together
    # with its padding-lane replays
    best = tables[0, 0].reshape(M, 16).argmin(axis=1).astype(np.uint8)
    codes[-1] = best[0::2] | (best[1::2] << 4)
    R = 100
    out = scan_forms(pyqadc, [codes], tables, R, variant=variant)
    a, pr = out["split5"]
    assert pr["split5_launches"] >= 2                      # [128 Ki, 512 Ki) and [512 Ki, n)
    assert pr["split5_launches"] == pr["split_launches"] and pr["split5_codes"] == pr["split_codes"], pr
    assert 0 < pr["split5_survivors"] <= pr["split5_codes"], pr
    reps = (16 - n % 16) % 16
    assert reps and np.count_nonzero(a["heaps"][0][0] == n - 1) == 1 + reps
    assert_same(out, 3, False, R)
    assert_reference(po, out, [codes], None, None, range(3), R, int8=False)


@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("pair", PAIRS)
def test_split5_every_deferred_pair(pyqadc, po, pair, flat):
    """Caller tables built so that the rule defers the pair (scan_i8: the choice is made by a kernel of its own)."""
    rng = np.random.default_rng(1000 + 10 * pair[0] + pair[1] + 100 * flat)
    n = 300_007
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = pair_tables(rng, 2, pair, flat)
    for q in range(2):
        j1, j2, c = expected_choice5(qt[q, 0])
        assert (j1, j2) == pair and (36 * 2 <= c < 127 if flat else c <= 16), (j1, j2, c)
    R = 150
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    pr = out["split5"][1]
    assert pr["split5_codes"] > 0 and pr["split5_survivors"] < pr["split5_codes"], pr
    assert_same(out, 2, True, R)
    assert_reference(po, out, [codes], None, qt, range(2), R)


def test_split5_choices_differ_inside_one_launch(pyqadc, po):
    """32 queries in one launch whose pairs cover every byte 0..6; and float tables (the quantizer makes the choice)."""
    rng = np.random.default_rng(32)
    n = 600_011
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    nq = 32
    pairs = [(0, 1), (2, 3), (4, 5), (5, 6), (0, 6), (1, 4), (2, 6), (3, 5)]
    qt = np.concatenate([pair_tables(rng, 1, pairs[q % 8], q % 2 == 0) for q in range(nq)])
    assert [expected_choice5(qt[q, 0])[:2] for q in range(nq)] == [pairs[q % 8] for q in range(nq)]
    R = 50
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, nq, True, R)
    assert_reference(po, out, [codes], None, qt, (0, 5, 13, 31), R)
    tables = float_tables(rng, nq, 1, M)
    for q in range(nq):                                      # float tables with two cheap pairs of sub-quantizers each
        for j in pairs[q % 8]:
            tables[q, 0].reshape(M, 16)[2 * j:2 * j + 2] *= np.float32(0.02)
    out = scan_forms(pyqadc, [codes], tables, R)
    a = out["split5"][0]
    chosen = [expected_choice5(np.asarray(a["qtables"][q]).reshape(-1, M, 16)[0])[:2] for q in range(nq)]
    assert {j for p in chosen for j in p} == set(range(7)) and len(set(chosen)) >= 4, chosen
    assert_same(out, nq, False, R)
    assert_reference(po, out, [codes], None, None, (1, 9, 20, 30), R, int8=False)


@pytest.mark.parametrize("case", ["clamp", "c0", "reach", "sat"])
def test_split5_slack_edges(pyqadc, po, case):
    rng = np.random.default_rng({"clamp": 300, "c0": 301, "reach": 302, "sat": 303}[case])
    n = 500_009
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = edge_tables(rng, case)
    if case == "c0":
        codes[:, 7] |= 1                                     # byte 7 never meets both zeros: every sum is >= 1 and so is every bound
    R = 50 if case == "reach" else 300
    for q in range(2):
        j1, j2, c = expected_choice5(qt[q, 0])
        assert (j1, j2) == (5, 6), (j1, j2)
        assert {"clamp": c == 127, "c0": c == 0, "reach": 6 <= c < 127, "sat": 2 <= c < 127}[case], c
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    pr = out["split5"][1]
    assert pr["regrows"] == 0, pr
    if case in ("clamp", "sat"):
        assert pr["split5_survivors"] == 0, pr
    elif case == "c0":
        assert pr["split5_survivors"] == pr["split5_codes"], pr
    else:
        # some 2 000 codes per query have the smallest sum there is (= c); with R = 50 the bound is down at c before the long
        # levels end, and from then on no code survives.  A c one too small would keep every code a survivor.
        assert pr["split5_survivors"] < pr["split5_codes"], pr
    assert_same(out, 2, True, R)
    assert_reference(po, out, [codes], None, qt, range(2), R)


@pytest.mark.parametrize("where", ["streamed", "deferred", "both"])
def test_split5_saturation(pyqadc, po, where):
    """Entries of 127: partial sums and full sums above 127, min(127, .) on both sides of the comparison with the bound."""
    rng = np.random.default_rng({"streamed": 51, "deferred": 52, "both": 53}[where])
    n = 700_003
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = saturation_tables(rng, where)
    assert all(expected_choice5(qt[q, 0])[:2] == (2, 5) for q in range(2))
    R = 400
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, 2, True, R)
    assert_reference(po, out, [codes], None, qt, range(2), R)


def test_split5_tie_heavy_tables(pyqadc, po):
    """Two distinct entry values only: thousands of codes share every sum, the heap's content is decided by scan order."""
    rng = np.random.default_rng(41)
    n = 800_021
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = (rng.integers(0, 2, (3, 1, M, 16)) * 9).astype(np.int8)
    R = 500
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, 3, True, R)
    assert_reference(po, out, [codes], None, qt, range(3), R)


@pytest.mark.parametrize("R", [1, 9_000, 10_003, 11_000])          # around the number of starts (10 000)
def test_split5_R_around_the_starts(pyqadc, po, R):
    rng = np.random.default_rng(R)
    n = 1_000_003
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    out = scan_forms(pyqadc, [codes], tables, R)
    assert_same(out, 2, False, R)
    a = out["split5"][0]
    # more neighbours than starts: the pre-scan's heap never fills, qmax stays FLT_MAX and the query is skipped with a status
    # (where the reference exits); the forms agree on that above, and there is no reference heap to compare
    assert np.all((a["status"] == 0) == (R <= 10_000)), a["status"]
    assert_reference(po, out, [codes], None, None, [q for q in range(2) if a["status"][q] == 0], R, int8=False)


def test_split5_with_labels_and_several_partitions(pyqadc, po):
    rng = np.random.default_rng(17)
    sizes = [700_001, 1_600_000, 16384 * 40 + 9]
    parts = [rng.integers(0, 256, (s, M // 2), dtype=np.uint8) for s in sizes]
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    nq, ma = 2, 3
    tables = float_tables(rng, nq, ma, M)
    assign = np.array([[0, 1, 2], [2, 0, 1]], np.int32)
    R = 64
    out = scan_forms(pyqadc, parts, tables, R, labels=labels, assign=assign)
    a, pr = out["split5"]
    assert 0 < pr["split5_codes"] < pr["scan_codes"], pr
    assert_same(out, nq, False, R)
    if po.have_ref():
        for q in range(nq):
            order = [int(p) for p in assign[q]]
            inter = [po.ref_interleave(parts[p]) for p in order]
            want = po.ref_scan_interleaved(M, inter, [len(parts[p]) for p in order], [labels[p] for p in order], a["qtables"][q], R)
            assert heaps_equal(a["heaps"][q], want), q


def test_split5_loose_bounds_and_region_overflow(pyqadc, po):
    """Large R: most codes survive; a small candidate region overflows and the batch is re-run (the existing fallback)."""
    rng = np.random.default_rng(6)
    n = 600_000
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    R = 4000
    out = scan_forms(pyqadc, [codes], tables, R, cand_capacity=256)
    assert out["split5"][1]["regrows"] >= 1, out["split5"][1]
    assert_same(out, 2, False, R)
    assert_reference(po, out, [codes], None, None, range(2), R, int8=False)


def test_split5_threshold_picks_the_form_per_launch(pyqadc):
    """set_split5(min_run5): only launches whose runs all have min_run5 codes take the 5-plane form, the others of this index
    (set_split6(1)) the 6-plane form; 0 = never.  A launch is counted under split5_* or split6_*, never both."""
    rng = np.random.default_rng(8)
    n = 3_000_000                                            # levels [128 Ki, 512 Ki), [512 Ki, 2 Mi), [2 Mi, n)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    res = {}
    for min5 in (0, 1, 1 << 20, 1 << 40):
        idx = make_index(pyqadc, [codes], "split6")
        idx.set_split5(min5)
        res[min5] = (idx.query_scan(np.zeros((2, 1), np.int32), tables.copy(), 100), idx.profile())
        idx.close()
    for min5, (_, pr) in res.items():
        assert pr["split5_launches"] <= pr["split_launches"], pr
        assert pr["split5_launches"] + pr["split6_launches"] == pr["split_launches"] > 0, pr
        assert pr["split5_codes"] + pr["split6_codes"] == pr["split_codes"], pr
        assert (pr["split5_survivors"] > 0) == (pr["split5_launches"] > 0) and (pr["split_survivors"] > 0) == (pr["split6_launches"] > 0), pr
    assert res[0][1]["split5_launches"] == 0 and res[1 << 40][1]["split5_launches"] == 0
    assert res[1][1]["split5_launches"] == res[1][1]["split_launches"]
    assert 0 < res[1 << 20][1]["split5_launches"] < res[1][1]["split5_launches"]
    for min5 in (1, 1 << 20, 1 << 40):
        for q in range(2):
            assert heaps_equal(res[min5][0]["heaps"][q], res[0][0]["heaps"][q]), (min5, q)
