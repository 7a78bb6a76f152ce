"""GPU: the 6-plane form of the split scan: 6 of the 7 planes of the byte-plane copy are streamed, the
query table's "cheapest" byte j (smallest pair-entry sum, ties: the highest j) and byte 7 are read from the row-major codes
for the survivors of the 6-byte bound only.  Every comparison is heaps bit for bit (keys, values, sizes, status): the
6-plane form forced at small sizes against the same index with 7 planes, with the row-major form, and against the
reference build."""
import numpy as np
import pytest

from helpers import float_tables, heaps_equal

pytestmark = pytest.mark.gpu
M = 16
ONE_QUERY_PER_PASS = dict(share_variant=0, mq=0, front_run_max=0, wgq=0)
FORMS = ("split6", "split7", "rows")


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def make_index(pyqadc, parts, form, labels=None, keep=0.01, **opts):
    idx = pyqadc.Index(M)
    for k, v in dict(ONE_QUERY_PER_PASS, **opts).items():
        idx.set_option(k, v)
    idx.set_split(0, 1) if form == "rows" else idx.set_split(1, 1)
    idx.set_split6(1 if form == "split6" else 0)
    idx.add_partitions(parts, labels)
    idx.finalize(keep)
    idx.set_option("profile", 1)
    return idx


def scan_forms(pyqadc, parts, tables, R, labels=None, assign=None, int8=False, **opts):
    """{form: (result, profile)} of the same query batch on three indexes: 6 planes, 7 planes, row-major."""
    nq = tables.shape[0]
    assign = np.zeros((nq, 1), np.int32) if assign is None else assign
    out = {}
    for form in FORMS:
        idx = make_index(pyqadc, parts, form, labels, **opts)
        res = idx.scan_i8(assign, tables, R) if int8 else idx.query_scan(assign, tables.copy(), R, want_qtables=True)
        pr = idx.profile()
        assert (pr["split_codes"] > 0) == (form != "rows"), pr
        assert (pr["split6_codes"] > 0) == (form == "split6") and (pr["split6_launches"] > 0) == (form == "split6"), pr
        assert pr["split6_codes"] <= pr["split_codes"] and pr["split6_launches"] <= pr["split_launches"], pr
        if form != "split6":
            assert pr["split_survivors"] == 0, pr
        out[form] = (res, pr)
        idx.close()
    return out


def result_heaps(res, q, int8):
    return res[q] if int8 else res["heaps"][q]


def assert_same(out, nq, int8, R):
    """Heaps, sizes and status of the 6-plane form against the two other forms."""
    a = out["split6"][0]
    for other in ("split7", "rows"):
        b = out[other][0]
        for q in range(nq):
            ha, hb = result_heaps(a, q, int8), result_heaps(b, q, int8)
            assert ha[0].shape == hb[0].shape and heaps_equal(ha, hb), (other, q)
        if not int8:
            assert np.array_equal(a["status"], b["status"]), other


def ref_heap(po, parts, labels, qtables, R):
    inter = [po.ref_interleave(p) for p in parts]
    return po.ref_scan_interleaved(M, inter, [len(p) for p in parts], labels, qtables, R)


def small_plane_tables(rng, nq, j, hi=40):
    """int8 tables whose pair of sub-quantizers (2 j, 2 j + 1) has uniformly small entries: the rule picks byte j."""
    qt = rng.integers(8, hi, (nq, 1, M, 16), dtype=np.int8)
    qt[:, :, 2 * j, :] = rng.integers(0, 3, (nq, 1, 16), dtype=np.int8)
    qt[:, :, 2 * j + 1, :] = rng.integers(0, 3, (nq, 1, 16), dtype=np.int8)
    return qt


def expected_choice(qt):
    """The rule of DESIGN.md 3.1 on one [M][16] int8 table: the j in 0..6 with the smallest pair-entry sum, ties: the highest."""
    t = qt.reshape(M, 16).astype(np.int64)
    sums = [int((t[2 * j][None, :] + t[2 * j + 1][:, None]).sum()) for j in range(7)]
    return max(j for j in range(7) if sums[j] == min(sums))


@pytest.mark.parametrize("variant", [0x0d, 0x01])                 # chunked tiles (default), grid-stride tiles
@pytest.mark.parametrize("n", [1_000_003, 786_432 + 16 * 7 + 5])   # a ragged last tile, n % 16 != 0
def test_split6_matches_split7_row_major_and_reference(pyqadc, po, n, variant):
    rng = np.random.default_rng(n + 1)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 3, 1, M)
    # the last code = the smallest sum query 0's tables allow: a sure candidate, emitted by the ragged end of a run together
    # with its padding-lane replays
    best = tables[0, 0].reshape(M, 16).argmin(axis=1).astype(np.uint8)
    codes[-1] = best[0::2] | (best[1::2] << 4)
    R = 100
    out = scan_forms(pyqadc, [codes], tables, R, variant=variant)
    a, pr = out["split6"]
    assert pr["split6_launches"] >= 2                      # [128 Ki, 512 Ki) and [512 Ki, n)
    assert 0 < pr["split_survivors"] <= pr["split6_codes"], pr
    reps = (16 - n % 16) % 16
    assert reps and np.count_nonzero(a["heaps"][0][0] == n - 1) == 1 + reps
    assert_same(out, 3, False, R)
    if po.have_ref():
        for q in range(3):
            assert heaps_equal(a["heaps"][q], ref_heap(po, [codes], None, a["qtables"][q], R)), q


@pytest.mark.parametrize("R", [1, 9_000, 10_003, 11_000])          # around the number of starts (10 000)
def test_split6_R_around_the_starts(pyqadc, po, R):
    rng = np.random.default_rng(R)
    n = 1_000_003
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    out = scan_forms(pyqadc, [codes], tables, R)
    assert_same(out, 2, False, R)
    a = out["split6"][0]
    # more neighbours than starts: the pre-scan's heap never fills, qmax stays FLT_MAX and the query is skipped with a status
    # (where the reference exits); the three forms agree on that above, and there is no reference heap to compare
    assert np.all((a["status"] == 0) == (R <= 10_000)), a["status"]
    if po.have_ref():
        for q in range(2):
            if a["status"][q] == 0:
                assert heaps_equal(a["heaps"][q], ref_heap(po, [codes], None, a["qtables"][q], R)), q


def test_split6_with_labels_and_several_partitions(pyqadc, po):
    rng = np.random.default_rng(17)
    sizes = [700_001, 1_600_000, 16384 * 40 + 9]
    parts = [rng.integers(0, 256, (s, M // 2), dtype=np.uint8) for s in sizes]
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    nq, ma = 2, 3
    tables = float_tables(rng, nq, ma, M)
    assign = np.array([[0, 1, 2], [2, 0, 1]], np.int32)
    R = 64
    out = scan_forms(pyqadc, parts, tables, R, labels=labels, assign=assign)
    a, pr = out["split6"]
    assert 0 < pr["split6_codes"] < pr["scan_codes"], pr
    assert_same(out, nq, False, R)
    if po.have_ref():
        for q in range(nq):
            order = [int(p) for p in assign[q]]
            want = ref_heap(po, [parts[p] for p in order], [labels[p] for p in order], a["qtables"][q], R)
            assert heaps_equal(a["heaps"][q], want), q


@pytest.mark.parametrize("j", range(7))
def test_split6_every_deferred_plane(pyqadc, po, j):
    """Caller tables built so that the rule defers byte j (scan_i8: the choice is made by a kernel of its own)."""
    rng = np.random.default_rng(100 + j)
    n = 900_017
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = small_plane_tables(rng, 2, j)
    assert all(expected_choice(qt[q, 0]) == j for q in range(2))
    R = 150
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert out["split6"][1]["split6_codes"] > 0
    assert_same(out, 2, True, R)
    if po.have_ref():
        for q in range(2):
            assert heaps_equal(out["split6"][0][q], ref_heap(po, [codes], None, qt[q], R)), q


def test_split6_choices_differ_inside_one_launch(pyqadc, po):
    """32 queries in one launch, every deferred byte 0..6 among them; and float tables (the quantizer makes the choice)."""
    rng = np.random.default_rng(32)
    n = 600_011
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    nq = 32
    qt = np.concatenate([small_plane_tables(rng, 1, q % 7) for q in range(nq)])
    assert sorted({expected_choice(qt[q, 0]) for q in range(nq)}) == list(range(7))
    R = 50
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, nq, True, R)
    if po.have_ref():
        for q in (0, 5, 13, 31):
            assert heaps_equal(out["split6"][0][q], ref_heap(po, [codes], None, qt[q], R)), q
    tables = float_tables(rng, nq, 1, M)
    for q in range(nq):                                      # float tables with one cheap pair of sub-quantizers each
        tables[q, 0].reshape(M, 16)[2 * (q % 7):2 * (q % 7) + 2] *= np.float32(0.02)
    out = scan_forms(pyqadc, [codes], tables, R)
    a = out["split6"][0]
    assert {expected_choice(np.asarray(a["qtables"][q]).reshape(-1, M, 16)[0]) for q in range(nq)} == set(range(7))
    assert_same(out, nq, False, R)
    if po.have_ref():
        for q in (1, 9, 20, 30):
            assert heaps_equal(a["heaps"][q], ref_heap(po, [codes], None, a["qtables"][q], R)), q


@pytest.mark.parametrize("streamed", [0, 127])
def test_split6_every_code_or_no_code_survives(pyqadc, po, streamed):
    """Bytes 0-6 all 0: all seven tie, the rule defers the highest (6), the 6-byte partial is 0 and byte 7's pair entries are
    >= 2, so the bound never reaches 0: every code is a survivor and the result is decided by the deferred bytes alone.
    Streamed bytes all 127 (byte 3, the cheapest, deferred): min(127, partial) = 127 is never below a bound: no survivor."""
    rng = np.random.default_rng(200 + streamed)
    n = 500_009
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = np.full((2, 1, M, 16), streamed, np.int8)
    qt[:, :, 14:16, :] = rng.integers(1, 60, (2, 1, 2, 16), dtype=np.int8)
    if streamed:
        qt[:, :, 6:8, :] = rng.integers(0, 20, (2, 1, 2, 16), dtype=np.int8)
    assert all(expected_choice(qt[q, 0]) == (3 if streamed else 6) for q in range(2))
    R = 300
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    pr = out["split6"][1]
    assert pr["regrows"] == 0, pr
    assert pr["split_survivors"] == (0 if streamed else pr["split6_codes"]), pr
    assert_same(out, 2, True, R)
    if po.have_ref():
        for q in range(2):
            assert heaps_equal(out["split6"][0][q], ref_heap(po, [codes], None, qt[q], R)), q


def test_split6_tie_heavy_tables(pyqadc, po):
    """Two distinct entry values only: thousands of codes share every sum, the heap's content is decided by scan order."""
    rng = np.random.default_rng(41)
    n = 800_021
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = (rng.integers(0, 2, (3, 1, M, 16)) * 9).astype(np.int8)
    R = 500
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, 3, True, R)
    if po.have_ref():
        for q in range(3):
            assert heaps_equal(out["split6"][0][q], ref_heap(po, [codes], None, qt[q], R)), q


@pytest.mark.parametrize("where", ["streamed", "deferred", "both"])
def test_split6_saturation(pyqadc, po, where):
    """Entries of 127: partial sums and full sums above 127, min(127, .) on both sides of the comparison with the bound."""
    rng = np.random.default_rng({"streamed": 51, "deferred": 52, "both": 53}[where])
    n = 700_003
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = rng.integers(0, 25, (2, 1, M, 16), dtype=np.int8)
    qt[:, :, 10:12, :] = rng.integers(0, 4, (2, 1, 2, 16), dtype=np.int8)     # byte 5 is the deferred one
    big = rng.random((2, 1, M, 16)) < 0.3
    if where == "streamed":
        big[:, :, 10:12, :] = False
        big[:, :, 14:16, :] = False
    elif where == "deferred":
        big[:, :, 0:14, :] = False
    else:
        big[:, :, 10:12, :] = False
    qt[big] = 127
    if where != "streamed":
        qt[:, :, 10, 3] = 127                                # (one entry per row: byte 5 stays the cheapest)
        qt[:, :, 11, 9] = 127
    assert all(expected_choice(qt[q, 0]) == 5 for q in range(2))
    R = 400
    out = scan_forms(pyqadc, [codes], qt, R, int8=True)
    assert_same(out, 2, True, R)
    if po.have_ref():
        for q in range(2):
            assert heaps_equal(out["split6"][0][q], ref_heap(po, [codes], None, qt[q], R)), q


def test_split6_loose_bounds_and_region_overflow(pyqadc, po):
    """Large R: most codes survive; a small candidate region overflows and the batch is re-run (the existing fallback)."""
    rng = np.random.default_rng(6)
    n = 600_000
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    R = 4000
    out = scan_forms(pyqadc, [codes], tables, R, cand_capacity=256)
    assert out["split6"][1]["regrows"] >= 1, out["split6"][1]
    assert_same(out, 2, False, R)
    if po.have_ref():
        a = out["split6"][0]
        for q in range(2):
            assert heaps_equal(a["heaps"][q], ref_heap(po, [codes], None, a["qtables"][q], R)), q


def test_split6_threshold_picks_the_form_per_launch(pyqadc):
    """set_split6(min_run6): only launches whose runs all have min_run6 codes take the 6-plane form; 0 = never."""
    rng = np.random.default_rng(8)
    n = 3_000_000                                            # levels [128 Ki, 512 Ki), [512 Ki, 2 Mi), [2 Mi, n)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    res = {}
    for min6 in (0, 1, 1 << 20, 1 << 40):
        idx = make_index(pyqadc, [codes], "split7")
        idx.set_split6(min6)
        res[min6] = (idx.query_scan(np.zeros((2, 1), np.int32), tables.copy(), 100), idx.profile())
        idx.close()
    assert res[0][1]["split6_launches"] == 0 and res[1 << 40][1]["split6_launches"] == 0
    assert res[1][1]["split6_launches"] == res[1][1]["split_launches"] > 0
    assert 0 < res[1 << 20][1]["split6_launches"] < res[1][1]["split6_launches"]
    for min6 in (1, 1 << 20, 1 << 40):
        for q in range(2):
            assert heaps_equal(res[min6][0]["heaps"][q], res[0][0]["heaps"][q]), (min6, q)
