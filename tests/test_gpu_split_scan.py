"""GPU: the split form of the one-query-per-pass level scan (16x4 runs read from the byte-plane copy of code bytes 0-6,
byte 7 only for the survivors of the 7-byte bound).  Every comparison is heaps bit for bit: the
split forced at small sizes against the same index without the copy, and against the reference build."""
import numpy as np
import pytest

from helpers import float_tables, heaps_equal

pytestmark = pytest.mark.gpu
M = 16
ONE_QUERY_PER_PASS = dict(share_variant=0, mq=0, front_run_max=0, wgq=0)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def make_index(pyqadc, parts, split, labels=None, keep=0.01, **opts):
    idx = pyqadc.Index(M)
    for k, v in dict(ONE_QUERY_PER_PASS, **opts).items():
        idx.set_option(k, v)
    idx.set_split(1, 1) if split else idx.set_split(0, 1)
    idx.add_partitions(parts, labels)
    idx.finalize(keep)
    idx.set_option("profile", 1)
    return idx


def scan_pair(pyqadc, parts, tables, R, labels=None, assign=None, int8=False, **opts):
    """(split result, row-major result, split profile) of the same query batch on two indexes."""
    nq = tables.shape[0]
    assign = np.zeros((nq, 1), np.int32) if assign is None else assign
    out = []
    for split in (True, False):
        idx = make_index(pyqadc, parts, split, labels, **opts)
        res = idx.scan_i8(assign, tables, R) if int8 else idx.query_scan(assign, tables.copy(), R, want_qtables=True)
        pr = idx.profile()
        assert (pr["split_codes"] > 0) == split and (pr["split_copy_bytes"] > 0) == split, pr
        out.append((res, pr))
        idx.close()
    return out[0][0], out[1][0], out[0][1]


def ref_heap(po, parts, labels, qtables, R):
    inter = [po.ref_interleave(p) for p in parts]
    return po.ref_scan_interleaved(M, inter, [len(p) for p in parts], labels, qtables, R)


@pytest.mark.parametrize("variant", [0x0d, 0x01])                 # chunked tiles (default), grid-stride tiles
@pytest.mark.parametrize("n", [1_000_003, 786_432 + 16 * 7 + 5])   # a ragged last tile, n % 16 != 0
def test_split_matches_row_major_and_reference(pyqadc, po, n, variant):
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 3, 1, M)
    # the last code = the smallest sum query 0's tables allow: a sure candidate, emitted by the ragged end of a split run
    # together with its padding-lane replays
    best = tables[0, 0].reshape(M, 16).argmin(axis=1).astype(np.uint8)
    codes[-1] = best[0::2] | (best[1::2] << 4)
    R = 100
    a, b, pr = scan_pair(pyqadc, [codes], tables, R, variant=variant)
    assert pr["split_launches"] >= 2                       # [128 Ki, 512 Ki) and [512 Ki, n)
    reps = (16 - n % 16) % 16
    assert reps and np.count_nonzero(a["heaps"][0][0] == n - 1) == 1 + reps
    for q in range(3):
        assert heaps_equal(a["heaps"][q], b["heaps"][q]), q
        if po.have_ref():
            assert heaps_equal(a["heaps"][q], ref_heap(po, [codes], None, a["qtables"][q], R)), q


def test_split_with_labels_and_several_partitions(pyqadc, po):
    rng = np.random.default_rng(7)
    # Runs are cut at the level bounds of each query's concatenated order: partition 1 follows 700 001 (query 0) or 1 355 370
    # (query 1) codes, so its run behind the 2 Mi bound starts at local 1 397 150 / 741 782, off the copy's tiles, and is
    # longer than small_run: a long launch that keeps the row-major form next to the split ones.
    sizes = [700_001, 1_600_000, 16384 * 40 + 9]
    parts = [rng.integers(0, 256, (s, M // 2), dtype=np.uint8) for s in sizes]
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    nq, ma = 2, 3
    tables = float_tables(rng, nq, ma, M)
    assign = np.array([[0, 1, 2], [2, 0, 1]], np.int32)
    R = 64
    a, b, pr = scan_pair(pyqadc, parts, tables, R, labels=labels, assign=assign)
    assert 0 < pr["split_codes"] < pr["scan_codes"] and pr["split_launches"] < pr["scan_launches"], pr
    for q in range(nq):
        assert heaps_equal(a["heaps"][q], b["heaps"][q]), q
        if po.have_ref():
            order = [int(p) for p in assign[q]]
            want = ref_heap(po, [parts[p] for p in order], [labels[p] for p in order], a["qtables"][q], R)
            assert heaps_equal(a["heaps"][q], want), q


@pytest.mark.parametrize("p7", [0, 127])
def test_split_hand_made_int8_tables(pyqadc, po, p7):
    """Byte-7 pair entries all 0 (every 7-byte survivor is a candidate) or all 127 (none is)."""
    rng = np.random.default_rng(11 + p7)
    n = 900_017
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    qt = rng.integers(0, 40, (2, 1, M, 16), dtype=np.int8)
    qt[:, :, 14, :] = p7
    qt[:, :, 15, :] = 0
    R = 200
    a, b, _ = scan_pair(pyqadc, [codes], qt, R, int8=True)
    for q in range(2):
        assert heaps_equal(a[q], b[q]), q
        if po.have_ref():
            assert heaps_equal(a[q], ref_heap(po, [codes], None, qt[q], R)), q


def test_split_loose_bounds_and_region_overflow(pyqadc, po):
    """Large R: most codes need byte 7; a small candidate region overflows and the batch is re-run."""
    rng = np.random.default_rng(5)
    n = 600_000
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    R = 4000
    a, b, pr = scan_pair(pyqadc, [codes], tables, R, cand_capacity=256)
    assert pr["regrows"] >= 1, pr
    for q in range(2):
        assert heaps_equal(a["heaps"][q], b["heaps"][q]), q
        if po.have_ref():
            assert heaps_equal(a["heaps"][q], ref_heap(po, [codes], None, a["qtables"][q], R)), q


def test_split_on_a_shard(pyqadc, po):
    """A multi-rank shard (first_pos > 0): the copy's tiles start at the shard's first local code.  The shard's heap is the
    reference's heap over the shard's codes, keyed by global position."""
    rng = np.random.default_rng(9)
    gn, first = 2_000_005, 600_000
    codes = rng.integers(0, 256, (gn, M // 2), dtype=np.uint8)
    tables = float_tables(rng, 2, 1, M)
    res = []
    for split in (True, False):
        idx = pyqadc.Index(M)
        for k, v in ONE_QUERY_PER_PASS.items():
            idx.set_option(k, v)
        idx.set_split(1 if split else 0, 1)
        idx.add_partition_shard(codes[first:], first, gn, starts=codes[:gn // 100])
        idx.finalize(0.01)
        idx.set_option("profile", 1)
        res.append(idx.query_scan(np.zeros((2, 1), np.int32), tables.copy(), 100, want_qtables=True))
        assert (idx.profile()["split_codes"] > 0) == split
        idx.close()
    for q in range(2):
        assert heaps_equal(res[0]["heaps"][q], res[1]["heaps"][q]), q
        if po.have_ref():
            keys = [np.arange(first, gn, dtype=np.uint32)]
            assert heaps_equal(res[0]["heaps"][q], ref_heap(po, [codes[first:]], keys, res[0]["qtables"][q], 100)), q


def test_no_copy_when_disabled(pyqadc):
    idx = pyqadc.Index(M)
    idx.set_split(0, 1)
    idx.add_partition_synthetic(1 << 22, 3)
    idx.finalize(0.01)
    pr = idx.profile()
    assert pr["split_copy_bytes"] == 0 and pr["split_copy_failed"] == 0
    idx.close()
    idx = pyqadc.Index(M)
    idx.set_split(1 << 20, 1)
    idx.add_partition_synthetic(1 << 22, 3)
    idx.finalize(0.01)
    assert idx.profile()["split_copy_bytes"] == (1 << 22) * 7
    with pytest.raises(Exception):
        idx.set_split(0, 1)                                  # the copy is made at finalize
    idx.close()


def test_1e8_headline_mode_default_thresholds_against_reference(pyqadc, po):
    if not po.have_ref():
        pytest.skip("oracle/_ref not present")
    n, R, keep, seed = 100_000_000, 100, 0.01, 0x5EED0001
    idx = pyqadc.Index(M)
    for k, v in ONE_QUERY_PER_PASS.items():
        idx.set_option(k, v)
    idx.add_partition_synthetic(n, seed)
    idx.finalize(keep)
    idx.set_option("profile", 1)
    rng = np.random.default_rng(3)
    nq = 4
    tables = float_tables(rng, nq, 1, M)
    res = idx.query_scan(np.zeros((nq, 1), np.int32), tables.copy(), R, want_qtables=True)
    pr = idx.profile()
    assert pr["split_copy_bytes"] > 0 and pr["split_launches"] > 0 and pr["split_codes"] > 0, pr
    inter = po.ref_interleave(po.fill_codes(0, n, seed).reshape(n, 8))
    for q in range(nq):
        want = po.ref_scan_interleaved(M, [inter], [n], None, res["qtables"][q], R)
        assert heaps_equal(res["heaps"][q], want), q
    idx.close()
