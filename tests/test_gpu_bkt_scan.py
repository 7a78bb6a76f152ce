"""GPU: the bucket form of the split scan: the run is streamed from a copy in which every block of
bkt_block codes is grouped by the codes' first two bytes, so sub-quantizers 0-3 come from a 2-byte id per 16 slots and NSP = 4, 5,
6 or 7 of the other 12 are paid for; the rest is read from the slot's 8-byte code for survivors only, and a candidate's position
comes from perm.  Every comparison is heaps bit for bit (keys, values, sizes, status): the bucket form forced at lists of a few
tiles (bkt_block = one or two tiles, bkt_max_pad lifted) against the same index's row-major form and against the CPU oracle
(po.query_scan); the copy itself is read back and checked against the numpy model (tests/bkt_model.py).

The planted list (planted_list): three blocks and a ragged 37-code end.  Block 0 has buckets of 1, 15, 16 and 17 codes among
larger ones; the bucket of 1 is query 0's best code (the bucket's last code: its 15 padding copies must not be emitted), the
bucket of 16 is one lane group of near-duplicates of it (several survivors in one lane).  Block 1 is one single key (its only
bucket ends exactly on the tile), block 2 has 16384 distinct keys (16 times the slots: the lifted pad limit), and the
partition's last code is the best code again (a candidate with its padding-lane replays, dup_pos).

The second half of the file is the nibble form's set of kernel edges (tests/test_gpu_nib_scan.py) under the bucket rule, each for
NSP = 4, 5, 6 and 7: both loop forms and one workgroup per run, every paid sub-quantizer in every role in one launch, masks chosen
by the quantizer, the slack edges, entries of 127, tie-heavy tables, R around the starts, the region overflow and its re-run,
the keys 0x0000 and 0xffff and a bucket across a tile boundary, and the thresholds that pick NSP per launch.  The copy across
index lives: tests/test_gpu_bkt_lifecycle.py."""
import os
import sys

import numpy as np
import pytest

import bkt_model
from helpers import float_tables, heaps_equal

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bucket_survivors as bs  # noqa: E402  (the numpy twin of the choice rule: choose_bkt)

pytestmark = pytest.mark.gpu
M = 16
TILE = 16384
ONE_QUERY_PER_PASS = dict(share_variant=0, mq=0, front_run_max=0, wgq=0)
TINY = dict(head_level=0, small_run=1, level_base=16384)    # lists of a few tiles: every level is a streaming launch on tiles
NSPS = (4, 5, 6, 7)
KEEPS = (0.01, 0.05)
R = 100


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def make_index(pyqadc, parts, form, labels=None, keep=0.01, block=TILE, **opts):
    """form: "rows", or NSP = 4..7 (the bucket form with that many paid planes from one code on; runs it cannot take: 9 nibble planes)."""
    idx = pyqadc.Index(M)
    for k, v in dict(ONE_QUERY_PER_PASS, **dict(TINY, **opts)).items():
        idx.set_option(k, v)
    idx.set_split(0, 1) if form == "rows" else idx.set_split(1, 1)
    idx.set_split6(0 if form == "rows" else 1)
    idx.set_split5(0 if form == "rows" else 1)
    idx.set_split_nib(0 if form == "rows" else 1, 0, 9)
    if form == "rows":
        idx.set_split_bkt(0)
    else:
        idx.set_split_bkt(1, block, int(form == 6), int(form == 5), int(form == 4), 1e6)
    idx.add_partitions(parts, labels)
    idx.finalize(keep)
    idx.set_option("profile", 1)
    return idx


def check_profile(pr, form, all_bkt=True, nib_copy=False):
    assert (pr["split_codes"] > 0) == (form != "rows"), pr
    assert (pr["bkt_copy_bytes"] > 0) == (form != "rows") and pr["bkt_copy_failed"] == pr["bkt_copy_padded_out"] == 0, pr
    # every split launch is counted under exactly one form
    assert pr["bkt_launches"] + pr["nib_launches"] + pr["nib8_launches"] + pr["split5_launches"] + pr["split6_launches"] == pr["split_launches"], pr
    assert pr["bkt_codes"] + pr["nib_codes"] + pr["nib8_codes"] + pr["split5_codes"] + pr["split6_codes"] == pr["split_codes"], pr
    if form == "rows":
        assert pr["bkt_launches"] == pr["bkt_survivors"] == 0, pr
    else:
        assert pr["bkt_launches"] > 0 and pr["bkt_codes"] <= pr["bkt_slots"] and pr["bkt_survivors"] <= pr["bkt_slots"], pr
        if all_bkt:
            assert pr["bkt_launches"] == pr["split_launches"], pr
        # one partition whose long runs all take the bucket form gets no nibble-plane copy
        assert (pr["nib_copy_bytes"] > 0) == nib_copy, pr


def best_code(table):
    """The code with the smallest sum a float table [M * 16] allows (the quantizer is monotone: also of its int8 table)."""
    b = table.reshape(M, 16).argmin(axis=1).astype(np.uint8)
    return b[0::2] | (b[1::2] << 4)


def with_key(rng, n, key):
    c = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    c[:, 0], c[:, 1] = key & 255, key >> 8
    return c


def planted_list(rng, best):
    """-> codes [3 * 16384 + 37, 8] as the module's docstring describes them."""
    bkey = int(best[0]) | int(best[1]) << 8
    free = [k for k in rng.permutation(65536).tolist() if k != bkey]
    k15, k16, k17, kone = free[:4]
    big = free[4:40]
    dup = np.tile(best, (16, 1))                                 # the bucket of 16: best with one late nibble changed, 16 ways
    dup[:, 0], dup[:, 1] = k16 & 255, k16 >> 8
    for i in range(16):
        dup[i, 2 + i % 6] ^= 1 << (i % 8)
    small = [best[None, :], with_key(rng, 15, k15), dup, with_key(rng, 17, k17)]
    nbig = TILE - sum(len(s) for s in small)
    bigs = rng.integers(0, 256, (nbig, M // 2), dtype=np.uint8)
    kk = np.array(big)[rng.integers(0, len(big), nbig)]
    bigs[:, 0], bigs[:, 1] = kk & 255, kk >> 8
    b0 = np.concatenate(small + [bigs])
    b0 = b0[rng.permutation(len(b0))]
    b1 = with_key(rng, TILE, kone)
    b2 = rng.integers(0, 256, (TILE, M // 2), dtype=np.uint8)
    k2 = rng.permutation(65536)[:TILE]
    b2[:, 0], b2[:, 1] = k2 & 255, k2 >> 8
    tail = rng.integers(0, 256, (37, M // 2), dtype=np.uint8)
    tail[:, 1] = 7
    tail[-1] = best
    codes = np.ascontiguousarray(np.concatenate([b0, b1, b2, tail]))
    sizes = np.unique(bkt_model.keys_of(codes[:TILE]), return_counts=True)[1].tolist()
    assert {1, 15, 16, 17} <= set(sizes) and len(np.unique(bkt_model.keys_of(b2))) == TILE
    return codes


@pytest.fixture(scope="module")
def planted(pyqadc, po):
    """The planted list, its tables, and per keep the row-major form's result and the oracle's: computed once, never changed."""
    rng = np.random.default_rng(2511)
    tables = float_tables(rng, 3, 1, M)
    codes = planted_list(rng, best_code(tables[0, 0]))
    want = {}
    for keep in KEEPS:
        idx = make_index(pyqadc, [codes], "rows", keep=keep)
        res = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
        check_profile(idx.profile(), "rows")
        idx.close()
        oracle = [po.query_scan(M, [codes], None, keep, [0], tables[q, 0].copy(), R) for q in range(3)]
        want[keep] = (res, oracle)
    return codes, tables, want


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_matches_rows_and_the_oracle_on_the_planted_list(pyqadc, planted, nsp, keep):
    codes, tables, want = planted
    n = len(codes)
    idx = make_index(pyqadc, [codes], nsp, keep=keep)
    got = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
    pr = idx.profile()
    idx.close()
    check_profile(pr, nsp)
    rows, oracle = want[keep]
    # blocks of 2, 1, 16 and 1 tiles (the planted shapes), levels [0, 16 Ki), [16 Ki, 64 Ki): two launches per query batch
    assert pr["bkt_codes"] == 3 * n and pr["bkt_slots"] > pr["bkt_codes"] and 0 < pr["bkt_survivors"], pr
    assert np.array_equal(got["status"], rows["status"]) and np.all(got["status"] == 0), got["status"]
    for q in range(3):
        assert got["heaps"][q][0].shape == rows["heaps"][q][0].shape and heaps_equal(got["heaps"][q], rows["heaps"][q]), q
        assert oracle[q]["rc"] == 0
        assert np.array_equal(got["heaps"][q][0], oracle[q]["keys"]) and np.array_equal(got["heaps"][q][1], oracle[q]["values"]), q
    # query 0's best code: once at its bucket of one (position: wherever the shuffle put it), and as the partition's last code with
    # the padding-lane replays; its 15 padding copies in the bucket are not emitted
    keys = got["heaps"][0][0]
    first = int(np.nonzero((codes[:TILE] == codes[-1]).all(axis=1))[0][0])
    assert np.count_nonzero(keys == first) == 1
    assert np.count_nonzero(keys == n - 1) == 1 + (16 - n % 16) % 16


def test_bkt_copy_equals_the_model(pyqadc, planted):
    codes = planted[0]
    idx = make_index(pyqadc, [codes], 6)
    copy = idx.bkt_copy(0)
    pr = idx.profile()
    idx.close()
    tiles = [l[2] // TILE for l in bkt_model.block_layout(codes, TILE)]
    assert tiles == [2, 1, 16, 1]
    assert copy is not None and pr["bkt_copy_slots"] == len(copy["perm"]) == sum(tiles) * TILE
    assert pr["bkt_copy_bytes"] == sum(tiles) * (100352 + 196608)
    bkt_model.check_copy(copy, codes, TILE)


def test_bkt_copy_two_tile_blocks_and_the_pad_limit(pyqadc):
    rng = np.random.default_rng(5)
    n = 5 * TILE + 4001
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] = 0
    codes[:, 0] &= 63                                            # 64 keys: buckets of some 500 codes
    idx = make_index(pyqadc, [codes], 5, block=2 * TILE)
    copy = idx.bkt_copy(0)
    idx.close()
    bkt_model.check_copy(copy, codes, 2 * TILE)
    # the default pad limit: a block of two tiles takes three with its padding, more than 1.125: no copy, counted, the runs keep the other forms
    idx = pyqadc.Index(M)
    idx.set_split(1, 1)
    idx.set_split_bkt(1, 2 * TILE)
    idx.add_partitions([codes])
    idx.finalize(0.01)
    pr = idx.profile()
    assert idx.bkt_copy(0) is None and pr["bkt_copy_padded_out"] == 1 and pr["bkt_copy_bytes"] == 0, pr
    idx.close()


@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_no_survivor_when_the_slack_reaches_the_bound(pyqadc, po, nsp):
    """Constant rows: all scores are 0, the highest rows are deferred; with 127 there c clamps to 127, bound <= c, bsurv = 0."""
    rng = np.random.default_rng(300 + nsp)
    n = 4 * TILE + 37
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] &= 1
    qt = np.zeros((2, 1, M, 16), np.int8)
    qt[:, :, 0:8, :] = 3
    qt[:, :, 8:16, :] = 127
    assert bs.choose_bkt(qt[0, 0], nsp) == (sum(1 << s for s in range(4 + nsp, M)), 127)
    assign = np.zeros((2, 1), np.int32)
    res = {}
    for form in (nsp, "rows"):
        idx = make_index(pyqadc, [codes], form)
        res[form] = idx.scan_i8(assign, qt, 300)
        pr = idx.profile()
        check_profile(pr, form)
        assert pr["bkt_survivors"] == 0, pr
        idx.close()
    for q in range(2):
        assert heaps_equal(res[nsp][q], res["rows"][q]), q
    if po.have_ref():
        want = po.ref_scan_interleaved(M, [po.ref_interleave(codes)], [n], None, qt[0], 300)
        assert heaps_equal(res[nsp][0], want)


def test_bkt_labels_and_two_partitions(pyqadc, po):
    rng = np.random.default_rng(17)
    sizes = [2 * TILE, 2 * TILE + 37]                            # every cut of both probe orders falls on a block of its partition
    parts = [rng.integers(0, 256, (s, M // 2), dtype=np.uint8) for s in sizes]
    for p in parts:
        p[:, 1] &= 3
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    tables = float_tables(rng, 2, 2, M)
    parts[1][-1] = best_code(tables[0, 1])                       # the labelled partition's last code is a candidate
    assign = np.array([[0, 1], [0, 1]], np.int32)
    out = {}
    for form in (6, "rows"):
        idx = make_index(pyqadc, parts, form, labels)
        out[form] = idx.query_scan(assign, tables.copy(), R)
        check_profile(idx.profile(), form, nib_copy=form != "rows")      # (two partitions: the cuts depend on the probe order)
        idx.close()
    assert np.all(out[6]["status"] == 0)
    for q in range(2):
        assert heaps_equal(out[6]["heaps"][q], out["rows"]["heaps"][q]), q
        want = po.query_scan(M, parts, labels, 0.01, [0, 1], tables[q].copy(), R)
        assert want["rc"] == 0 and np.array_equal(out[6]["heaps"][q][0], want["keys"]) and np.array_equal(out[6]["heaps"][q][1], want["values"])
    assert np.count_nonzero(out[6]["heaps"][0][0] == labels[1][-1]) >= 1 + (16 - sizes[1] % 16) % 16


def test_bkt_and_nibble_launches_in_one_batch(pyqadc, po):
    """Blocks of two tiles: the levels [0, 16 Ki) and [16 Ki, 64 Ki) miss a block boundary by one tile and take the nibble form;
    [64 Ki, n) starts on a block and ends the partition: the bucket form."""
    rng = np.random.default_rng(23)
    n = 65536 + 3 * 2 * TILE + 37
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] &= 1
    tables = float_tables(rng, 2, 1, M)
    out = {}
    for form in (5, "rows"):
        idx = make_index(pyqadc, [codes], form, block=2 * TILE)
        out[form] = (idx.query_scan(np.zeros((2, 1), np.int32), tables.copy(), R), idx.profile())
        idx.close()
    pr = out[5][1]
    check_profile(pr, 5, all_bkt=False, nib_copy=True)
    assert pr["bkt_launches"] == 1 and pr["nib_launches"] == 2 and pr["split_launches"] == 3, pr
    assert pr["bkt_codes"] == 2 * (n - 65536) and pr["nib_codes"] == 2 * 65536 and pr["nib_copy_bytes"] > 0, pr
    assert pr["bkt_survivors"] > 0 and pr["nib_survivors"] > 0, pr
    for q in range(2):
        assert heaps_equal(out[5][0]["heaps"][q], out["rows"][0]["heaps"][q]), q
        want = po.query_scan(M, [codes], None, 0.01, [0], tables[q, 0].copy(), R)
        assert want["rc"] == 0 and np.array_equal(out[5][0]["heaps"][q][0], want["keys"])


def test_bkt_choice_bytes_equal_the_twin(pyqadc):
    rng = np.random.default_rng(77)
    qt = np.concatenate([rng.integers(0, hi, (40, M, 16)) for hi in (2, 5, 30, 128)]).astype(np.int8)
    qt[0] = 0                                                    # all rows equal
    qt[1] = 127
    qt[2, 8:] = qt[2, :8]                                        # pairs of equal rows: ties
    got = pyqadc.bkt_choice(qt)
    want = [[[m & 0xff, m >> 8, c, 0] for m, c in (bs.choose_bkt(qt[t], nsp) for nsp in NSPS)] for t in range(len(qt))]
    assert got.tolist() == want
    assert got[0].tolist() == [[0x00, 0xff, 0, 0], [0x00, 0xfe, 0, 0], [0x00, 0xfc, 0, 0], [0x00, 0xf8, 0, 0]]


# ---- the kernel's edges: the nibble form's set (tests/test_gpu_nib_scan.py) under the bucket rule ------------------------------
# Every list below has a few tiles (TINY: levels [0, 16 Ki), [16 Ki, 64 Ki), [64 Ki, 256 Ki), ...; block = one tile unless said:
# every cut falls on a block).  A row-major result and an oracle result are computed once per case (once) and shared by the NSP.

_once = {}


def once(key, make):
    if key not in _once:
        _once[key] = make()
    return _once[key]


def scan(pyqadc, parts, form, tables, R, int8=False, labels=None, assign=None, keep=0.01, block=TILE, **opts):
    """-> (result, profile) of one batch on a fresh index of the form: scan_i8's heaps [(keys, values)] or query_scan's dict."""
    assign = np.zeros((len(tables), 1), np.int32) if assign is None else assign
    idx = make_index(pyqadc, parts, form, labels, keep=keep, block=block, **opts)
    try:
        res = idx.scan_i8(assign, tables, R) if int8 else idx.query_scan(assign, tables.copy(), R, want_qtables=True)
        return res, idx.profile()
    finally:
        idx.close()


def heaps_of(res, q):
    return res[q] if isinstance(res, list) else res["heaps"][q]


def assert_rows(got, rows, nq):
    """Heaps (keys, values, sizes) of every query and, for float tables, the status: the bucket form against the row-major form."""
    for q in range(nq):
        a, b = heaps_of(got, q), heaps_of(rows, q)
        assert a[0].shape == b[0].shape and heaps_equal(a, b), q
    if not isinstance(got, list):
        assert np.array_equal(got["status"], rows["status"]) and np.array_equal(got["sizes"], rows["sizes"])


def reference_i8(po, key, parts, labels, qt, queries, R):
    """{q: the reference's heap} of int8 tables qt [nq, 1, 16, 16] on the partitions in order, or None without the reference build."""
    if not po.have_ref():
        return None
    inter = [po.ref_interleave(p) for p in parts]
    return once(("reference", key), lambda: {q: po.ref_scan_interleaved(M, inter, [len(p) for p in parts], labels, qt[q], R) for q in queries})


def assert_reference_i8(got, want):
    for q, w in (want or {}).items():
        assert heaps_equal(heaps_of(got, q), w), q


def oracle_float(po, key, parts, labels, keep, tables, queries, R, assign=None):
    """{q: po.query_scan's result} for float tables [nq, ma, 256]."""
    return once(("oracle", key), lambda: {q: po.query_scan(M, parts, labels, keep, [0] if assign is None else assign[q], tables[q].copy(), R) for q in queries})


def assert_oracle_float(got, want):
    for q, w in want.items():
        assert w["rc"] == got["status"][q], q
        if w["rc"] == 0:
            assert np.array_equal(got["heaps"][q][0], w["keys"]) and np.array_equal(got["heaps"][q][1], w["values"]), q


def mask_of(subs):
    return sum(1 << s for s in subs)


def subs_of(mask):
    return [s for s in range(M) if mask >> s & 1]


def few_key_codes(rng, n, key_bits):
    """Random codes with 2^key_bits distinct keys (byte 1 = 0): buckets of n / 2^key_bits codes per block."""
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] = 0
    codes[:, 0] &= (1 << key_bits) - 1
    return codes


def random_key_codes(rng, n, nkeys):
    """Random codes whose keys are nkeys random ones of the 65536: every entry of the free rows is met by some bucket."""
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    kk = rng.permutation(65536)[:nkeys][rng.integers(0, nkeys, n)]
    codes[:, 0], codes[:, 1] = kk & 255, kk >> 8
    return codes


# ---- 1. both loop forms, and one workgroup that walks every tile ---------------------------------------------------------------

@pytest.mark.parametrize("opts", [dict(variant=0x0d), dict(variant=0x01), dict(wgs_per_item=1), dict(variant=0x01, wgs_per_item=1)],
                         ids=["chunked", "grid-stride", "one-workgroup", "grid-stride-one-workgroup"])
@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_loop_forms_on_the_planted_list(pyqadc, planted, nsp, opts):
    """variant 0x0d: chunked tiles (the default), 0x01: grid-stride; wgs_per_item = 1: one workgroup walks the run's 2 and 18
    tiles, so pend -> resolve -> emit crosses every tile iteration and ends on the last tile (the ragged block's: the
    partition's last code with its replays is emitted by the epilogue)."""
    codes, tables, want = planted
    n, keep = len(codes), KEEPS[0]
    got, pr = scan(pyqadc, [codes], nsp, tables, R, keep=keep, **opts)
    check_profile(pr, nsp)
    rows, oracle = want[keep]
    assert pr["bkt_codes"] == 3 * n and 0 < pr["bkt_survivors"] < pr["bkt_slots"], pr
    assert np.all(got["status"] == 0)
    assert_rows(got, rows, 3)
    assert_oracle_float(got, dict(enumerate(oracle)))
    keys = got["heaps"][0][0]
    first = int(np.nonzero((codes[:TILE] == codes[-1]).all(axis=1))[0][0])
    assert np.count_nonzero(keys == first) == 1 and np.count_nonzero(keys == n - 1) == 1 + (16 - n % 16) % 16


# ---- 2. every paid sub-quantizer in every role, in one launch ------------------------------------------------------------------

def bkt_window(k, nsp):
    """12 - nsp consecutive sub-quantizers of 4..15 from 4 + k on, cyclically."""
    return [4 + (k + i) % 12 for i in range(12 - nsp)]


def window_tables_bkt(rng, nsp):
    """16 int8 tables, test_gpu_nib_scan.window_tables restricted to sub-quantizers 4..15: the rule defers bkt_window(k, nsp) for
    table k < 12.  Even k: those rows hold 12..14 (a large c below the clamp), the others 0..13; odd k: 0..2 (c near 0), the
    others 8..39.  Tables 12..15 defer every second sub-quantizer from 4 + (k - 12) on (and the window's rest): in an ascending
    list of paid rows the parity of a row's place changes, so every row is the low and the high member of a pair somewhere."""
    qt = np.empty((16, 1, M, 16), np.int8)
    want = []
    for k in range(16):
        flat = k % 2 == 0
        qt[k, 0] = rng.integers(0, 14, (M, 16)) if flat else rng.integers(8, 40, (M, 16))
        if k < 12:
            deferred = bkt_window(k, nsp)
        else:
            comb = [4 + (k - 12 + 2 * i) % 12 for i in range(6)]                # six rows, every second one
            deferred = (comb + [s for s in range(15, 3, -1) if s not in comb])[:12 - nsp]
        for s in deferred:
            qt[k, 0, s] = rng.integers(12, 15, 16) if flat else rng.integers(0, 3, 16)
        want.append(mask_of(deferred))
    return qt, want


def roles(masks, nsp):
    """-> (deferred, low of a pair, high of a pair, single plane): the sets of sub-quantizers that take each role under the masks."""
    deferred, low, high, single = set(), set(), set(), set()
    for m in masks:
        paid = bs.bkt_paid(m)
        assert len(paid) == nsp
        deferred |= set(subs_of(m))
        low |= set(paid[0:2 * (nsp // 2):2])
        high |= set(paid[1:2 * (nsp // 2):2])
        single |= set(paid[2 * (nsp // 2):])
    return deferred, low, high, single


@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_every_paid_sub_quantizer_in_every_role_in_one_launch(pyqadc, po, nsp):
    rng = np.random.default_rng(2000 + nsp)
    n = 4 * TILE + 37
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] &= 1
    qt, want_masks = window_tables_bkt(rng, nsp)
    chosen = [bs.choose_bkt(qt[k, 0], nsp) for k in range(16)]
    assert [m for m, _ in chosen] == want_masks
    assert all(12 * (12 - nsp) <= c < 127 if k % 2 == 0 else c <= 16 for k, (_, c) in enumerate(chosen)), chosen
    deferred, low, high, single = roles(want_masks, nsp)
    every = set(range(4, M))
    # every role the ascending paid list allows: 4 is first (never a high member); the last one is the high member of the last
    # pair (even NSP: 15 is never low) or the single plane (odd NSP: 15 is nothing else, so 14 is never low; nor can a row
    # below 3 + NSP be last)
    assert deferred == every and high == every - ({4, 15} if nsp % 2 else {4}), (deferred, high)
    assert low == every - ({14, 15} if nsp % 2 else {15}), low
    assert single == (set(range(3 + nsp, M)) if nsp % 2 else set()), single
    got_choice = pyqadc.bkt_choice(qt)
    assert got_choice[:, nsp - 4].tolist() == [[m & 0xff, m >> 8, c, 0] for m, c in chosen]
    Rr = 150
    rows = once(("roles", nsp, "rows"), lambda: scan(pyqadc, [codes], "rows", qt, Rr, int8=True))[0]
    got, pr = scan(pyqadc, [codes], nsp, qt, Rr, int8=True)
    check_profile(pr, nsp)
    assert 0 < pr["bkt_survivors"] < pr["bkt_slots"], pr
    assert_rows(got, rows, 16)
    assert_reference_i8(got, reference_i8(po, ("roles", nsp), [codes], None, qt, (0, 5, 10, 13, 15), Rr))


# ---- 3. float tables: the quantizer's workgroup picks a different mask per query -----------------------------------------------

@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_float_tables_choose_different_masks_inside_one_launch(pyqadc, po, nsp):
    rng = np.random.default_rng(32)
    n = 4 * TILE + 37
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] &= 1
    nq = 12
    tables = float_tables(rng, nq, 1, M)
    for q in range(nq):
        for s in bkt_window(q, nsp):
            tables[q, 0].reshape(M, 16)[s] *= np.float32(0.02)
    want = oracle_float(po, ("masks", nsp), [codes], None, 0.01, tables, range(nq), R)

    def masks(qtables):
        chosen = [bs.choose_bkt(np.asarray(qtables[q]).reshape(-1, M, 16)[0], nsp)[0] for q in range(nq)]
        assert len(set(chosen)) >= 8 and {s for m in chosen for s in subs_of(m)} == set(range(4, M)), chosen
        return chosen

    masks([want[q]["qtables"] for q in range(nq)])                             # the oracle's int8 tables: before anything runs
    rows = once(("masks", nsp, "rows"), lambda: scan(pyqadc, [codes], "rows", tables, R))[0]
    got, pr = scan(pyqadc, [codes], nsp, tables, R)
    check_profile(pr, nsp)
    masks(got["qtables"])
    assert np.all(got["status"] == 0) and 0 < pr["bkt_survivors"] < pr["bkt_slots"], pr
    assert_rows(got, rows, nq)
    assert_oracle_float(got, want)


# ---- 4. slack edges ------------------------------------------------------------------------------------------------------------

def edge_tables(rng, case):
    """test_gpu_nib_scan.edge_tables under the bucket rule: rows 0-3 are always exact, only rows 4..15 can be deferred; in every
    case the rule defers rows 4 + NSP .. 15 (constant rows score 0, ties: the highest)."""
    qt = np.zeros((2, 1, M, 16), np.int8)
    if case == "clamp":                 # 127 in the deferred rows: c clamps to 127, bsurv = 0
        qt[:, :, 0:8, :] = 3
        qt[:, :, 8:16, :] = 127
    elif case == "c0":                  # rows 8..15: 0 with one 1 (minimum 0: c = 0, score 1); rows 0..7 spread wide
        qt[:, :, 0:8, :] = rng.integers(0, 60, (2, 1, 8, 16), dtype=np.int8)
        qt[:, :, 8:16, 3] = 1
    elif case == "reach":               # rows 0..10: 0 but for one entry; rows 8..15: 2 (8..10 with that entry: score 50, deferred last;
        qt[:, :, 0:11, 5] = 50          # 15: some threes): every sum is >= 16, c = 2 (12 - NSP), the smallest partial 2 (NSP - 4)
        qt[:, :, 8:16, :] = 2
        qt[:, :, 8:11, 5] = 52
        qt[:, :, 15, 0:4] = 3
    else:                               # "sat": rows 0..7 127, rows 8..15 4: min(127, partial) is never below a bound
        qt[:, :, 0:8, :] = 127
        qt[:, :, 8:16, :] = 4
    return qt


EDGE_C = {"clamp": lambda nsp: 127, "c0": lambda nsp: 0, "reach": lambda nsp: 2 * (12 - nsp), "sat": lambda nsp: 4 * (12 - nsp)}
EDGE_R = {"c0": 300, "c0-every-candidate": 4000, "reach": 50, "sat": 300}


@pytest.mark.parametrize("case", ["c0", "c0-every-candidate", "reach", "sat"])
@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_slack_edges(pyqadc, po, nsp, case):
    """c0: c = 0, bsurv = bound.  c0-every-candidate: the same tables with an R above the number of codes whose sum is below 127:
    the bound stays 127 and the heap holds every one of them, those of value 126 whose deferred entries are all 0 too, which a
    c one too large (or a bsurv one too small) loses.  reach: level 0's bound is 127 (most of its codes are candidates); more than a third of the
    codes have the smallest sum there is, 16, so from level 1 on the bound is 16, bsurv = 16 - c = 2 (NSP - 4) = the smallest
    partial there is: no survivor.  A c one too small keeps that third of the codes survivors to the end; a c one too large loses
    candidates wherever a candidate's deferred rows are all at their minimum (c0: most codes).  sat: no partial below any bound."""
    tabs = case.split("-")[0]
    rng = np.random.default_rng({"c0": 301, "reach": 302, "sat": 303}[tabs])
    n = 4 * TILE + 37
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] &= 1
    qt = edge_tables(rng, tabs)
    for q in range(2):
        assert bs.choose_bkt(qt[q, 0], nsp) == (mask_of(range(4 + nsp, M)), EDGE_C[tabs](nsp)), (q, nsp)
    Rr = EDGE_R[case]
    rows = once(("edge", case, "rows"), lambda: scan(pyqadc, [codes], "rows", qt, Rr, int8=True))[0]
    got, pr = scan(pyqadc, [codes], nsp, qt, Rr, int8=True)
    check_profile(pr, nsp)
    if case == "sat":
        assert pr["bkt_survivors"] == 0 and pr["regrows"] == 0, pr
    elif case == "reach":
        assert 0 < pr["bkt_survivors"] <= 2 * bkt_model.block_layout(codes, TILE)[0][2], pr     # two queries: level 0's slots at the most
    else:
        assert 0 < pr["bkt_survivors"] <= pr["bkt_slots"] and pr["regrows"] == 0, pr
    if case == "c0-every-candidate":
        for q in range(2):                                                       # the row-major form's heap: not full, and it holds the value 126
            assert len(heaps_of(rows, q)[1]) < Rr and np.count_nonzero(heaps_of(rows, q)[1] == 126) >= 10, q
    assert_rows(got, rows, 2)
    assert_reference_i8(got, reference_i8(po, ("edge", case), [codes], None, qt, range(2), Rr))


# ---- 5. saturation -------------------------------------------------------------------------------------------------------------

SAT_CHEAP = (15, 14, 11, 10, 9, 7, 6, 4)       # the rows the rule may defer: 12 - NSP of them


def saturation_tables(rng, where):
    """3 float tables [3, 1, 256]: rows SAT_CHEAP scaled by 0.02 (the rule's choice), entries of 1e4 (far above any qmax: 127 in
    the int8 table): one in each free row, two in each of the other four rows (paid for every NSP), one in each cheap row, or
    all three (a quarter of the codes then meet none of them: more than R of the starts, so qmax stays an ordinary sum)."""
    tables = float_tables(rng, 3, 1, M)
    t = tables.reshape(3, M, 16)
    t[:, SAT_CHEAP, :] *= np.float32(0.02)
    t[:, [s for s in range(4, M) if s not in SAT_CHEAP], :] *= np.float32(2)    # (wide rows: a cheap row stays the choice with one 127 in it)
    for q in range(3):
        for s in range(M):
            role = "free" if s < 4 else "deferred" if s in SAT_CHEAP else "paid"
            if where in (role, "all"):
                t[q, s, rng.permutation(16)[:2 if role == "paid" else 1]] = 1e4
    return tables


def saturated_rows(qt):
    return {s for s in range(M) if (np.asarray(qt).reshape(M, 16)[s] == 127).any()}


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("where", ["free", "paid", "deferred", "all"])
@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_saturation(pyqadc, po, nsp, where, keep):
    """Entries of 127 in the free rows (the exact free-pair partial P01 + P23 rises to 508), the paid rows (partials above 127 in
    the survivor's byte-packed partial), the deferred rows (full sums above 127: min(127, .) against the bound) and all three."""
    rng = np.random.default_rng({"free": 50, "paid": 51, "deferred": 52, "all": 53}[where])
    n = 12 * TILE + 37                                                           # 1966 starts at keep 0.01
    codes = random_key_codes(rng, n, 256)
    tables = saturation_tables(rng, where)
    Rr = 400
    want = oracle_float(po, ("sat", where, keep), [codes], None, keep, tables, range(3), Rr)
    for q in range(3):                                                           # on the oracle's int8 tables, before anything runs
        qt = want[q]["qtables"][0]
        mask, c = bs.choose_bkt(qt, nsp)
        assert len(subs_of(mask)) == 12 - nsp and set(subs_of(mask)) <= set(SAT_CHEAP), (q, hex(mask))
        sat = saturated_rows(qt)
        assert (where in ("free", "all")) == ({0, 1, 2, 3} <= sat) and (where in ("free", "all") or not sat & {0, 1, 2, 3}), sat
        assert (where in ("paid", "all")) == (set(range(4, M)) - set(SAT_CHEAP) <= sat), sat
        assert (where in ("deferred", "all")) == (set(SAT_CHEAP) <= sat) and (where in ("deferred", "all") or not sat & set(SAT_CHEAP)), sat
    rows = once(("sat", where, keep, "rows"), lambda: scan(pyqadc, [codes], "rows", tables, Rr, keep=keep))[0]
    got, pr = scan(pyqadc, [codes], nsp, tables, Rr, keep=keep)
    check_profile(pr, nsp)
    assert np.all(got["status"] == 0) and 0 < pr["bkt_survivors"] < pr["bkt_slots"], pr
    for q in range(3):
        assert np.array_equal(got["qtables"][q, 0], want[q]["qtables"][0]), q
    assert_rows(got, rows, 3)
    assert_oracle_float(got, want)
    assert_reference_i8(got, reference_i8(po, ("sat", where, keep), [codes], None, got["qtables"], range(3), Rr))


# ---- 6. tie-heavy tables -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_tie_heavy_tables(pyqadc, po, nsp, keep):
    """Two distinct entry values only, and a table whose rows are all equal: thousands of codes share every sum, and which of
    them the heap keeps is decided by scan order, which only the position sort before the replay restores.  Four keys per
    block: buckets of 4096 codes, the equal sums lie scattered over the buckets of five blocks.  Int8 tables, and the same
    two-valued tables as floats (the quantizer keeps two values two values) at both keep values."""
    rng = np.random.default_rng(41)
    n = 4 * TILE + 37
    codes = few_key_codes(rng, n, 2)
    qt = (rng.integers(0, 2, (3, 1, M, 16)) * 9).astype(np.int8)
    qt[2, 0, :] = qt[2, 0, 0]
    Rr = 500
    rows = once(("ties", "rows"), lambda: scan(pyqadc, [codes], "rows", qt, Rr, int8=True))[0]
    got, pr = scan(pyqadc, [codes], nsp, qt, Rr, int8=True, keep=keep)
    check_profile(pr, nsp)
    for q in range(3):                                                           # a full heap in which one value is shared by a hundred codes
        vals = heaps_of(rows, q)[1]
        assert len(vals) == Rr and np.unique(vals, return_counts=True)[1].max() >= 100, q
    assert_rows(got, rows, 3)
    assert_reference_i8(got, reference_i8(po, "ties", [codes], None, qt, range(3), Rr))
    tables = np.ascontiguousarray(qt.astype(np.float32).reshape(3, 1, M * 16))
    want = oracle_float(po, ("ties", keep), [codes], None, keep, tables, range(3), Rr)
    frows = once(("ties", keep, "rows"), lambda: scan(pyqadc, [codes], "rows", tables, Rr, keep=keep))[0]
    fgot, fpr = scan(pyqadc, [codes], nsp, tables, Rr, keep=keep)
    check_profile(fpr, nsp)
    assert_rows(fgot, frows, 3)
    assert_oracle_float(fgot, want)


# ---- 7. R around the number of starts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_R_around_the_starts(pyqadc, po, planted, nsp, keep):
    codes, tables, _ = planted
    starts = max(1, int(len(codes) * keep))
    assert starts in (491, 2459)
    for Rr in (1, starts - 1, starts, starts + 1):
        rows = once(("R", keep, Rr, "rows"), lambda: scan(pyqadc, [codes], "rows", tables, Rr, keep=keep))[0]
        want = oracle_float(po, ("R", keep, Rr), [codes], None, keep, tables, range(3), Rr)
        got, pr = scan(pyqadc, [codes], nsp, tables, Rr, keep=keep)
        assert np.array_equal(got["status"], rows["status"]) and np.all((got["status"] == 0) == (Rr <= starts)), (Rr, got["status"])
        for q in range(3):
            assert (want[q]["rc"] == 0) == (got["status"][q] == 0), (Rr, q)
            if got["status"][q] == 0:
                assert heaps_equal(got["heaps"][q], rows["heaps"][q]), (Rr, q)
                assert np.array_equal(got["heaps"][q][0], want[q]["keys"]) and np.array_equal(got["heaps"][q][1], want[q]["values"]), (Rr, q)
        if Rr <= starts:
            check_profile(pr, nsp)


# ---- 8. region overflow and the re-run of the batch ----------------------------------------------------------------------------

@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_region_overflow_and_rerun(pyqadc, po, nsp):
    """cand_capacity = 256 with R = 4000: level 0 alone emits thousands of candidates per query, the region overflows and the
    batch is re-run with a larger one; the partition's last code (n % 16 = 5) is query 0's best one, so its padding-lane replays
    (dup_pos) pass through the re-run."""
    rng = np.random.default_rng(6)
    n, keep, Rr = 6 * TILE + 5, 0.05, 4000
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] &= 1
    tables = float_tables(rng, 2, 1, M)
    codes[-1] = best_code(tables[0, 0])
    assert int(n * keep) >= Rr and n % 16 != 0
    rows, rpr = once(("overflow", "rows"), lambda: scan(pyqadc, [codes], "rows", tables, Rr, keep=keep, cand_capacity=256))
    want = oracle_float(po, "overflow", [codes], None, keep, tables, range(2), Rr)
    got, pr = scan(pyqadc, [codes], nsp, tables, Rr, keep=keep, cand_capacity=256)
    check_profile(pr, nsp)
    assert pr["regrows"] >= 1 and rpr["regrows"] >= 1, (pr, rpr)
    assert np.all(got["status"] == 0)
    assert_rows(got, rows, 2)
    assert_oracle_float(got, want)
    assert np.count_nonzero(got["heaps"][0][0] == n - 1) == 1 + (16 - n % 16) % 16


# ---- 9. keys and bucket shapes that are scanned, not only copied ---------------------------------------------------------------

def shaped_list(rng, tables):
    """Blocks of two tiles.  Block 0: a bucket for key 0x0000 (100 codes, one of them query 0's best code), behind it the
    bucket of key 0x0001 with 20 000 codes: slots 112 .. 20 111, across the tile boundary inside the block (one of them query
    2's best code), a bucket for key 0xffff (200 codes, with query 1's best code: the block's last bucket) and 16 others; the
    block is full, so its few padding slots add a third tile, which holds nothing but copies.  Block 1: 1080 buckets of one
    code (15 padding slots each) and eight large ones: a third tile again, half real.  Block 2: 37 codes."""
    best = [best_code(tables[q, 0]) for q in range(3)]
    assert [int(b[0]) | int(b[1]) << 8 for b in best] == [0x0000, 0xffff, 0x0001]
    k0, kstraddle, kff = with_key(rng, 100, 0x0000), with_key(rng, 20000, 0x0001), with_key(rng, 200, 0xffff)
    k0[17], kff[150], kstraddle[16300] = best
    rest = rng.integers(0, 256, (2 * TILE - 20300, M // 2), dtype=np.uint8)
    rest[:, 1] = 0x40
    rest[:, 0] &= 15
    b0 = np.concatenate([k0, kstraddle, kff, rest])
    b0 = b0[rng.permutation(len(b0))]
    ones = rng.integers(0, 256, (1080, M // 2), dtype=np.uint8)
    k1 = 0x1000 + rng.permutation(0x8000)[:1080]
    ones[:, 0], ones[:, 1] = k1 & 255, k1 >> 8
    large = rng.integers(0, 256, (2 * TILE - 1080, M // 2), dtype=np.uint8)
    large[:, 1] = 0xee
    large[:, 0] &= 7
    b1 = np.concatenate([ones, large])
    b1 = b1[rng.permutation(len(b1))]
    tail = rng.integers(0, 256, (37, M // 2), dtype=np.uint8)
    tail[:, 1] = 7
    return np.ascontiguousarray(np.concatenate([b0, b1, tail])), best


def shaped_tables(rng):
    """Three float tables whose best codes have the keys 0x0000, 0xffff and 0x0001: the smallest entry of rows 0-3 is moved there."""
    tables = float_tables(rng, 3, 1, M)
    t = tables.reshape(3, M, 16)
    for q, nibbles in enumerate(((0, 0, 0, 0), (15, 15, 15, 15), (1, 0, 0, 0))):
        for s, e in enumerate(nibbles):
            t[q, s, e] = t[q, s].min() * np.float32(0.5)
    return tables


@pytest.mark.parametrize("nsp", NSPS)
def test_bkt_scans_the_edge_keys_and_a_bucket_across_tiles(pyqadc, po, nsp):
    rng = np.random.default_rng(909)
    tables = shaped_tables(rng)
    codes, best = shaped_list(rng, tables)
    n = len(codes)
    layout = bkt_model.block_layout(codes, 2 * TILE)
    assert [l[2] // TILE for l in layout] == [3, 3, 1]
    (key_a, start_a, cnt_a), (key_b, start_b, cnt_b) = layout[0][1][0], layout[0][1][1]
    assert (key_a, start_a, cnt_a) == (0x0000, 0, 100) and (key_b, start_b, cnt_b) == (0x0001, 112, 20000) and start_b < TILE < start_b + cnt_b
    assert layout[0][1][-1][0] == 0xffff and layout[0][1][-1][2] == 200
    want = oracle_float(po, "shapes", [codes], None, 0.01, tables, range(3), R)
    # levels [0, 32 Ki), [32 Ki, 128 Ki): block 0 is level 0's run, blocks 1 and 2 are level 1's
    rows = once(("shapes", "rows"), lambda: scan(pyqadc, [codes], "rows", tables, R, level_base=2 * TILE))[0]
    idx = make_index(pyqadc, [codes], nsp, block=2 * TILE, level_base=2 * TILE)
    try:
        copy = idx.bkt_copy(0)
        got = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
        pr = idx.profile()
    finally:
        idx.close()
    bkt_model.check_copy(copy, codes, 2 * TILE)
    assert pr["bkt_copy_slots"] == 7 * TILE and pr["bkt_launches"] == 2 and pr["bkt_codes"] == 3 * n and pr["bkt_slots"] == 3 * 7 * TILE, pr
    check_profile(pr, nsp)
    assert np.all(got["status"] == 0)
    assert_rows(got, rows, 3)
    assert_oracle_float(got, want)
    for q in range(3):                                                           # each best code is in its query's heap, once
        pos = int(np.nonzero((codes == best[q]).all(axis=1))[0][0])
        assert np.count_nonzero(got["heaps"][q][0] == pos) == 1, q


# ---- 10. the thresholds pick NSP per launch ------------------------------------------------------------------------------------

def bkt_planes(run, min_run6, min_run5, min_run4):
    """host/level_plan.hpp: bkt_planes (swept on a CPU by tests/test_level_plan_bkt_host.py)."""
    return 4 if min_run4 and run >= min_run4 else 5 if min_run5 and run >= min_run5 else 6 if min_run6 and run >= min_run6 else 7


def test_bkt_thresholds_pick_the_planes_per_launch(pyqadc, po):
    """One list of 256 Ki + 37 codes: levels of 16 Ki, 48 Ki, 192 Ki and 37 codes, one launch each for the batch's two queries.
    bkt6/5/4_min_run decide the paid planes of each launch; they may change on the finalized index (the copy serves every NSP)."""
    rng = np.random.default_rng(10)
    n = 16 * TILE + 37
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    codes[:, 1] &= 1
    tables = float_tables(rng, 2, 1, M)
    assign = np.zeros((2, 1), np.int32)
    runs = [TILE, 3 * TILE, 12 * TILE, 37]
    K = 1024
    configs = [(48 * K, 192 * K, 0), (16 * K, 48 * K, 192 * K), (0, 0, 1), (192 * K + 1, 0, 0), (0, 48 * K, 0)]
    planes = [[bkt_planes(r, *cfg) for r in runs] for cfg in configs]
    assert planes[:3] == [[7, 6, 5, 7], [6, 5, 4, 7], [4, 4, 4, 4]] and planes[3] == [7] * 4 and planes[4] == [7, 5, 5, 7]
    rows = scan(pyqadc, [codes], "rows", tables, R)[0]
    want = oracle_float(po, "thresholds", [codes], None, 0.01, tables, range(2), R)

    def check(idx, cfg, what):
        idx.profile_reset()
        got = idx.query_scan(assign, tables.copy(), R)
        pr = idx.profile()
        check_profile(pr, 7)
        count = [pr["bkt%d_launches" % p] for p in NSPS]
        assert count == [[bkt_planes(r, *cfg) for r in runs].count(p) for p in NSPS] and sum(count) == pr["bkt_launches"] == 4, (what, cfg, pr)
        assert pr["bkt_codes"] == 2 * n and pr["bkt_survivors"] > 0, (what, pr)
        assert np.all(got["status"] == 0), what
        assert_rows(got, rows, 2)
        assert_oracle_float(got, want)

    for cfg in configs[:2]:                                                      # the thresholds in force at finalize
        idx = pyqadc.Index(M)
        try:
            for k, v in dict(ONE_QUERY_PER_PASS, **TINY).items():
                idx.set_option(k, v)
            idx.set_split(1, 1)
            idx.set_split_bkt(1, TILE, cfg[0], cfg[1], cfg[2], 1e6)
            idx.add_partitions([codes])
            idx.finalize(0.01)
            idx.set_option("profile", 1)
            check(idx, cfg, "at finalize")
            for later in configs[::-1]:                                          # ... and changed afterwards, on the same copy
                idx.set_split_bkt(1, TILE, later[0], later[1], later[2], 1e6)
                check(idx, later, "changed on the finalized index")
        finally:
            idx.close()
