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
partition's last code is the best code again (a candidate with its padding-lane replays, dup_pos)."""
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
