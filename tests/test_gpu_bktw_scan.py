"""GPU: the wide form of the bucket scan ("wide octaves"): from position W on the bucket copy is stored in
octave blocks grouped by the 20-bit key (code bytes 0, 1 and the low nibble of byte 2), so sub-quantizers 0-4 come from a 3-byte
id per 16 slots and NSP = 3, 4, 5 or 6 of the other 11 are paid for.  Every comparison is heaps bit for bit (keys, values, sizes,
status): the wide form forced at lists of a few tiles (W = one or two tiles) against the same index's row-major form and against
the CPU oracle (po.query_scan; the reference build's scan for int8 tables); the copies are read back and checked against the numpy
model (tests/bktw_model.py).

Levels (TINY): [0, 16 Ki), [16 Ki, 64 Ki), [64 Ki, 256 Ki).  With W = one tile the octaves are [1, 2), [2, 4), [4, 8), [8, ..) tiles:
level 0 is a narrow bucket launch (block = one tile), levels 1 and 2 cover two octaves each and are wide launches.

The planted list (planted_wide): 12 tiles + 37 codes.  Its keys come from a pool of 20-bit prefixes that holds 0x00000, 0xfffff and
the prefix of query 0's best code; row 4 and row 5 (the high nibble of byte 2, NOT part of the key) vary inside every pool.  The
octaves of one and two tiles hold buckets that are multiples of 16 (no padding: one padded slot would cost a whole tile, twice
the codes); the octave of four tiles holds buckets of 1 (the best code: its 15 padding copies must not be emitted), 15, 16 and
17 codes among buckets of thousands that cross tile boundaries; the last octave (4 tiles + 37) has 8 keys and ends on the best
code again (a candidate with its padding-lane replays).  Every octave stays under the cap the tests set (1.3; checked on the CPU).

Mutants and the tests that catch them (each was reasoned from the kernel; the first four are the issue's):
  id4 from the wrong nibble (the high nibble of byte 2, or the fill kernel writing it)  -> copy_equals_the_model (the id4 plane),
      planted / roles (row 4's entries differ widely: every partial sum is wrong)
  c one too large                                       -> slack_edges[c0-every-candidate] (the heap keeps every candidate, those
      of value 126 whose deferred entries are all 0 included)
  a padding slot emitted                                -> planted (the best code exactly once at its bucket of one)
  the choice made among rows 4-15 instead of 5-15       -> choice_bytes_equal_the_twin (a flat row 4 would be deferred), roles
  row 4 fused on the wrong side of the pair / the single slot's high half read -> roles (odd and even NSP)
  a paid plane's offset taken from the narrow tile's 12 planes -> planted, roles
  an octave's perm relative to the octave instead of the partition -> planted (keys), shard
  narrow blocks kept under a wide octave, or a narrow run planned over one -> copy_equals_the_model, fallback
  bktw_off, bktw_block, the wide allocation or the covered ranges kept from an earlier finalize -> rebuilt_after_growth (a tail that
      turns wide, a new octave), rebuilt_after_remove"""
import os
import sys

import numpy as np
import pytest

import bktw_model as wm
import test_gpu_bkt_scan as narrow
from dist_cases import start_size
from helpers import float_tables, heaps_equal

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bucket_survivors as bs  # noqa: E402

pytestmark = pytest.mark.gpu
M = 16
TILE = 16384
NSPS = (3, 4, 5, 6)
R = 100
CAP = 1.3          # the planted list's cap; LOOSE for lists whose one-tile octave may take two tiles
LOOSE = 2.01
N12 = 12 * TILE + 37


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def make_index(pyqadc, parts, form, labels=None, keep=0.01, W=TILE, cap=LOOSE, block=TILE, thresholds=None, finalize=True, idx=None, **opts):
    """form: "rows", or NSP = 3..6: wide blocks from W on with that many paid planes from one code on; narrow blocks (6 paid planes)
    elsewhere; runs neither fits: 9 nibble planes.  thresholds: (min_run, min_run5, min_run4, min_run3) instead.  idx: an index
    that exists already (with its quantizers set) takes the settings instead of a new one."""
    idx = pyqadc.Index(M) if idx is None else idx
    for k, v in dict(narrow.ONE_QUERY_PER_PASS, **dict(narrow.TINY, **opts)).items():
        idx.set_option(k, v)
    rows = form == "rows"
    idx.set_split(0 if rows else 1, 1)
    idx.set_split6(0 if rows else 1)
    idx.set_split5(0 if rows else 1)
    idx.set_split_nib(0 if rows else 1, 0, 9)
    if rows:
        idx.set_split_bkt(0)
        idx.set_split_bkt_wide(0)
    else:
        idx.set_split_bkt(1, block, 1, 0, 0, 1e6)
        t = thresholds or (1, int(form <= 5), int(form <= 4), int(form == 3))
        idx.set_split_bkt_wide(W, t[0], t[1], t[2], t[3], cap)
    if parts is not None:
        idx.add_partitions(parts, labels)
    if finalize:
        idx.finalize(keep)
        idx.set_option("profile", 1)
    return idx


def check_profile(pr, form, wide_launches=True):
    """Every split launch is counted under exactly one form; a rows index has no copy and no form."""
    forms = ("bktw", "bkt", "nib", "nib8", "split5", "split6")
    assert sum(pr[f + "_launches"] for f in forms) == pr["split_launches"], pr
    assert sum(pr[f + "_codes"] for f in forms) == pr["split_codes"], pr
    assert pr["bktw3_launches"] + pr["bktw4_launches"] + pr["bktw5_launches"] + pr["bktw6_launches"] == pr["bktw_launches"], pr
    if form == "rows":
        assert pr["bktw_launches"] == pr["bktw_copy_bytes"] == pr["bkt_copy_bytes"] == pr["split_codes"] == 0, pr
    else:
        assert pr["bktw%d_launches" % form] == pr["bktw_launches"] and pr["bktw_codes"] <= pr["bktw_slots"], pr
        assert (pr["bktw_launches"] > 0) == wide_launches, pr
        assert pr["bktw_survivors"] <= pr["bktw_slots"] and pr["bkt_copy_failed"] == pr["bkt_copy_padded_out"] == 0, pr
        assert pr["bktw_copy_bytes"] == pr["bktw_copy_slots"] // TILE * (wm.TILE_BYTES + wm.SIDE_BYTES) > 0, pr


def set_key(codes, key):
    key = np.asarray(key, np.uint32)
    codes[:, 0], codes[:, 1] = key & 255, (key >> 8) & 255
    codes[:, 2] = (codes[:, 2] & 0xf0) | (key >> 16)


def pooled(rng, counts, keys):
    """Random codes, counts[i] of them with the 20-bit key keys[i], shuffled."""
    out = []
    for c, k in zip(counts, keys):
        part = rng.integers(0, 256, (c, M // 2), dtype=np.uint8)
        set_key(part, np.full(c, k))
        out.append(part)
    out = np.concatenate(out)
    return out[rng.permutation(len(out))]


def planted_wide(rng, best):
    bkey = int(wm.keys_of(best[None, :])[0])
    pool = [0x00000, 0xfffff] + [int(k) for k in rng.permutation(1 << 20)[:38] if k not in (0, 0xfffff, bkey)]
    head = rng.integers(0, 256, (TILE, M // 2), dtype=np.uint8)
    head[:, 1] &= 1                                               # the narrow block: 512 keys
    o0 = pooled(rng, [16 * 64] * 16, pool[:16])                   # one tile: 16 buckets of 1024
    o1 = pooled(rng, [16 * 100] * 20 + [2 * TILE - 16 * 100 * 20], pool[10:31])      # two tiles: multiples of 16
    k15, k16, k17 = pool[31:34]
    dup = np.tile(best, (16, 1))                                  # the bucket of 16: best with one late nibble changed, 16 ways
    set_key(dup, np.full(16, k16))
    for i in range(16):
        dup[i, 3 + i % 5] ^= 1 << (i % 8)
    small = [best[None, :].copy(), pooled(rng, [15], [k15]), dup, pooled(rng, [17], [k17])]
    nbig = 4 * TILE - sum(len(s) for s in small)
    big_keys = [k for k in pool[:24]]
    o2 = np.concatenate(small + [pooled(rng, np.bincount(rng.integers(0, 24, nbig), minlength=24).tolist(), big_keys)])
    o2 = o2[rng.permutation(len(o2))]
    n3 = 4 * TILE + 37
    o3 = pooled(rng, np.bincount(rng.integers(0, 8, n3), minlength=8).tolist(), pool[30:38])
    o3[-1] = best
    codes = np.ascontiguousarray(np.concatenate([head, o0, o1, o2, o3]))
    assert len(codes) == N12
    return codes


def assert_under_cap(codes, W, cap, fallback=()):
    """On the CPU: which octaves the model stores wide under the cap."""
    wide = wm.wide_layout(codes, W, cap)
    assert [i for i, l in enumerate(wide) if not l[4]] == list(fallback), [(l[0], l[1], l[4]) for l in wide]
    return wide


@pytest.fixture(scope="module")
def planted(pyqadc, po):
    """The planted list, its tables, the row-major form's result and the oracle's: computed once, never changed."""
    rng = np.random.default_rng(2612)
    tables = float_tables(rng, 3, 1, M)
    codes = planted_wide(rng, narrow.best_code(tables[0, 0]))
    wide = assert_under_cap(codes, TILE, CAP)
    sizes = {c for _, _, _, buckets, _ in wide for _, _, c in buckets}
    assert {1, 15, 16, 17} <= sizes and max(sizes) > 2000
    keys = {k for _, _, _, buckets, _ in wide for k, _, _ in buckets}
    assert {0x00000, 0xfffff} <= keys and 8 <= len(keys) <= 41
    idx = make_index(pyqadc, [codes], "rows")
    rows = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
    check_profile(idx.profile(), "rows")
    idx.close()
    oracle = [po.query_scan(M, [codes], None, 0.01, [0], tables[q, 0].copy(), R) for q in range(3)]
    return codes, tables, rows, oracle


@pytest.mark.parametrize("opts", [dict(variant=0x0d), dict(variant=0x01), dict(variant=0x01, wgs_per_item=1)],
                         ids=["chunked", "grid-stride", "grid-stride-one-workgroup"])
@pytest.mark.parametrize("nsp", NSPS)
def test_wide_matches_rows_and_the_oracle_on_the_planted_list(pyqadc, planted, nsp, opts):
    codes, tables, rows, oracle = planted
    n = len(codes)
    idx = make_index(pyqadc, [codes], nsp, cap=CAP, **opts)
    got = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
    pr = idx.profile()
    idx.close()
    check_profile(pr, nsp)
    # per query: level 0 narrow (one tile), levels 1 and 2 wide (octaves 0-1 and 2-3): no nibble copy is ever needed
    assert pr["bkt_launches"] == 1 and pr["bktw_launches"] == 2 and pr["split_launches"] == 3 and pr["nib_copy_bytes"] == 0, pr
    assert pr["bkt_codes"] == 3 * TILE and pr["bktw_codes"] == 3 * (n - TILE) and pr["bktw_slots"] > pr["bktw_codes"], pr
    assert 0 < pr["bktw_survivors"] < pr["bktw_slots"] and pr["bktw_copy_fallback"] == 0, pr
    assert np.array_equal(got["status"], rows["status"]) and np.all(got["status"] == 0), got["status"]
    for q in range(3):
        assert got["heaps"][q][0].shape == rows["heaps"][q][0].shape and heaps_equal(got["heaps"][q], rows["heaps"][q]), q
        assert oracle[q]["rc"] == 0
        assert np.array_equal(got["heaps"][q][0], oracle[q]["keys"]) and np.array_equal(got["heaps"][q][1], oracle[q]["values"]), q
    keys = got["heaps"][0][0]
    first = int(np.nonzero((codes[:8 * TILE] == codes[-1]).all(axis=1))[0][0])
    assert 4 * TILE <= first < 8 * TILE and np.count_nonzero(keys == first) == 1      # the bucket of one: once, no padding copy
    assert np.count_nonzero(keys == n - 1) == 1 + (16 - n % 16) % 16


@pytest.mark.parametrize("W", [TILE, 2 * TILE])
def test_wide_copy_equals_the_model(pyqadc, planted, W):
    """W = two tiles: octaves [2, 4), [4, 8), [8, ..): levels 0 and 1 miss them (level 1 starts one tile early): level 0 is narrow,
    level 1 meets a wide octave without covering whole ones and takes the nibble form, level 2 is wide."""
    codes, tables, rows, _ = planted
    idx = make_index(pyqadc, [codes], 4, W=W, cap=CAP)
    wc, nc = idx.bktw_copy(0), idx.bkt_copy(0)
    got = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
    pr = idx.profile()
    idx.close()
    wide, nar = wm.check_copies(wc, nc, codes, W, TILE, CAP)
    assert all(l[4] for l in wide) and [l[4] > 0 for l in nar] == [True] * (W // TILE) + [False] * (13 - W // TILE)
    assert pr["bktw_copy_slots"] == sum(l[4] for l in wide) and pr["bkt_copy_slots"] == sum(l[4] for l in nar), pr
    assert pr["bkt_copy_bytes"] == pr["bkt_copy_slots"] // TILE * (100352 + 196608), pr
    check_profile(pr, 4)
    if W == TILE:
        assert (pr["bkt_launches"], pr["bktw_launches"], pr["nib_launches"]) == (1, 2, 0) and pr["nib_copy_bytes"] == 0, pr
    else:
        assert (pr["bkt_launches"], pr["bktw_launches"], pr["nib_launches"]) == (1, 1, 1) and pr["nib_copy_bytes"] > 0, pr
    for q in range(3):
        assert heaps_equal(got["heaps"][q], rows["heaps"][q]), q


@pytest.mark.parametrize("nsp", NSPS)
def test_last_octave_over_the_cap_falls_back_to_narrow_blocks(pyqadc, po, nsp):
    """8 tiles + 37: the last octave is the 37-code tail, a whole tile for 37 codes; and an octave of 16384 distinct keys (16 slots
    per code).  Both keep narrow blocks (counted), the levels over them take the narrow form or, mixed with a wide octave, the
    nibble form; the heaps do not change."""
    rng = np.random.default_rng(41)
    n = 8 * TILE + 37
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    kk = rng.permutation(1 << 20)[:12][rng.integers(0, 12, n)]
    set_key(codes, kk)
    set_key(codes[TILE:2 * TILE], rng.permutation(1 << 20)[:TILE])           # octave 0: every code its own key
    assert_under_cap(codes, TILE, LOOSE, fallback=(0, 3))
    tables = float_tables(rng, 2, 1, M)
    codes[-1] = narrow.best_code(tables[0, 0])
    out = {}
    for form in (nsp, "rows"):
        idx = make_index(pyqadc, [codes], form)
        if form != "rows":
            wm.check_copies(idx.bktw_copy(0), idx.bkt_copy(0), codes, TILE, TILE, LOOSE)
        out[form] = (idx.query_scan(np.zeros((2, 1), np.int32), tables.copy(), R), idx.profile())
        idx.close()
    pr = out[nsp][1]
    check_profile(pr, nsp, wide_launches=False)
    assert pr["bktw_copy_fallback"] == 2, pr
    # level 0 [0, 1): narrow; level 1 [1, 4): octave 0 fell back, octave 1 is wide: neither form, nibble; level 2 [4, 8 + 37 codes):
    # octave 2 wide, octave 3 narrow: nibble
    assert (pr["bkt_launches"], pr["bktw_launches"], pr["nib_launches"]) == (1, 0, 2), pr
    for q in range(2):
        assert heaps_equal(out[nsp][0]["heaps"][q], out["rows"][0]["heaps"][q]), q
        want = po.query_scan(M, [codes], None, 0.01, [0], tables[q, 0].copy(), R)
        assert want["rc"] == 0 and np.array_equal(out[nsp][0]["heaps"][q][0], want["keys"]) and np.array_equal(out[nsp][0]["heaps"][q][1], want["values"])


def few_wide_keys(rng, n, nkeys=16):
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    set_key(codes, rng.permutation(1 << 20)[:nkeys][rng.integers(0, nkeys, n)])
    return codes


@pytest.mark.parametrize("nsp", NSPS)
def test_short_tail_octave_is_narrow_and_still_matches(pyqadc, po, nsp):
    """4 tiles + 37: levels 1 (octaves 0-1, wide) and 2 (the 37-code octave: narrow blocks, a narrow launch of its own)."""
    rng = np.random.default_rng(43)
    n = 4 * TILE + 37
    codes = few_wide_keys(rng, n)
    tables = float_tables(rng, 2, 1, M)
    codes[-1] = narrow.best_code(tables[1, 0])
    out = {}
    for form in (nsp, "rows"):
        idx = make_index(pyqadc, [codes], form)
        out[form] = (idx.query_scan(np.zeros((2, 1), np.int32), tables.copy(), R), idx.profile())
        idx.close()
    pr = out[nsp][1]
    check_profile(pr, nsp)
    assert (pr["bkt_launches"], pr["bktw_launches"], pr["nib_launches"], pr["bktw_copy_fallback"]) == (2, 1, 0, 1), pr
    for q in range(2):
        assert heaps_equal(out[nsp][0]["heaps"][q], out["rows"][0]["heaps"][q]), q
        want = po.query_scan(M, [codes], None, 0.01, [0], tables[q, 0].copy(), R)
        assert want["rc"] == 0 and np.array_equal(out[nsp][0]["heaps"][q][0], want["keys"])
    assert np.count_nonzero(out[nsp][0]["heaps"][1][0] == n - 1) == 1 + (16 - n % 16) % 16


# ---- every row 5-15 in every role, in one launch -------------------------------------------------------------------------------

def window(k, nsp):
    """11 - nsp consecutive sub-quantizers of 5..15 from 5 + k on, cyclically."""
    return [5 + (k + i) % 11 for i in range(11 - nsp)]


def window_tables(rng, nsp):
    """16 int8 tables: the rule defers window(k, nsp) for table k < 11; tables 11..15 defer every second row from 5 + (k - 11) on
    (and the top rows): the parity of a paid row's place in the ascending list changes, so it is the low and the high member of a
    pair somewhere.  Even k: deferred rows hold 12..14 (a large c), the others 0..13; odd k: 0..2, the others 8..39.  Row 4 is
    always spread wide, 0..39 with a flat stretch in table 0 (it is never deferred, however it scores)."""
    qt = np.empty((16, 1, M, 16), np.int8)
    want = []
    for k in range(16):
        flat = k % 2 == 0
        qt[k, 0] = rng.integers(0, 14, (M, 16)) if flat else rng.integers(8, 40, (M, 16))
        if k < 11:
            deferred = window(k, nsp)
        else:
            comb = [5 + (k - 11 + 2 * i) % 11 for i in range(5)]
            deferred = (comb + [s for s in range(15, 4, -1) if s not in comb])[:11 - nsp]
        for s in deferred:
            qt[k, 0, s] = rng.integers(12, 15, 16) if flat else rng.integers(0, 3, 16)
        qt[k, 0, 4] = rng.permutation(16) * 2 + (0 if flat else 8) if k else 13
        want.append(sum(1 << s for s in deferred))
    return qt, want


def roles_of(masks, nsp):
    """-> (deferred, fused with row 4, low of a pair, high of a pair) under the masks (scan_bkt_body: an odd NSP fuses the first
    paid row with row 4 and pairs the rest; an even NSP pairs all of them)."""
    deferred, fused, low, high = set(), set(), set(), set()
    for m in masks:
        paid = bs.bktw_paid(m)
        assert len(paid) == nsp
        deferred |= {s for s in range(M) if m >> s & 1}
        rest = paid[1:] if nsp % 2 else paid
        fused |= set(paid[:1]) if nsp % 2 else set()
        low |= set(rest[0::2])
        high |= set(rest[1::2])
    return deferred, fused, low, high


@pytest.mark.parametrize("nsp", NSPS)
def test_wide_every_row_in_every_role_in_one_launch(pyqadc, po, nsp):
    rng = np.random.default_rng(3000 + nsp)
    n = 4 * TILE + 37
    codes = few_wide_keys(rng, n, 40)
    qt, want_masks = window_tables(rng, nsp)
    chosen = [bs.choose_bktw(qt[k, 0], nsp) for k in range(16)]
    assert [m for m, _ in chosen] == want_masks
    assert all(12 * (11 - nsp) <= c < 127 if k % 2 == 0 else c <= 16 for k, (_, c) in enumerate(chosen)), chosen
    deferred, fused, low, high = roles_of(want_masks, nsp)
    every = set(range(5, M))
    assert deferred == every, deferred
    if nsp % 2:
        # the ascending paid list: the fused row is its first (one of the lowest 12 - nsp rows), the last is a high member
        assert fused == set(range(5, 5 + 12 - nsp)) and high == every - {5, 6} and low == every - {5, 15}, (fused, low, high)
    else:
        assert fused == set() and low == every - {15} and high == every - {5}, (low, high)
    got_choice = pyqadc.bktw_choice(qt)
    assert got_choice[:, nsp - 3].tolist() == [[m & 0xff, m >> 8, c, 0] for m, c in chosen]
    Rr = 150
    rows = narrow.once(("wide-roles", nsp, "rows"), lambda: scan(pyqadc, [codes], "rows", qt, Rr, int8=True))[0]
    got, pr = scan(pyqadc, [codes], nsp, qt, Rr, int8=True)
    check_profile(pr, nsp)
    assert 0 < pr["bktw_survivors"] < pr["bktw_slots"], pr
    narrow.assert_rows(got, rows, 16)
    narrow.assert_reference_i8(got, narrow.reference_i8(po, ("wide-roles", nsp), [codes], None, qt, (0, 5, 10, 13, 15), Rr))


def scan(pyqadc, parts, form, tables, R, int8=False, labels=None, assign=None, keep=0.01, **kw):
    assign = np.zeros((len(tables), 1), np.int32) if assign is None else assign
    idx = make_index(pyqadc, parts, form, labels, keep=keep, **kw)
    try:
        res = idx.scan_i8(assign, tables, R) if int8 else idx.query_scan(assign, tables.copy(), R, want_qtables=True)
        return res, idx.profile()
    finally:
        idx.close()


def test_wide_choice_bytes_equal_the_twin(pyqadc):
    rng = np.random.default_rng(78)
    qt = np.concatenate([rng.integers(0, hi, (40, M, 16)) for hi in (2, 5, 30, 128)]).astype(np.int8)
    qt[0] = 0                                                    # all rows equal
    qt[1] = 127
    qt[2, 8:] = qt[2, :8]                                        # pairs of equal rows: ties
    qt[3:40, 4] = 7                                              # a flat row 4 scores 0: the rule among 4-15 would defer it first
    got = pyqadc.bktw_choice(qt)
    want = [[[m & 0xff, m >> 8, c, 0] for m, c in (bs.choose_bktw(qt[t], nsp) for nsp in NSPS)] for t in range(len(qt))]
    assert got.tolist() == want
    assert got[0].tolist() == [[0x00, 0xff, 0, 0], [0x00, 0xfe, 0, 0], [0x00, 0xfc, 0, 0], [0x00, 0xf8, 0, 0]]
    assert not np.any(got[:, :, 0] & 0x1f)                       # rows 0-4 are never deferred
    # the narrow choice keeps its layout and its rule
    assert pyqadc.bkt_choice(qt[:8]).tolist() == [[[m & 0xff, m >> 8, c, 0] for m, c in (bs.choose_bkt(qt[t], p) for p in (4, 5, 6, 7))] for t in range(8)]


# ---- slack edges, entries of 127, ties -----------------------------------------------------------------------------------------

EDGE_C = {"clamp": lambda nsp: 127, "c0": lambda nsp: 0, "reach": lambda nsp: 2 * (11 - nsp), "sat": lambda nsp: 4 * (11 - nsp)}


@pytest.mark.parametrize("case", ["clamp", "c0", "c0-every-candidate", "reach", "sat"])
@pytest.mark.parametrize("nsp", NSPS)
def test_wide_slack_edges(pyqadc, po, nsp, case):
    """The narrow suite's edge tables (test_gpu_bkt_scan.edge_tables): under the wide rule they defer rows 5 + NSP .. 15.  clamp: 127
    in deferred rows, c = 127, no survivor.  c0: c = 0, bsurv = bound.  c0-every-candidate: R above the number of codes below 127:
    the heap keeps every candidate, those of value 126 too, which a c one too large loses.  reach: every sum is >= 16 = c + the
    smallest partial: bound - c equals the smallest partial and nothing survives the later levels.  sat: 127 in free and paid
    rows: min(127, partial) is never below a bound.  All rows but a few entries are constant: ties everywhere."""
    base = case.split("-")[0]
    rng = np.random.default_rng({"clamp": 500, "c0": 501, "reach": 502, "sat": 503}[base])      # the same tables for every NSP: the rows result is shared
    n = 4 * TILE + 37
    codes = few_wide_keys(np.random.default_rng(44), n)
    qt = narrow.edge_tables(rng, base)
    m, c = bs.choose_bktw(qt[0, 0], nsp)
    assert (m, c) == (sum(1 << s for s in range(5 + nsp, M)), EDGE_C[base](nsp)), (m, c)
    Rr = {"clamp": 300, "c0": 300, "c0-every-candidate": 4000, "reach": 50, "sat": 300}[case]
    rows = narrow.once(("wide-edge", case, "rows"), lambda: scan(pyqadc, [codes], "rows", qt, Rr, int8=True))[0]
    got, pr = scan(pyqadc, [codes], nsp, qt, Rr, int8=True)
    check_profile(pr, nsp)
    narrow.assert_rows(got, rows, 2)
    narrow.assert_reference_i8(got, narrow.reference_i8(po, ("wide-edge", case), [codes], None, qt, (0,), Rr))
    if base in ("clamp", "sat", "reach"):
        assert pr["bktw_survivors"] == 0, pr
    if case == "c0-every-candidate":
        for q in range(2):                                       # the row-major form's heap: not full, and it holds the value 126
            assert len(narrow.heaps_of(rows, q)[1]) < Rr and np.count_nonzero(narrow.heaps_of(rows, q)[1] == 126) >= 10, q


# ---- partitions, shards, thresholds, lifecycle -----------------------------------------------------------------------------------

@pytest.mark.parametrize("nsp", NSPS)
def test_wide_labels_and_two_partitions_in_one_launch(pyqadc, po, nsp):
    """Two labelled partitions of four tiles (+ 37); query 0 probes 0 then 1, query 1 probes 1 then 0: level 1 is [1, 4) tiles of
    partition 0 for query 0 and of partition 1 for query 1, one wide launch of two runs.  Level 2 holds a whole second partition per
    query (it starts at position 0: neither form, and it meets wide octaves: not narrow) beside query 1's narrow 37-code tail: a
    mixed launch, all nibble."""
    rng = np.random.default_rng(19)
    sizes = [4 * TILE, 4 * TILE + 37]
    parts = [few_wide_keys(rng, s) for s in sizes]
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    tables = float_tables(rng, 2, 2, M)
    parts[1][-1] = narrow.best_code(tables[0, 1])
    parts[0][3 * TILE + 5] = narrow.best_code(tables[0, 0])        # a candidate inside partition 0's wide octave 1: its label
    assign = np.array([[0, 1], [1, 0]], np.int32)
    out = {}
    for form in (nsp, "rows"):
        idx = make_index(pyqadc, parts, form, labels)
        out[form] = (idx.query_scan(assign, tables.copy(), R), idx.profile())
        idx.close()
    pr = out[nsp][1]
    check_profile(pr, nsp)
    assert pr["bktw_launches"] == 1 and pr["bktw_codes"] == 2 * 3 * TILE and pr["bkt_launches"] == 1 and pr["nib_launches"] == 1, pr
    assert np.all(out[nsp][0]["status"] == 0)
    for q in range(2):
        assert heaps_equal(out[nsp][0]["heaps"][q], out["rows"][0]["heaps"][q]), q
        want = po.query_scan(M, parts, labels, 0.01, assign[q].tolist(), tables[q].copy(), R)
        assert want["rc"] == 0 and np.array_equal(out[nsp][0]["heaps"][q][0], want["keys"]) and np.array_equal(out[nsp][0]["heaps"][q][1], want["values"])
    assert np.count_nonzero(out[nsp][0]["heaps"][0][0] == labels[0][3 * TILE + 5]) == 1


@pytest.mark.parametrize("nsp", NSPS)
def test_wide_range_shard_with_an_odd_first_pos_and_key_base(pyqadc, nsp):
    """The last shard of the planted size from first_pos = 18 (2 mod 16) on, key_base 1000: the octaves are cut in the shard's LOCAL
    positions, keys are key_base + first_pos + perm.  The shard's ordered streams equal the row-major form's of the same shard,
    which tests/test_gpu_shard_forms.py pins to the unsharded oracle."""
    rng = np.random.default_rng(47)
    n, first, keep = N12 + 18, 18, 0.01
    codes = few_wide_keys(rng, n, 24)
    tables = float_tables(rng, 2, 1, M)
    codes[-1] = narrow.best_code(tables[0, 0])
    out = {}
    for form in (nsp, "rows"):
        idx = make_index(pyqadc, None, form, finalize=False)
        idx.add_partition_shard(codes[first:], first, n, starts=codes[:start_size(n, keep)])
        idx.set_key_base(0, 1000)
        idx.finalize(keep)
        idx.set_option("profile", 1)
        if form != "rows":
            wm.check_copies(idx.bktw_copy(0), idx.bkt_copy(0), codes[first:], TILE, TILE, LOOSE)
        out[form] = (idx.query_scan_shard_streams(np.zeros((2, 1), np.int32), tables.copy(), R), idx.profile())
        idx.close()
    pr = out[nsp][1]
    check_profile(pr, nsp)
    assert pr["bktw_launches"] == 2 and pr["bktw_codes"] == 2 * (N12 - TILE), pr
    a, b = out[nsp][0], out["rows"][0]
    assert np.all(a["status"] == 0) and np.array_equal(a["offsets"], b["offsets"])
    for q in range(2):
        lo, hi = int(a["offsets"][q]), int(a["offsets"][q + 1])
        sa = np.lexsort((a["vals"][lo:hi], a["keys"][lo:hi], a["slots"][lo:hi]))
        sb = np.lexsort((b["vals"][lo:hi], b["keys"][lo:hi], b["slots"][lo:hi]))
        for k in ("keys", "vals", "slots"):
            assert np.array_equal(a[k][lo:hi][sa], b[k][lo:hi][sb]), (q, k)
        assert a["keys"][lo:hi].min() >= 1000 + first
    last = 1000 + n - 1
    assert np.count_nonzero(a["keys"][:int(a["offsets"][1])] == last) == 1 + (16 - n % 16) % 16


def test_wide_thresholds_pick_the_paid_planes_per_launch(pyqadc, planted):
    """Level 1's runs have 3 tiles, level 2's 8 tiles + 37: thresholds between them give the launches different paid counts; a
    min_run above both turns the form off for that launch only (the planner then has no bucket form for a wide range: nibble)."""
    codes, tables, rows, _ = planted
    cases = [((1, 3 * TILE, 3 * TILE + 1, 0), {5: 1, 4: 1}), ((1, 0, 0, 8 * TILE), {6: 1, 3: 1}), ((1, 1, 1, 1), {3: 2}),
             ((3 * TILE + 1, 0, 4 * TILE, 0), {4: 1}), ((1, 0, 0, 0), {6: 2})]
    idx = make_index(pyqadc, [codes], 6, cap=CAP)
    try:
        for thr, want in cases:
            idx.set_split_bkt_wide(TILE, *thr, CAP)               # thresholds may change after finalize; W and the cap may not
            idx.profile_reset()
            got = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
            pr = idx.profile()
            assert {p: pr["bktw%d_launches" % p] for p in NSPS if pr["bktw%d_launches" % p]} == want, (thr, pr)
            assert pr["bktw_launches"] == sum(want.values()) and pr["bkt_launches"] == 1, (thr, pr)
            assert pr["nib_launches"] + pr["split5_launches"] == 2 - sum(want.values()), (thr, pr)
            for q in range(3):
                assert heaps_equal(got["heaps"][q], rows["heaps"][q]), (thr, q)
        with pytest.raises(pyqadc.QadcError, match="finalize"):
            idx.set_split_bkt_wide(2 * TILE, 1, 0, 0, 0, CAP)
        with pytest.raises(pyqadc.QadcError, match="power of two"):
            idx.set_split_bkt_wide(3 * TILE, 1, 0, 0, 0, CAP)
    finally:
        idx.close()


@pytest.mark.parametrize("nsp", NSPS)
def test_wide_copy_is_rebuilt_after_remove_and_finalize(pyqadc, po, nsp):
    rng = np.random.default_rng(53)
    n = 8 * TILE + 37
    codes = few_wide_keys(rng, n, 24)
    labels = rng.permutation(3 * n)[:n].astype(np.uint32)
    tables = float_tables(rng, 2, 1, M)
    assign = np.zeros((2, 1), np.int32)
    idx = make_index(pyqadc, [codes], nsp, [labels])
    try:
        def check(cur_codes, cur_labels, what):
            wide, _ = wm.check_copies(idx.bktw_copy(0), idx.bkt_copy(0), cur_codes, TILE, TILE, LOOSE)
            idx.profile_reset()
            got = idx.query_scan(assign, tables.copy(), R)
            pr = idx.profile()
            assert pr["bktw_copy_slots"] == sum(l[4] for l in wide) and pr["bktw_launches"] > 0, (what, pr)
            for q in range(2):
                want = po.query_scan(M, [cur_codes], [cur_labels], 0.01, [0], tables[q, 0].copy(), R)
                assert want["rc"] == 0 and np.array_equal(got["heaps"][q][0], want["keys"]) and np.array_equal(got["heaps"][q][1], want["values"]), (what, q)
        check(codes, labels, "built")
        gone = labels[rng.permutation(n)[:TILE + 100]]
        assert idx.remove_labels(gone) == len(gone)
        got_codes, got_labels = idx.read_partition(0)
        assert len(got_codes) == n - len(gone)
        idx.finalize(0.01)
        check(got_codes, got_labels, "after remove")             # 7 tiles - 63 codes: the last octave is clipped elsewhere
        idx.finalize(0.01)
        check(got_codes, got_labels, "finalized again")
    finally:
        idx.close()


@pytest.mark.parametrize("nsp", NSPS)
def test_wide_copy_is_rebuilt_after_growth(pyqadc, po, nsp):
    """add_vectors on a finalized index, W = one tile.  The partition starts at 4 tiles + 37: octaves [1, 2), [2, 4) wide, the 37-code
    tail narrow.  A first append of one tile + 3000 rows turns that tail into a wide octave [4 tiles, 5 tiles + 3037); a second one
    carries the partition across the boundary at 8 tiles: the octave [4, 8) is whole and a new one, [8 tiles, 8 tiles + 9000), opens.
    After each finalize both copies equal the model built from the rows the index holds (a stale bktw_off, bktw_block or wide range
    of the earlier build would leave rows out or twice), and the heaps equal the oracle's on those rows.  The appended vectors are
    the coarse centroid plus one codebook entry per sub-quantizer, so they encode to codes with 16 distinct 20-bit keys (checked)."""
    from test_gpu_index_add import Quantizers4
    rng = np.random.default_rng(61)
    n0, a1, n2 = 4 * TILE + 37, TILE + 3000, 8 * TILE + 9000
    nadd = n2 - n0
    q = Quantizers4(M, 16, K=1, n=8, seed=11)
    want = few_wide_keys(rng, nadd)
    nib = np.empty((nadd, M), np.uint8)
    nib[:, 0::2], nib[:, 1::2] = want & 15, want >> 4
    q.vectors = (q.coarse[0][None, :] + q.codebooks[np.arange(M)[None, :], nib, 0]).astype(np.float32)
    q.cache = {}
    assign_new, new_codes = q.encoded()
    assert not assign_new.any() and len(np.unique(wm.keys_of(new_codes))) <= 24
    codes = few_wide_keys(rng, n0)
    labels = rng.permutation(3 * n0)[:n0].astype(np.uint32)
    tables = float_tables(rng, 2, 1, M)
    assign = np.zeros((2, 1), np.int32)
    idx = make_index(pyqadc, [codes], nsp, [labels], idx=q.index())
    try:
        def check(cur_codes, cur_labels, wide_flags, what):
            got_codes, got_labels = idx.read_partition(0)
            assert np.array_equal(got_codes, cur_codes) and np.array_equal(got_labels, cur_labels), what
            wide, _ = wm.check_copies(idx.bktw_copy(0), idx.bkt_copy(0), cur_codes, TILE, TILE, LOOSE)
            assert [l[4] > 0 for l in wide] == wide_flags, (what, [(l[0], l[1], l[4]) for l in wide])
            idx.profile_reset()
            got = idx.query_scan(assign, tables.copy(), R)
            pr = idx.profile()
            check_profile(pr, nsp)
            assert pr["bktw_copy_slots"] == sum(l[4] for l in wide) and pr["bktw_copy_fallback"] == wide_flags.count(False), (what, pr)
            for qi in range(2):
                w = po.query_scan(M, [cur_codes], [cur_labels], 0.01, [0], tables[qi, 0].copy(), R)
                assert w["rc"] == 0 and np.array_equal(got["heaps"][qi][0], w["keys"]) and np.array_equal(got["heaps"][qi][1], w["values"]), (what, qi)
            return pr
        pr = check(codes, labels, [True, True, False], "built")
        assert pr["bktw_launches"] == 1 and pr["bkt_launches"] == 2, pr       # level 2 is the narrow 37-code tail
        idx.add_vectors(q.vectors[:a1], labels_offset=3 * n0 + 7)
        idx.finalize(0.01)
        codes1 = np.concatenate([codes, new_codes[:a1]])
        labels1 = np.concatenate([labels, (np.arange(a1) + 3 * n0 + 7).astype(np.uint32)])
        pr = check(codes1, labels1, [True, True, True], "the tail turned wide")
        assert pr["bktw_launches"] == 2 and pr["bkt_launches"] == 1, pr
        idx.add_vectors(q.vectors[a1:], labels_offset=3 * n0 + 7 + a1)
        idx.finalize(0.01)
        codes2 = np.concatenate([codes, new_codes])
        labels2 = np.concatenate([labels, (np.arange(nadd) + 3 * n0 + 7).astype(np.uint32)])
        pr = check(codes2, labels2, [True, True, True, True], "across the octave boundary at 8 tiles")
        assert pr["bktw_launches"] == 2 and pr["bktw_codes"] == 2 * (n2 - TILE), pr
    finally:
        idx.close()


def test_a_block_raised_above_w_raises_the_octaves_start(pyqadc, planted):
    """qadc_index_set_split_bkt after the wide setter may make bkt_block larger than W: finalize then starts the octaves at bkt_block
    (every narrow block still lies inside one octave or outside all), the diagnostic reports it, and the heaps do not change."""
    codes, tables, rows, _ = planted
    idx = make_index(pyqadc, None, 4, W=TILE, cap=LOOSE, finalize=False)
    idx.set_split_bkt(1, 2 * TILE, 1, 0, 0, 1e6)
    idx.add_partitions([codes])
    idx.finalize(0.01)
    idx.set_option("profile", 1)
    wc, nc = idx.bktw_copy(0), idx.bkt_copy(0)
    got = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
    pr = idx.profile()
    idx.close()
    assert wc is not None and wc["block"] == 2 * TILE
    wm.check_copies(wc, nc, codes, 2 * TILE, 2 * TILE, LOOSE)
    check_profile(pr, 4)
    assert pr["bktw_launches"] == 1, pr                          # the level from 4 tiles on; [1, 4) tiles starts off the octaves
    for q in range(3):
        assert heaps_equal(got["heaps"][q], rows["heaps"][q]), q
