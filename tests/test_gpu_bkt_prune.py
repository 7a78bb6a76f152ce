"""GPU: the group test of the wide bucket form ("pruned groups"; qadc_index_set_bkt_prune).  A 16-slot lane
group whose free rows already reach the bound, s0 + pmin >= bsurv, holds no survivor; a wave iteration whose 64 groups are all
like that loads no plane.  Nothing a caller sees may change: every case compares heaps bit for bit with the row-major form and the
reference.  Every case builds ONE index and runs it with the option at 0 and at 1, under both loop forms and with one workgroup per
run, and compares the launch counters, the candidates and the survivor counter between the two values.  (One index, because the
survivor counter counts padding slots, and those hold a copy of whichever code the copy's scatter put last in its bucket or block:
their survivors, up to a tile's remainder at once, change from one finalize to the next, with any kernel.)  Every test sets wgq and
head_level itself, so the scan paths of tests/conftest.py would run the same launches thrice.

The planted list (12 tiles + 37, W = one tile: levels 1 and 2 are wide launches over octaves of 1, 2, 4 and 4 tiles + 37) is scanned
with int8 tables brought by the caller and R above the number of codes below 127, so the bound stays 127 and bsurv = 127 - c is
known: the groups the kernel must prune follow from the copy's ids and tools/bucket_prune.py's terms, and the three counters
(wave iterations skipped, run, lane groups pruned) are compared EXACTLY.  A key is (segment number << 4) | n0: row 0 alone decides
how hot a group is (T0 = 0 hot, 123 the edge that must be kept, 124 the edge that must be pruned, 127 cold), segments are laid out
in key order, so the list decides which lanes of which waves keep:
  octave 0 (1 tile): a hot group with the best code in wave 0, everything else cold; octave 1 (2 tiles): all cold: under one
      workgroup per run level 1 is a kept tile with a candidate, then only skipped tiles (late resolve and emit in skipped iterations)
  octave 2 (4 tiles): waves in which exactly lane 0, lane 63, lane 31, lane 32 keeps; a tile in which exactly one wave keeps;
      two tiles skipped whole; both edge groups, each with the code whose other rows are all at their minimum
  octave 3 (4 tiles + 37): skipped tiles first, a hot bucket across a tile boundary, buckets with padding slots (hot and cold), a
      key whose row 4 alone pushes it over the bound (pruned for an even NSP, kept for an odd one, where row 4 is fused and counts
      with its minimum), key 0xfffff with 127 in all five free rows (s0 = 635: an 8-bit sum would wrap to 123 and keep it), and the
      copy's last kept group (n4 = 2) in its last tile: skipped tiles, then a kept one whose candidates leave through the drain behind the loop
Table 1 is 127 everywhere (c = 127: bsurv = 0, every wave skipped, no result), table 2 has free rows of 0 (nothing pruned).

Mutants and what catches them: pmin one too large, or a kept edge lost -> the value-126 code of the edge group (heaps);
>= written as >, row 4's minimum left out of pmin or T4[id4] added to s0 under FUSE, an 8-bit s0 -> the exact counters;
pend / res not carried across a skipped iteration, ids of the wrong tile after a skip -> heaps (one workgroup per run and chunked)."""
import os
import sys

import numpy as np
import pytest

import bktw_model as wm
import test_gpu_bkt_scan as narrow
import test_gpu_bktw_scan as wide
from dist_cases import start_size
from helpers import float_tables, heaps_equal, path_independent
from test_gpu_bktw_scan import planted  # noqa: F401  (the wide suite's planted list, float tables: the bound tightens level by level)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bucket_prune as bp  # noqa: E402
import bucket_survivors as bs  # noqa: E402

pytestmark = pytest.mark.gpu
M, TILE, NSPS, LOOSE = wide.M, wide.TILE, wide.NSPS, wide.LOOSE
MODES = (0, 1)                  # every value of the option kept in the tree
WAVE = 64 * 16                  # slots of a wave iteration
R_ALL = 4000                    # above the number of codes below 127: the bound stays 127
LOOPS = [dict(variant=0x0d), dict(variant=0x01), dict(variant=0x01, wgs_per_item=1)]
LOOP_IDS = ["chunked", "grid-stride", "grid-stride-one-workgroup"]
HOT, EDGE_KEEP, EDGE_PRUNE, COLD, COLD2, ALL127 = 0, 1, 2, 3, 4, 15      # n0 of a key: see plant_tables


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def plant_tables(rng):
    """int8 [3, 1, 16, 16]: the planted table, all 127, free rows 0 (the module's docstring).  Rows 5-15 of table 0 are random in
    0..15 with 0 at nibble 0: c = 0 and pmin = 0 whatever the rule defers (+ 3 = min T4 under FUSE), so s0 + pmin reaches
    bsurv = 127 exactly at T0 = 124 for both parities."""
    qt = np.zeros((3, 1, M, 16), np.int8)
    t = qt[0, 0]
    t[5:] = rng.integers(0, 16, (11, 16))
    t[5:, 0] = 0
    t[0] = 127
    t[0, [HOT, EDGE_KEEP, EDGE_PRUNE]] = 0, 123, 124
    t[4] = 3
    t[4, 1] = 127                                                # row 4 alone reaches the bound at n4 = 1
    t[1:5, 15] = 127                                             # key 0xfffff: 5 x 127
    qt[1] = 127
    qt[2, 0, 5:] = 20                                            # a code is below 127 with at most 6 of its 11 late nibbles non-zero: a few dozen
    qt[2, 0, 5:, 0] = 0
    return qt


def segment(rng, key, groups, codes=None, first=None):
    """`groups` lane groups of one key (codes: fewer than 16 x groups leaves padding slots), the first code given or random."""
    n = 16 * groups if codes is None else codes
    c = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    if first is not None:
        c[0] = first
    wide.set_key(c, np.full(n, key))
    return c


def plant_codes(rng):
    """The planted list and the best code's position.  Octaves are filled by (n0, groups) segments whose keys ascend."""
    zero_late = np.zeros(M // 2, np.uint8)                       # every row 5-15 at nibble 0: their minimum
    seg = [-1]

    def next_key(n0):
        seg[0] += 1
        while any((seg[0] >> sh) & 15 == 15 for sh in (0, 4, 8)):    # rows 1-3 hold 127 at nibble 15: 0xfffff alone has it
            seg[0] += 1
        assert seg[0] < 1 << 12                                  # n4 = 0
        return (seg[0] << 4) | n0

    def fill(spec, slots):
        out = [segment(rng, next_key(n0), groups, **(kw[0] if kw else {})) for n0, groups, *kw in spec]
        used = sum(len(o) for o in out)
        assert used <= slots
        while used < slots:                                      # cold to the octave's end, in buckets of at most 300 groups
            g = min(300, (slots - used + 15) // 16)
            out.append(segment(rng, next_key(COLD if len(out) % 2 else COLD2), g, codes=min(16 * g, slots - used)))
            used += len(out[-1])
        out = np.concatenate(out)
        return out[rng.permutation(len(out))]

    head = rng.integers(0, 256, (TILE, M // 2), dtype=np.uint8)
    head[:, 0] = (head[:, 0] & 0xf0) | COLD                      # level 0 and the starts: no code below 127
    o0 = fill([(HOT, 1, dict(first=zero_late))], TILE)           # key 0x00000, the best code: value 3
    o1 = fill([], 2 * TILE)
    one = [(COLD, 63)]
    o2 = fill([(HOT, 1)] + one +                                             # wave 0: lane 0
              one + [(HOT, 1)] +                                             # wave 1: lane 63
              [(COLD, 31), (HOT, 1), (COLD2, 32)] +                          # wave 2: lane 31
              [(COLD, 32), (HOT, 1), (COLD2, 31)] +                          # wave 3: lane 32
              [(COLD, 64), (EDGE_KEEP, 1, dict(first=zero_late)), (COLD, 31), (EDGE_PRUNE, 1, dict(first=zero_late)), (COLD, 31)] +
              [(COLD, 300), (COLD2, 340)] +                                  # ... to the end of tile 0 (1024 groups)
              [(COLD, 320), (HOT, 1)],                                       # tile 1: wave 5, lane 0; tiles 2 and 3: cold
              4 * TILE)
    last = 4 * TILE + 37
    o3 = fill([(COLD, 300), (COLD2, 300), (COLD, 300), (COLD2, 122),         # 1022 groups: the hot bucket crosses into tile 1
               (HOT, 4), (COLD, 50), (HOT, 2, dict(codes=19)), (COLD2, 3, dict(codes=33))],
              last - 37)
    # n4 = 1: row 4 decides; n4 = 2 (T4 = 3): hot, the copy's last kept group, in its last tile; 0xfffff
    tail = [segment(rng, (1 << 16) | HOT, 1), segment(rng, (2 << 16) | HOT, 1), segment(rng, 0xfffff, 1, codes=5)]
    o3 = np.concatenate([o3] + tail)
    o3 = o3[rng.permutation(len(o3))]
    codes = np.ascontiguousarray(np.concatenate([head, o0, o1, o2, o3]))
    assert len(codes) == wide.N12
    return codes


def expected_counters(copy, first_octave, qt, nsp, bound=127):
    """(skipped, run, groups) of one query's wide launches over the octaves from first_octave on, from the copy's own ids."""
    lo = int(copy["off"][first_octave]) // 16
    keys = wm.keys_of(copy["codes"][0::16])[lo:]
    s0, pmin, bsurv = bp.wide_terms(qt, nsp, bound)
    pruned = ~(s0[keys] + pmin < bsurv)
    waves = pruned.reshape(-1, 64).all(axis=1)
    return int(waves.sum()), int(len(waves) - waves.sum()), int(pruned.sum())


def both_modes(idx, run):
    """{mode: (result, profile)} of `run(idx)` with the option at every value, on ONE index: the copy is the same for both (its
    padding slots hold whichever code the scatter put last, so their survivors differ from one finalize to the next)."""
    out = {}
    for mode in MODES:
        idx.set_bkt_prune(mode)
        idx.profile_reset()
        res = run(idx)
        out[mode] = (res, idx.profile())
    return out


def scan_i8(pyqadc, codes, form, qt, W=TILE, **opts):
    """-> ({mode: (heaps, profile)}, the wide copy) of the planted tables on a fresh index (form "rows": mode 0 alone)."""
    idx = wide.make_index(pyqadc, [codes], form, W=W, cap=LOOSE, **opts)
    try:
        run = lambda ix: ix.scan_i8(np.zeros((len(qt), 1), np.int32), qt, R_ALL)      # noqa: E731
        if form == "rows":
            return {0: (run(idx), idx.profile())}, None
        copy = idx.bktw_copy(0)
        return both_modes(idx, run), copy
    finally:
        idx.close()


@pytest.fixture(scope="module")
def plant(pyqadc, po):
    rng = np.random.default_rng(1313)
    qt = plant_tables(rng)
    codes = plant_codes(rng)
    rows = scan_i8(pyqadc, codes, "rows", qt)[0][0][0]
    ref = narrow.reference_i8(po, ("prune-plant",), [codes], None, qt, (0, 1, 2), R_ALL)
    v0 = rows[0][1]
    # the heap keeps every candidate: not full; the best code (3) and the edge group's code (126) are in it
    below = [int(np.count_nonzero(rows[q][1] < 127)) for q in range(3)]       # (a heap that is not full may hold a 127 sentinel)
    assert all(len(rows[q][1]) < R_ALL for q in range(3)) and below[1] == 0 and 10 < below[2] < 1000, below
    assert v0.min() == 3 and np.count_nonzero(v0 == 126) >= 1 and 100 < below[0] < 2000, below
    return codes, qt, rows, ref


def check_counters(pr, mode, want):
    got = (pr["bktw_prune_skipped"], pr["bktw_prune_run"], pr["bktw_prune_groups"])
    assert got == (tuple(want) if mode else (0, 0, 0)), (got, want)


LAUNCH_KEYS = ("bktw_launches", "bktw_codes", "bktw_slots", "bkt_launches", "bkt_survivors", "nib_launches", "split_launches", "scan_launches",
               "candidates")


def check_modes_agree(out):
    """The option changes neither the launches nor the survivors; off, its counters stay 0; on, every wave iteration is counted once."""
    p0, p1 = out[0][1], out[1][1]
    assert [p0[k] for k in LAUNCH_KEYS] == [p1[k] for k in LAUNCH_KEYS], (p0, p1)
    assert p0["bktw_survivors"] == p1["bktw_survivors"], (p0["bktw_survivors"], p1["bktw_survivors"])
    check_counters(p0, 0, None)
    assert p1["bktw_prune_skipped"] + p1["bktw_prune_run"] == p1["bktw_slots"] // WAVE > 0, p1
    assert p1["bktw_prune_skipped"] * 64 <= p1["bktw_prune_groups"] <= p1["bktw_slots"] // 16, p1


@path_independent
@pytest.mark.parametrize("opts", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("W", [TILE, 2 * TILE], ids=["W1", "W2"])
@pytest.mark.parametrize("nsp", NSPS)
def test_planted_groups_counters_exact_and_heaps_unchanged(pyqadc, plant, nsp, W, opts):
    codes, qt, rows, ref = plant
    out, copy = scan_i8(pyqadc, codes, nsp, qt, W=W, **opts)
    first = 0 if W == TILE else 1                                          # W = two tiles: level 1 meets octave [2, 4) half: nibble form
    want = np.sum([expected_counters(copy, first, qt[q, 0], nsp) for q in range(3)], axis=0)
    for mode in MODES:
        got, pr = out[mode]
        wide.check_profile(pr, nsp)
        assert pr["bktw_launches"] == (2 if W == TILE else 1), pr
        narrow.assert_rows(got, rows, 3)
        narrow.assert_reference_i8(got, ref)
        check_counters(pr, mode, want)
        assert want[0] + want[1] == pr["bktw_slots"] // WAVE
    check_modes_agree(out)
    assert out[1][1]["bktw_survivors"] > 0


@path_independent
@pytest.mark.parametrize("opts", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("nsp", NSPS)
def test_each_table_alone_and_the_list_is_what_the_docstring_says(pyqadc, plant, nsp, opts):
    codes, qt, rows, _ = plant
    fuse = nsp % 2 == 1
    for q in range(3):
        out, copy = scan_i8(pyqadc, codes, nsp, qt[q:q + 1], **opts)
        want = expected_counters(copy, 0, qt[q, 0], nsp)
        for mode in MODES:
            got, pr = out[mode]
            assert heaps_equal(got[0], rows[q]), (q, mode)
            check_counters(pr, mode, want)
        check_modes_agree(out)
        pr = out[1][1]
        nwaves = pr["bktw_slots"] // WAVE
        if q == 1:
            assert want == (nwaves, 0, nwaves * 64) and pr["bktw_survivors"] == 0       # bsurv = 0: everything pruned
        if q == 2:
            assert want == (0, nwaves, 0)                                               # free rows 0: nothing pruned
    # the planted table: which lanes keep, wave by wave, from the copy
    keys = wm.keys_of(copy["codes"][0::16])
    s0, pmin, bsurv = bp.wide_terms(qt[0, 0], nsp, 127)
    assert (pmin, bsurv) == (3 if fuse else 0, 127)
    keep = (s0[keys] + pmin < bsurv).reshape(-1, 64)
    off = (copy["off"] // WAVE).astype(int)
    assert keep[off[0]].tolist() == [True] + [False] * 63 and not keep[off[0] + 1:off[2]].any()   # octaves 0 and 1
    o2 = keep[off[2]:off[3]]
    assert [np.nonzero(w)[0].tolist() for w in o2[:4]] == [[0], [63], [31], [32]]
    assert [np.nonzero(w)[0].tolist() for w in o2[4:7]] == [[], [0], []]                          # the kept edge at lane 0, the pruned one not
    assert o2[:16].any(axis=1).sum() == 5 and np.nonzero(o2[16:32].any(axis=1))[0].tolist() == [5] and not o2[32:].any()
    o3 = keep[off[3]:]
    assert not o3[:15].any() and o3[15].tolist() == [False] * 62 + [True] * 2 and o3[16, :2].all()  # skipped tiles, then the hot bucket across the boundary
    # row 4 decides: the hot key with n4 = 1 is kept only where row 4 is fused (an odd NSP); 0xfffff (s0 = 635 or 508) is pruned
    k1 = np.nonzero(keys == (1 << 16))[0]
    assert len(k1) == 1 and (s0[1 << 16] + pmin < bsurv) == fuse and s0[0xfffff] == (508 if fuse else 635) and (keys == 0xfffff).sum() >= 1
    assert (keys == 0).sum() == 1
    k2 = np.nonzero(keys == (2 << 16))[0]                         # the last kept group: a candidate pending when the loop ends
    assert len(k2) == 1 and k2[0] >= off[3] * 64 + 4096 and keep.reshape(-1)[k2[0]] and not keep.reshape(-1)[k2[0] + 1:].any()
    pad = copy["perm"].reshape(-1, 16) == wm.PAD
    assert pad[keep.reshape(-1)].any() and pad[~keep.reshape(-1)].any()                           # padding slots in kept and in pruned groups


@path_independent
@pytest.mark.parametrize("opts", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("nsp", NSPS)
def test_float_tables_over_tightening_levels(pyqadc, planted, nsp, opts):  # noqa: F811
    """The wide suite's planted list with float tables: the bound tightens from launch to launch, keys 0x00000 and 0xfffff, buckets
    of 1, 15, 16 and 17 codes, a bucket across tiles, the best code in a padded last group."""
    codes, tables, rows, oracle = planted
    idx = wide.make_index(pyqadc, [codes], nsp, cap=wide.CAP, **opts)
    try:
        out = both_modes(idx, lambda ix: ix.query_scan(np.zeros((3, 1), np.int32), tables.copy(), wide.R))
    finally:
        idx.close()
    for mode in MODES:
        got, pr = out[mode]
        wide.check_profile(pr, nsp)
        assert np.array_equal(got["status"], rows["status"])
        for q in range(3):
            assert heaps_equal(got["heaps"][q], rows["heaps"][q]), q
            assert np.array_equal(got["heaps"][q][0], oracle[q]["keys"]) and np.array_equal(got["heaps"][q][1], oracle[q]["values"]), q
    check_modes_agree(out)
    assert out[1][1]["bktw_survivors"] > 0


@path_independent
@pytest.mark.parametrize("opts", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("nsp", NSPS)
def test_sixteen_tables_with_their_own_pmin_in_one_launch(pyqadc, po, nsp, opts):
    """The wide suite's window tables: 16 tables in one launch, every row 5-15 paid somewhere and deferred somewhere: pmin and c
    differ from table to table."""
    rng = np.random.default_rng(3000 + nsp)
    n = 4 * TILE + 37
    codes = wide.few_wide_keys(rng, n, 40)
    qt, _ = wide.window_tables(rng, nsp)
    pmins = {bp.wide_terms(qt[k, 0], nsp, 127)[1] for k in range(16)}
    assert len(pmins) >= 8, pmins
    rows = narrow.once(("prune-roles", nsp, "rows"), lambda: wide.scan(pyqadc, [codes], "rows", qt, 150, int8=True))[0]
    ref = narrow.reference_i8(po, ("prune-roles", nsp), [codes], None, qt, (0, 5, 10, 13, 15), 150)
    idx = wide.make_index(pyqadc, [codes], nsp, **opts)
    try:
        out = both_modes(idx, lambda ix: ix.scan_i8(np.zeros((16, 1), np.int32), qt, 150))
    finally:
        idx.close()
    for mode in MODES:
        narrow.assert_rows(out[mode][0], rows, 16)
        narrow.assert_reference_i8(out[mode][0], ref)
    check_modes_agree(out)
    assert out[1][1]["bktw_survivors"] > 0


@path_independent
@pytest.mark.parametrize("opts", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("nsp", NSPS)
def test_labels_and_two_partitions_in_one_launch(pyqadc, nsp, opts):
    """The wide suite's labelled launch of two runs: the labels are those of the row-major form at either value of the option."""
    rng = np.random.default_rng(19)
    sizes = [4 * TILE, 4 * TILE + 37]
    parts = [wide.few_wide_keys(rng, s) for s in sizes]
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    tables = float_tables(rng, 2, 2, M)
    parts[1][-1] = narrow.best_code(tables[0, 1])
    parts[0][3 * TILE + 5] = narrow.best_code(tables[0, 0])
    assign = np.array([[0, 1], [1, 0]], np.int32)

    def rows_result():
        idx = wide.make_index(pyqadc, parts, "rows", labels)
        try:
            return idx.query_scan(assign, tables.copy(), wide.R)
        finally:
            idx.close()
    rows = narrow.once(("prune-labels", "rows"), rows_result)
    idx = wide.make_index(pyqadc, parts, nsp, labels, **opts)
    try:
        out = both_modes(idx, lambda ix: ix.query_scan(assign, tables.copy(), wide.R))
    finally:
        idx.close()
    for mode in MODES:
        got, pr = out[mode]
        assert pr["bktw_launches"] == 1 and np.all(got["status"] == 0)
        for q in range(2):
            assert heaps_equal(got["heaps"][q], rows["heaps"][q]), (mode, q)
        assert np.count_nonzero(got["heaps"][0][0] == labels[0][3 * TILE + 5]) == 1
    check_modes_agree(out)


@path_independent
@pytest.mark.parametrize("opts", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("nsp", NSPS)
def test_range_shard_with_an_odd_first_pos_and_key_base(pyqadc, nsp, opts):
    """The wide suite's shard from first_pos = 18 with key_base 1000: keys, values and slots of the ordered streams are those of the
    row-major form of the same shard at either value of the option."""
    rng = np.random.default_rng(47)
    n, first, keep = wide.N12 + 18, 18, 0.01
    codes = wide.few_wide_keys(rng, n, 24)
    tables = float_tables(rng, 2, 1, M)
    codes[-1] = narrow.best_code(tables[0, 0])

    def shard_index(form, **o):
        idx = wide.make_index(pyqadc, None, form, finalize=False, **o)
        idx.add_partition_shard(codes[first:], first, n, starts=codes[:start_size(n, keep)])
        idx.set_key_base(0, 1000)
        idx.finalize(keep)
        idx.set_option("profile", 1)
        return idx

    def streams(ix):
        return ix.query_scan_shard_streams(np.zeros((2, 1), np.int32), tables.copy(), wide.R)

    def rows_result():
        idx = shard_index("rows")
        try:
            return streams(idx)
        finally:
            idx.close()
    b = narrow.once(("prune-shard", "rows"), rows_result)
    idx = shard_index(nsp, **opts)
    try:
        out = both_modes(idx, streams)
    finally:
        idx.close()
    for mode in MODES:
        a, pr = out[mode]
        assert pr["bktw_launches"] == 2, pr
        assert np.all(a["status"] == 0) and np.array_equal(a["offsets"], b["offsets"])
        for q in range(2):
            lo, hi = int(a["offsets"][q]), int(a["offsets"][q + 1])
            sa = np.lexsort((a["vals"][lo:hi], a["keys"][lo:hi], a["slots"][lo:hi]))
            sb = np.lexsort((b["vals"][lo:hi], b["keys"][lo:hi], b["slots"][lo:hi]))
            for k in ("keys", "vals", "slots"):
                assert np.array_equal(a[k][lo:hi][sa], b[k][lo:hi][sb]), (mode, q, k)
            assert a["keys"][lo:hi].min() >= 1000 + first
    check_modes_agree(out)


@path_independent
def test_the_setter_takes_zero_and_one(pyqadc):
    idx = pyqadc.Index(M)
    try:
        idx.set_bkt_prune(1)
        idx.set_bkt_prune(0)
        with pytest.raises(pyqadc.QadcError):
            idx.set_bkt_prune(2)
    finally:
        idx.close()
