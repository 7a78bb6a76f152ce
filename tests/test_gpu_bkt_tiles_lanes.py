"""GPU: the bucket launches' tile order (qadc_index_set_bkt_tiles) and the group test's load granularity
(qadc_index_set_bkt_prune_lanes; DESIGN.md section 3.1, "pruned groups").  bkt_tiles = 1 makes the bucket launches walk strided
tiles whatever variant bit 3 says; bkt_prune_lanes = 16 makes a wave iteration that runs load its planes by aligned 16-lane
quarters: a quarter none of whose lane groups keeps loads nothing and goes through the pair loop with index 0.  Nothing a caller
sees may change.  Every case builds ONE index (the survivor counter counts padding slots, whose codes differ from one finalize to
the next; tests/test_gpu_bkt_prune.py) and runs it under every combination of bkt_tiles {0, 1} x bkt_prune_lanes {64, 16} x
bkt_prune {0, 1}: heaps bit for bit those of the row-major form and of the reference, launch counters, candidates and survivors
equal across all eight, the group test's counters exact.  The chunked loop is asked for explicitly (variant 0x0d, bkt_tiles 0):
under the default tile order variant 0x0d alone no longer reaches it.

The quarter plant (7 tiles + 37, W = one tile; keys and tables as in tests/test_gpu_bkt_prune.py: row 0 alone decides how hot a
group is): level 1 = octaves of 1 and 2 tiles (under wgs_per_item = 3 a chunk of one tile each), level 2 = an octave of 3 tiles +
37 (4 tiles: chunks of 2, 2 and none; under wgs_per_item = 1 one workgroup per run).
  octave 0 (1 tile): the best code's group in wave 0, the rest cold
  octave 1 (2 tiles), tile 0: waves 0-7 in which exactly one lane keeps, at 0, 15, 16, 31, 32, 47, 48, 63; waves 8-11 in which
      exactly quarter 0, 1, 2, 3 keeps whole; wave 12: quarters 0 and 2, wave 13: quarters 1 and 3; wave 14: one lane in each of
      the four; wave 15 cold; tile 1: both edge groups (T0 = 123 kept, 124 pruned), each with the code whose other rows are at
      their minimum, the rest cold
  octave 2 (3 tiles + 37): tile 0 cold; tile 1: its first quarter keeps (right after a skipped tile) and its last quarter keeps
      (right before one); tile 2 cold; the 37 in a fourth tile: the copy's last kept groups (a hot bucket with padding slots), a
      cold bucket with padding slots, then key 0xfffff

Mutants and what catches them: the quarter mask shifted by the wrong lane bits, or 15 / 17 lanes wide -> the single-lane waves
(heaps: the lane's candidates are lost; or the exact fourth counter); stale plane registers in an idle quarter in place of index 0
-> nothing a caller sees, by the exactness argument, which is why the counters are compared; counting idle quarters of skipped
waves -> the fourth counter; a chunk's first / last off by one or a workgroup without tiles reading one -> heaps and survivors."""
import itertools

import numpy as np
import pytest

import bktw_model as wm
import test_gpu_bkt_prune as gp
import test_gpu_bkt_scan as narrow
import test_gpu_bktw_scan as wide
from dist_cases import start_size
from helpers import float_tables, heaps_equal, path_independent
from test_gpu_bkt_prune import bp
from test_gpu_bktw_scan import planted  # noqa: F401  (float tables: the bound tightens level by level)

pytestmark = pytest.mark.gpu
M, TILE, NSPS, LOOSE = wide.M, wide.TILE, wide.NSPS, wide.LOOSE
WAVE = gp.WAVE
R_ALL = gp.R_ALL
HOT, EDGE_KEEP, EDGE_PRUNE, COLD, COLD2 = gp.HOT, gp.EDGE_KEEP, gp.EDGE_PRUNE, gp.COLD, gp.COLD2
COMBOS = list(itertools.product((0, 1), (64, 16), (0, 1)))      # (bkt_tiles, bkt_prune_lanes, bkt_prune)
LOOPS = [dict(variant=0x0d), dict(variant=0x01), dict(variant=0x0d, wgs_per_item=1), dict(variant=0x0d, wgs_per_item=3),
         dict(variant=0x01, wgs_per_item=3)]
LOOP_IDS = ["chunked", "grid-stride", "one-workgroup", "chunks-of-2-2-0", "stride-3"]
N7 = 7 * TILE + 37
SINGLE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def quarter_codes(rng):
    zero_late = np.zeros(M // 2, np.uint8)                       # every row 5-15 at nibble 0: their minimum
    seg = [-1]

    def next_key(n0):
        seg[0] += 1
        while any((seg[0] >> sh) & 15 == 15 for sh in (0, 4, 8)):    # rows 1-3 hold 127 at nibble 15
            seg[0] += 1
        assert seg[0] < 1 << 12
        return (seg[0] << 4) | n0

    def fill(spec, slots):
        out = [gp.segment(rng, next_key(n0), groups, **(kw[0] if kw else {})) for n0, groups, *kw in spec if groups]
        used = sum(len(o) for o in out)
        assert used <= slots
        while used < slots:                                      # cold to the octave's end, in buckets of at most 300 groups
            g = min(300, (slots - used + 15) // 16)
            out.append(gp.segment(rng, next_key(COLD if len(out) % 2 else COLD2), g, codes=min(16 * g, slots - used)))
            used += len(out[-1])
        out = np.concatenate(out)
        return out[rng.permutation(len(out))]

    head = rng.integers(0, 256, (TILE, M // 2), dtype=np.uint8)
    head[:, 0] = (head[:, 0] & 0xf0) | COLD                      # level 0 and the starts: no code below 127
    o0 = fill([(HOT, 1, dict(first=zero_late))], TILE)
    spec = []
    for lane in SINGLE_LANES:                                    # waves 0-7
        spec += [(COLD, lane), (HOT, 1), (COLD2, 63 - lane)]
    for q in range(4):                                           # waves 8-11
        spec += [(COLD, 16 * q), (HOT, 16), (COLD2, 48 - 16 * q)]
    spec += [(HOT, 16), (COLD, 16), (HOT, 1), (COLD2, 31)]       # wave 12: quarters 0 and 2
    spec += [(COLD, 16), (HOT, 1), (COLD2, 31), (HOT, 16)]       # wave 13: quarters 1 and 3
    spec += [(HOT, 1), (COLD, 15)] * 4                           # wave 14: all four
    spec += [(COLD, 64)]                                         # wave 15
    spec += [(COLD, 70), (EDGE_KEEP, 1, dict(first=zero_late)), (COLD2, 20), (EDGE_PRUNE, 1, dict(first=zero_late))]   # tile 1
    o1 = fill(spec, 2 * TILE)
    o2 = fill([(COLD, 300), (COLD2, 300), (COLD, 300), (COLD2, 124),                 # tile 0
               (HOT, 16), (COLD, 300), (COLD2, 300), (COLD, 300), (COLD2, 92), (HOT, 16),     # tile 1
               (COLD, 300), (COLD2, 300), (COLD, 300), (COLD2, 124)],                # tile 2
              3 * TILE)
    # the 37: n4 = 2 (T4 = 3), hot: the copy's last kept groups, 19 codes in two groups; a cold bucket of 13; 0xfffff (127 in every
    # free row) ends the octave, so the tile's remainder is cold
    tail = [gp.segment(rng, (2 << 16) | HOT, 2, codes=19), gp.segment(rng, (3 << 16) | COLD, 1, codes=13), gp.segment(rng, 0xfffff, 1, codes=5)]
    codes = np.ascontiguousarray(np.concatenate([head, o0, o1, o2] + tail))
    assert len(codes) == N7
    return codes


def expected_counters(copy, first_octave, qt, nsp, bound=127):
    """(skipped, run, groups, idle quarters of run wave iterations) of one query's wide launches, from the copy's own ids."""
    lo = int(copy["off"][first_octave]) // 16
    keys = wm.keys_of(copy["codes"][0::16])[lo:]
    s0, pmin, bsurv = bp.wide_terms(qt, nsp, bound)
    keep = (s0[keys] + pmin < bsurv).reshape(-1, 4, 16)
    q = keep.any(axis=2)
    run = q.any(axis=1)
    return int((~run).sum()), int(run.sum()), int((~keep).sum()), int((~q[run]).sum())


def all_combos(idx, run):
    """{(tiles, lanes, prune): (result, profile)} of run(idx) on ONE index."""
    out = {}
    for tiles, lanes, prune in COMBOS:
        idx.set_bkt_tiles(tiles)
        idx.set_bkt_prune_lanes(lanes)
        idx.set_bkt_prune(prune)
        idx.profile_reset()
        res = run(idx)
        out[(tiles, lanes, prune)] = (res, idx.profile())
    return out


def counters(pr):
    return (pr["bktw_prune_skipped"], pr["bktw_prune_run"], pr["bktw_prune_groups"], pr["bktw_prune_quarters"])


def check_combos_agree(out, want=None):
    """No option changes the launches, the candidates or the survivors; without the test every counter is 0; with it the first
    three are the same at either granularity (want: their exact values) and the fourth counts only with 16 lanes."""
    base = out[COMBOS[0]][1]
    for (tiles, lanes, prune), (_, pr) in out.items():
        assert [pr[k] for k in gp.LAUNCH_KEYS] == [base[k] for k in gp.LAUNCH_KEYS], ((tiles, lanes, prune), pr, base)
        assert pr["bktw_survivors"] == base["bktw_survivors"], ((tiles, lanes, prune), pr["bktw_survivors"], base["bktw_survivors"])
        got = counters(pr)
        if not prune:
            assert got == (0, 0, 0, 0), ((tiles, lanes, prune), got)
            continue
        assert got[0] + got[1] == pr["bktw_slots"] // WAVE > 0, pr
        assert got[0] * 64 <= got[2] <= pr["bktw_slots"] // 16, pr
        assert got[:3] == counters(out[(0, 64, 1)][1])[:3], ((tiles, lanes, prune), got)
        if lanes == 64:
            assert got[3] == 0, got
        else:
            assert got[3] <= 3 * got[1] and 16 * got[3] + 64 * got[0] <= got[2], got      # a wave that runs has a quarter that loads
            assert got[3] == out[(0, 16, 1)][1]["bktw_prune_quarters"], ((tiles, lanes, prune), got)
        if want is not None:
            assert got == (tuple(want) if lanes == 16 else tuple(want[:3]) + (0,)), ((tiles, lanes, prune), got, want)


@pytest.fixture(scope="module")
def quarters(pyqadc, po):
    rng = np.random.default_rng(1414)
    qt = gp.plant_tables(rng)
    codes = quarter_codes(rng)
    idx = wide.make_index(pyqadc, [codes], "rows", cap=LOOSE)
    try:
        rows = idx.scan_i8(np.zeros((3, 1), np.int32), qt, R_ALL)
    finally:
        idx.close()
    ref = narrow.reference_i8(po, ("quarter-plant",), [codes], None, qt, (0, 1, 2), R_ALL)
    below = [int(np.count_nonzero(rows[q][1] < 127)) for q in range(3)]
    assert all(len(rows[q][1]) < R_ALL for q in range(3)) and below[1] == 0 and below[2] > 0, below      # the heap keeps every candidate
    assert rows[0][1].min() == 3 and np.count_nonzero(rows[0][1] == 126) >= 1 and 1000 < below[0] < R_ALL, below
    return codes, qt, rows, ref


@path_independent
@pytest.mark.parametrize("opts", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("nsp", NSPS)
def test_planted_quarters_counters_exact_and_heaps_unchanged(pyqadc, quarters, nsp, opts):
    codes, qt, rows, ref = quarters
    idx = wide.make_index(pyqadc, [codes], nsp, cap=LOOSE, **opts)
    try:
        copy = idx.bktw_copy(0)
        out = all_combos(idx, lambda ix: ix.scan_i8(np.zeros((3, 1), np.int32), qt, R_ALL))
    finally:
        idx.close()
    per_table = [expected_counters(copy, 0, qt[q, 0], nsp) for q in range(3)]
    nwaves = int(copy["off"][-1]) // WAVE
    assert per_table[1] == (nwaves, 0, 64 * nwaves, 0)                      # all 127: bsurv = 0, every wave iteration skipped
    assert per_table[2] == (0, nwaves, 0, 0)                                # free rows of 0: nothing pruned
    assert per_table[0][3] > 0
    want = np.sum(per_table, axis=0)
    for combo in COMBOS:
        got, pr = out[combo]
        wide.check_profile(pr, nsp)
        assert pr["bktw_launches"] == 2, pr
        narrow.assert_rows(got, rows, 3)
        narrow.assert_reference_i8(got, ref)
    check_combos_agree(out, want)
    assert out[(1, 16, 1)][1]["bktw_survivors"] > 0


@path_independent
@pytest.mark.parametrize("nsp", NSPS)
def test_the_quarter_plant_is_what_the_docstring_says(pyqadc, quarters, nsp):
    codes, qt, _, _ = quarters
    idx = wide.make_index(pyqadc, [codes], nsp, cap=LOOSE)
    try:
        copy = idx.bktw_copy(0)
    finally:
        idx.close()
    keys = wm.keys_of(copy["codes"][0::16])
    s0, pmin, bsurv = bp.wide_terms(qt[0, 0], nsp, 127)
    assert (pmin, bsurv) == (3 if nsp % 2 else 0, 127)
    keep = (s0[keys] + pmin < bsurv).reshape(-1, 64)
    off = (copy["off"] // WAVE).astype(int)
    assert off.tolist() == [0, 16, 48, 112]                                # octaves of 1, 2 and 4 tiles
    lanes = [np.nonzero(w)[0].tolist() for w in keep]
    assert lanes[0] == [0] and not keep[1:16].any()
    o1 = lanes[off[1]:off[2]]
    assert o1[:8] == [[l] for l in SINGLE_LANES]
    assert o1[8:12] == [list(range(16 * q, 16 * q + 16)) for q in range(4)]
    assert o1[12] == list(range(16)) + [32] and o1[13] == [16] + list(range(48, 64))
    assert o1[14] == [0, 16, 32, 48] and not o1[15] and keep[off[1] + 16:off[2]].sum() == 1       # tile 1: the kept edge alone
    o2 = lanes[off[2]:]
    assert not any(o2[:16]) and o2[16] == list(range(16)) and not any(o2[17:31]) and o2[31] == list(range(48, 64))
    assert not any(o2[32:48])                                              # tile 2: skipped whole
    assert o2[48] == [0, 1] and not keep[-15:].any()                       # the last tile: the hot bucket's two groups, then cold
    pad = copy["perm"].reshape(-1, 16) == wm.PAD
    assert pad[keep.reshape(-1)].any() and pad[~keep.reshape(-1)].any()


@path_independent
@pytest.mark.parametrize("opts", LOOPS[:3], ids=LOOP_IDS[:3])
@pytest.mark.parametrize("nsp", NSPS)
def test_the_prune_suites_plant_under_every_combination(pyqadc, po, nsp, opts):
    """tests/test_gpu_bkt_prune.py's list (lanes 0, 63, 31, 32; a key that row 4 alone decides; key 0xfffff) with the fourth counter."""
    rng = np.random.default_rng(1313)
    qt = gp.plant_tables(rng)
    codes = gp.plant_codes(rng)
    rows = narrow.once(("tiles-lanes-plant", "rows"), lambda: gp.scan_i8(pyqadc, codes, "rows", qt)[0][0][0])
    ref = narrow.reference_i8(po, ("tiles-lanes-plant",), [codes], None, qt, (0, 1, 2), R_ALL)
    idx = wide.make_index(pyqadc, [codes], nsp, cap=LOOSE, **opts)
    try:
        copy = idx.bktw_copy(0)
        out = all_combos(idx, lambda ix: ix.scan_i8(np.zeros((3, 1), np.int32), qt, R_ALL))
    finally:
        idx.close()
    want = np.sum([expected_counters(copy, 0, qt[q, 0], nsp) for q in range(3)], axis=0)
    assert tuple(want[:3]) == tuple(np.sum([gp.expected_counters(copy, 0, qt[q, 0], nsp) for q in range(3)], axis=0))
    for combo in COMBOS:
        narrow.assert_rows(out[combo][0], rows, 3)
        narrow.assert_reference_i8(out[combo][0], ref)
    check_combos_agree(out, want)


@path_independent
@pytest.mark.parametrize("opts", LOOPS[:3], ids=LOOP_IDS[:3])
@pytest.mark.parametrize("nsp", NSPS)
def test_float_tables_over_tightening_levels(pyqadc, planted, nsp, opts):  # noqa: F811
    codes, tables, rows, oracle = planted
    idx = wide.make_index(pyqadc, [codes], nsp, cap=wide.CAP, **opts)
    try:
        out = all_combos(idx, lambda ix: ix.query_scan(np.zeros((3, 1), np.int32), tables.copy(), wide.R))
    finally:
        idx.close()
    for combo in COMBOS:
        got, pr = out[combo]
        wide.check_profile(pr, nsp)
        assert np.array_equal(got["status"], rows["status"])
        for q in range(3):
            assert heaps_equal(got["heaps"][q], rows["heaps"][q]), (combo, q)
            assert np.array_equal(got["heaps"][q][0], oracle[q]["keys"]) and np.array_equal(got["heaps"][q][1], oracle[q]["values"]), (combo, q)
    check_combos_agree(out)
    assert out[(1, 16, 1)][1]["bktw_survivors"] > 0


@path_independent
@pytest.mark.parametrize("opts", [dict(variant=0x0d, wgs_per_item=4), dict(variant=0x01, wgs_per_item=4), dict(variant=0x0d)],
                         ids=["chunks-4", "stride-4", "chunked"])
@pytest.mark.parametrize("nsp", NSPS)
def test_labels_and_two_runs_of_different_tile_counts_in_one_launch(pyqadc, nsp, opts):
    """Two labelled partitions whose level-1 runs have 3 and 5 tiles (the first one's buckets are multiples of 16 codes; in the
    second an octave's padding takes one tile more): with four workgroups per run the shorter run's last workgroup gets no tile
    (first >= last under chunks, blockIdx.x >= ntiles under strides) and the longer run's chunks are 2, 2, 1 and none."""
    rng = np.random.default_rng(23)
    sizes = [4 * TILE, 4 * TILE + 37]
    parts = [wide.few_wide_keys(rng, s) for s in sizes]
    keys16 = rng.permutation(1 << 20)[:16]
    wide.set_key(parts[0][TILE:2 * TILE], rng.permutation(np.repeat(keys16, TILE // 16)))
    wide.set_key(parts[0][2 * TILE:], rng.permutation(np.repeat(keys16, TILE // 8)))
    labels = [rng.integers(0, 1 << 30, s, dtype=np.uint32) for s in sizes]
    tables = float_tables(rng, 2, 2, M)
    parts[1][-1] = narrow.best_code(tables[0, 1])
    assign = np.array([[0, 1], [1, 0]], np.int32)

    def rows_result():
        idx = wide.make_index(pyqadc, parts, "rows", labels)
        try:
            return idx.query_scan(assign, tables.copy(), wide.R)
        finally:
            idx.close()
    rows = narrow.once(("tiles-lanes-labels", "rows"), rows_result)
    idx = wide.make_index(pyqadc, parts, nsp, labels, **opts)
    try:
        tiles = [int(idx.bktw_copy(p)["off"][-1]) // TILE for p in range(2)]
        out = all_combos(idx, lambda ix: ix.query_scan(assign, tables.copy(), wide.R))
    finally:
        idx.close()
    assert tiles == [3, 5], tiles
    for combo in COMBOS:
        got, pr = out[combo]
        assert pr["bktw_launches"] == 1 and np.all(got["status"] == 0), pr
        for q in range(2):
            assert heaps_equal(got["heaps"][q], rows["heaps"][q]), (combo, q)
    check_combos_agree(out)


@path_independent
@pytest.mark.parametrize("opts", LOOPS[:3], ids=LOOP_IDS[:3])
@pytest.mark.parametrize("nsp", NSPS)
def test_range_shard_with_an_odd_first_pos_and_key_base(pyqadc, nsp, opts):
    rng = np.random.default_rng(53)
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
    b = narrow.once(("tiles-lanes-shard", "rows"), rows_result)
    idx = shard_index(nsp, **opts)
    try:
        out = all_combos(idx, streams)
    finally:
        idx.close()
    for combo in COMBOS:
        a, pr = out[combo]
        assert pr["bktw_launches"] == 2, pr
        assert np.all(a["status"] == 0) and np.array_equal(a["offsets"], b["offsets"])
        for q in range(2):
            lo, hi = int(a["offsets"][q]), int(a["offsets"][q + 1])
            sa = np.lexsort((a["vals"][lo:hi], a["keys"][lo:hi], a["slots"][lo:hi]))
            sb = np.lexsort((b["vals"][lo:hi], b["keys"][lo:hi], b["slots"][lo:hi]))
            for k in ("keys", "vals", "slots"):
                assert np.array_equal(a[k][lo:hi][sa], b[k][lo:hi][sb]), (combo, q, k)
            assert a["keys"][lo:hi].min() >= 1000 + first
    check_combos_agree(out)


@path_independent
def test_the_setters_refuse_other_values(pyqadc):
    idx = pyqadc.Index(M)
    try:
        for ok in (0, 1):
            idx.set_bkt_tiles(ok)
        for ok in (64, 16):
            idx.set_bkt_prune_lanes(ok)
        for bad in (-1, 2, 8):
            with pytest.raises(pyqadc.QadcError):
                idx.set_bkt_tiles(bad)
        for bad in (0, 1, 8, 32, 48, 128):
            with pytest.raises(pyqadc.QadcError):
                idx.set_bkt_prune_lanes(bad)
        idx.set_bkt_prune(1)
        idx.set_bkt_prune(0)
        with pytest.raises(pyqadc.QadcError):
            idx.set_bkt_prune(2)
    finally:
        idx.close()
