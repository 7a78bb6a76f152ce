"""GPU: the id ring of the wide bucket scan's group test ("the tile loop"; scan_bkt_body in
csrc/qadc_kernels.hip).  The PRUNE loop loads the ids of a workgroup's tiles kBktwRing tiles ahead into a ring of registers and
carries the id4 byte raw (its users mask it).  Every case runs with the profile option on (the four counters) and off.  Nothing a
caller sees may change: every case builds ONE index (the survivor counter counts padding slots, tests/test_gpu_bkt_prune.py) and runs
it under bkt_tiles {0, 1} x bkt_prune_lanes {64, 16} x bkt_prune {0, 1}, for every NSP, with int8 tables brought by the caller and a
heap that keeps every candidate.  Heaps are bit for bit those of the row-major form and of the CPU oracle (po.scan_i8; the reference
build's scan as well where it exists); launches, candidates and the survivor counter equal those of the bkt_prune = 0 launch; the
four prune counters are exact from the copy's own ids (tests/bktw_model.py, tools/bucket_prune.py's terms).

The lists are planted, with W forced to one tile (levels as in tests/test_gpu_bktw_scan.py: level 1 = the octaves of 1 and 2 tiles,
level 2 = the rest, both wide launches) and to two tiles (the octaves start at tile 2; level 1 takes the nibble form and the wide form
runs level 2 alone).  A key is (segment number << 4) | n0 and row 0 alone decides how hot a 16-slot group is (tests/test_gpu_bkt_prune.py's
tables: T0 = 0 hot, 123 the edge that is kept, 124 the edge that is pruned, 127 cold), so a cell (tile, wave) of 64 groups is planted
as KEPT (exactly one hot or kept-edge group at a chosen lane, the rest cold) or SKIPPED (all cold, or cold with the pruned edge).
The list ends with 37 codes in a tile of their own: a hot key with n4 = 2, a hot key with n4 = 15 (T4[15] = 127: row 4 alone decides;
pruned for an even NSP, kept for an odd one, where row 4 is fused and counts with its minimum), a cold one, and 0xfffff, whose copies
pad the tile: in that last tile wave 0 is kept and every other wave skipped.  Every other key has n4 = 0 (T4[0] = 3), and with it the
edges decide at id4 = 0 for both parities.

  ring edges: lists of 4 to 12 tiles + 37 (not 8; at 4 tiles the 37 stay in narrow blocks and, W = two tiles, nothing is wide) under 1, 2, 3 and 4 workgroups per run, strided (bkt_tiles 1) and chunked (bkt_tiles 0,
      variant 0x0d): a workgroup gets 0, 1, 2, 3, 4, 5, 7 or 9 tiles, which holds 0, 1, 2, D - 1, D, D + 1 and 2 D + 1 for every ring
      depth D up to 3 (checked against kBktwRing as the source states it); two labelled partitions whose runs of 3 and 5 tiles share
      one launch (float tables), and two planted ones probed in either order
  skip patterns: the 12-tile list under one workgroup per run gives wave w of level 2 (8 planted tiles, then the last one) the
      sequences: w0 skip x 8, keep (the last tile after skips; its candidates leave through the drain); w1 all skipped; w4 keep x 8;
      and for every d in 1..3: w(3 + 2 d) keep, skip x d, keep; w(4 + 2 d) skip x (d + 1), keep; level 1 (3 tiles): w0 none skipped,
      w1 all skipped, w2 keep skip keep, w3 skip skip keep.  Table 1 (all 127) skips everything, table 2 (free rows 0) nothing.
  profile on / off on one index: heaps and candidate streams equal, counters exact when on.

Left out, and why.  A copy whose id4 bytes have non-zero high nibbles: the fill kernel always stores the byte masked
((v >> 16) & 15) and the C-ABI has no call that writes a copy, so a test cannot plant one; the masks at the byte's two users are
covered as far as id4 = 15 goes (a mask that loses a bit turns T4[15] into another entry: counters and heaps).  The guard words
around prune_cnt: the four words are the library's own allocation, never a caller's, and with the profile option off the launch
is given a null pointer, so there is nothing to put a guard around; what a test can see is that the profile's four fields stay 0,
which is checked.

Mutants and what catches them: a slot handed the ids of the wrong tile, the ring's prologue or tail off by one, a tile dropped or
run twice at a workgroup with fewer tiles than the ring is deep -> heaps, survivors and the exact counters at the ring edges and the
patterns; the clamp reading past the workgroup's last tile -> not visible in a result (the ids are not used), which is why the clamp
is argued in the source; id4 unmasked or masked with the wrong constant -> the n4 = 15 keys."""
import os
import re

import numpy as np
import pytest

import bktw_model as wm
import test_gpu_bkt_prune as gp
import test_gpu_bkt_scan as narrow
import test_gpu_bkt_tiles_lanes as tl
import test_gpu_bktw_scan as wide
from dist_cases import start_size
from helpers import float_tables, heaps_equal, path_independent
from test_gpu_bkt_prune import bp
from test_gpu_bktw_scan import planted  # noqa: F401  (float tables: the bound tightens level by level)

pytestmark = pytest.mark.gpu
M, TILE, NSPS, LOOSE = wide.M, wide.TILE, wide.NSPS, wide.LOOSE
WAVE, R_ALL, COMBOS = gp.WAVE, gp.R_ALL, tl.COMBOS
HOT, EDGE_KEEP, EDGE_PRUNE, COLD, COLD2 = gp.HOT, gp.EDGE_KEEP, gp.EDGE_PRUNE, gp.COLD, gp.COLD2
K, S = True, False
LANES = (0, 15, 16, 31, 32, 47, 48, 63)
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quick-adc_amd", "csrc", "qadc_kernels.hip")
RING = int(re.search(r"constexpr uint32_t kBktwRing = (\d+);", open(SRC).read()).group(1))


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def plant(rng, ntiles, cell):
    """A list of ntiles tiles + 37 codes; cell(level, tile of the level, wave) -> K or S."""
    # (8 is left out: its last octave would hold the 37 alone and fall back to narrow blocks beside a wide octave of the same level;
    # at 4 tiles that fallback is the whole of level 2 and the wide form runs level 1 alone)
    assert 4 <= ntiles <= 12 and ntiles != 8
    zero_late = np.zeros(M // 2, np.uint8)                       # every row 5-15 at nibble 0: their minimum
    seg = [-1]

    def next_key(n0, n4=0):
        seg[0] += 1
        while any((seg[0] >> sh) & 15 == 15 for sh in (0, 4, 8)):    # rows 1-3 hold 127 at nibble 15
            seg[0] += 1
        assert seg[0] < 1 << 12
        return (n4 << 16) | (seg[0] << 4) | n0

    def cells(level, t0, t1):
        out = []
        for t in range(t0, t1):
            for w in range(16):
                if cell(level, t, w):
                    lane = LANES[int(rng.integers(len(LANES)))]
                    kind = (HOT, 1) if rng.integers(2) else (EDGE_KEEP, 1, dict(first=zero_late))
                    spec = [(COLD, lane), kind, (COLD2, 63 - lane)]
                elif rng.integers(2):
                    spec = [(COLD, 64)]
                else:
                    spec = [(COLD2, 40), (EDGE_PRUNE, 1, dict(first=zero_late)), (COLD, 23)]
                out += [gp.segment(rng, next_key(n0), groups, **(kw[0] if kw else {})) for n0, groups, *kw in spec if groups]
        return out

    def octave(segments):
        o = np.concatenate(segments)
        return o[rng.permutation(len(o))]

    head = rng.integers(0, 256, (TILE, M // 2), dtype=np.uint8)
    head[:, 0] = (head[:, 0] & 0xf0) | COLD                      # level 0 and the starts: no code below 127
    first = gp.segment(rng, next_key(HOT), 1, first=zero_late)    # the best code (value 3) opens octave 0 whatever its cell says
    o0 = cells(1, 0, 1)
    o0 = [first, o0[0][16:]] + o0[1:]
    parts = [head, octave(o0), octave(cells(1, 1, 3))]
    n2 = ntiles - 4
    tail = [gp.segment(rng, next_key(HOT, 2), 1, codes=10), gp.segment(rng, next_key(HOT, 15), 1, codes=9),
            gp.segment(rng, next_key(COLD, 15), 1, codes=13), gp.segment(rng, 0xfffff, 1, codes=5)]
    if n2 <= 4:
        parts.append(octave(cells(2, 0, n2) + tail))             # (n2 = 0: the 37 alone)
    else:
        parts += [octave(cells(2, 0, 4)), octave(cells(2, 4, n2) + tail)]
    codes = np.ascontiguousarray(np.concatenate(parts))
    assert len(codes) == ntiles * TILE + 37
    return codes


def random_cell(rng):
    m = rng.integers(0, 2, (3, 16, 16)).astype(bool)
    return lambda level, t, w: bool(m[level, t, w])


def pattern_cell(rng):
    """The module docstring's sequences (12 tiles: level 2 has 8 planted tiles); every other cell random."""
    rnd = random_cell(rng)
    l2 = {0: [S] * 8, 1: [S] * 8, 4: [K] * 8}
    for d in (1, 2, 3):
        l2[3 + 2 * d] = ([K] + [S] * d + [K] + [S] * 8)[:8]
        l2[4 + 2 * d] = ([S] * (d + 1) + [K] + [S] * 8)[:8]
    l1 = {0: [K, K, K], 1: [S, S, S], 2: [K, S, K], 3: [S, S, K]}

    def cell(level, t, w):
        table = l1 if level == 1 else l2
        return table[w][t] if w in table else rnd(level, t, w)
    return cell, l1, l2


def keep_matrix(copy, qt, nsp):
    """[wave iteration of the copy][lane]: the groups the kernel must keep, from the copy's own ids."""
    keys = wm.keys_of(copy["codes"][0::16])
    s0, pmin, bsurv = bp.wide_terms(qt, nsp, 127)
    return (s0[keys] + pmin < bsurv).reshape(-1, 64)


def tiles_per_workgroup(ntiles, wgs, chunked):
    if chunked:
        per = (ntiles + wgs - 1) // wgs
        return [max(0, min(ntiles, (b + 1) * per) - b * per) for b in range(wgs)]
    return [len(range(b, ntiles, wgs)) for b in range(wgs)]


def rows_and_oracle(pyqadc, po, key, parts, qt, assign):
    """The row-major form's heaps and the CPU oracle's, computed once per list."""
    def make():
        idx = wide.make_index(pyqadc, parts, "rows", cap=LOOSE)
        try:
            rows = idx.scan_i8(assign, qt, R_ALL)
        finally:
            idx.close()
        nq = len(assign)
        assert all(len(rows[q][1]) < R_ALL for q in range(nq))   # the heap keeps every candidate
        cpu = [po.scan_i8(M, [parts[p] for p in assign[q]], None, qt[q], R_ALL) for q in range(nq)]
        for q in range(nq):
            assert heaps_equal(rows[q], cpu[q]), q
        ref = narrow.reference_i8(po, ("prefetch",) + key, parts, None, qt, tuple(range(nq)), R_ALL) if assign.shape[1] == 1 else None
        return rows, ref
    return narrow.once(("prefetch-rows",) + key, make)


def unprofiled(idx, run):
    """[result] of run(idx) with the profile option off (no counter buffer, no survivor counter), under every combination with the
    group test."""
    out = []
    idx.set_option("profile", 0)
    for tiles, lanes, prune in COMBOS:
        if prune:
            idx.set_bkt_tiles(tiles)
            idx.set_bkt_prune_lanes(lanes)
            idx.set_bkt_prune(prune)
            out.append(run(idx))
    idx.set_option("profile", 1)
    return out


def run_all(pyqadc, parts, nsp, qt, assign, **opts):
    """-> ({combination: (heaps, profile)} with the profile option on, [heaps] with it off, the copies)"""
    idx = wide.make_index(pyqadc, parts, nsp, cap=LOOSE, **opts)
    try:
        copies = [idx.bktw_copy(p) for p in range(len(parts))]
        run = lambda ix: ix.scan_i8(assign, qt, R_ALL)           # noqa: E731
        out = tl.all_combos(idx, run)
        out["unprofiled"] = unprofiled(idx, run)
    finally:
        idx.close()
    return out, copies


def check_all(out, rows, ref, want, nq, launches):
    for got in out.pop("unprofiled"):
        narrow.assert_rows(got, rows, nq)
        narrow.assert_reference_i8(got, ref)
    for combo in COMBOS:
        got, pr = out[combo]
        assert pr["bktw_launches"] == launches if launches else pr["bktw_launches"] > 0, (combo, pr)
        narrow.assert_rows(got, rows, nq)
        narrow.assert_reference_i8(got, ref)
    tl.check_combos_agree(out, want)
    assert [out[c][1]["candidates"] for c in COMBOS] == [out[COMBOS[0]][1]["candidates"]] * len(COMBOS)


# (tiles of the list, workgroups per run): the level-2 run has tiles - 3 tiles (none at 4 tiles: the 37 stay narrow), the level-1 run 3.
# W = two tiles: the octaves start at tile 2, level 1 (tiles 1 to 3) meets the first one half and takes the nibble form, and the wide
# form runs level 2 alone, whose run is the same tiles - 3 tiles; a list of 4 tiles then has no wide launch and is left out.
EDGES = [(4, 1), (4, 3), (4, 4), (5, 1), (5, 3), (6, 4), (7, 1), (7, 3), (9, 4), (10, 1), (10, 3), (12, 1), (12, 2), (12, 4)]
EDGES_W = [(n, w, W) for n, w in EDGES for W in (1, 2) if not (n == 4 and W == 2)]


def wide_runs(ntiles, W):
    """Tiles of the wide runs of a planted list (one run per level that the wide form takes)."""
    return ([3] if W == 1 else []) + ([ntiles - 3] if ntiles > 4 else [])


def test_the_edge_cases_reach_every_tile_count_around_the_ring():
    seen = set()
    for W in (1, 2):
        at_w = set()
        for ntiles, wgs, _ in [e for e in EDGES_W if e[2] == W]:
            for run in wide_runs(ntiles, W):
                for chunked in (False, True):
                    at_w |= set(tiles_per_workgroup(run, wgs, chunked))
        assert {0, 1, 2, RING - 1, RING, RING + 1, 2 * RING + 1} <= at_w and {0, 1, 2, 3, 4, 5, 7, 9} <= at_w, (W, sorted(at_w))
        seen |= at_w
    assert 1 <= RING <= 3
    assert {1, 3, 4} <= {w for _, w in EDGES}


@path_independent
@pytest.mark.parametrize("ntiles,wgs,W", EDGES_W, ids=["%dt-%dwg-W%d" % e for e in EDGES_W])
@pytest.mark.parametrize("nsp", NSPS)
def test_ring_edges(pyqadc, po, nsp, ntiles, wgs, W):
    rng = np.random.default_rng(1500 + ntiles)
    qt = gp.plant_tables(rng)
    codes = narrow.once(("prefetch-list", ntiles), lambda: plant(rng, ntiles, random_cell(rng)))
    assign = np.zeros((3, 1), np.int32)
    rows, ref = rows_and_oracle(pyqadc, po, (ntiles,), [codes], qt, assign)
    out, (copy,) = run_all(pyqadc, [codes], nsp, qt, assign, variant=0x0d, wgs_per_item=wgs, W=W * TILE)
    off = (copy["off"] // TILE).tolist()
    if W == 1:                                                   # the copy: octaves of 1 and 2 tiles (level 1), then level 2's ntiles - 3
        assert off[:3] == [0, 1, 3] and off[-1] == (ntiles if ntiles > 4 else 3), off
    else:                                                        # the copy: the octave of tiles 2 and 3 (not launched), then level 2's
        assert off[:2] == [0, 2] and off[-1] == ntiles - 1, off
    assert off[-1] - off[3 - W] == (ntiles - 3 if ntiles > 4 else 0), off      # level 2's wide run
    want = np.sum([tl.expected_counters(copy, W - 1, qt[q, 0], nsp) for q in range(3)], axis=0)
    check_all(out, rows, ref, want, 3, len(wide_runs(ntiles, W)))
    assert out[(1, 16, 1)][1]["bktw_survivors"] > 0 and want[0] > 0 and want[1] > 0


@path_independent
@pytest.mark.parametrize("wgs", [1, 3, 4])
@pytest.mark.parametrize("nsp", NSPS)
def test_two_planted_partitions_probed_in_either_order(pyqadc, po, nsp, wgs):
    """Two partitions of 5 and 7 tiles + 37 probed by every query, in either order: the levels are cut on the probe sequence, so the
    planner gives the wide form only the runs that start and end on its blocks there (the counters are compared between the
    combinations, not with the copies' totals); the heaps are those of the row-major form and the oracle."""
    rng = np.random.default_rng(1533)
    qt = np.concatenate([gp.plant_tables(rng), gp.plant_tables(rng)], axis=1)
    qt[:, 1] = qt[:, 0]                                          # the plant's keys mean the same in both partitions
    parts = narrow.once(("prefetch-two",), lambda: [plant(rng, 5, random_cell(rng)), plant(rng, 7, random_cell(rng))])
    assign = np.array([[0, 1], [1, 0], [0, 1]], np.int32)
    rows, _ = rows_and_oracle(pyqadc, po, ("two",), parts, qt, assign)
    out, copies = run_all(pyqadc, parts, nsp, qt, assign, variant=0x0d, wgs_per_item=wgs)
    assert [int(c["off"][-1]) // TILE for c in copies] == [5, 7]
    check_all(out, rows, None, None, 3, None)
    assert out[(1, 16, 1)][1]["bktw_slots"] > 0


@pytest.fixture(scope="module")
def patterns(pyqadc, po):
    rng = np.random.default_rng(1515)
    qt = gp.plant_tables(rng)
    cell, l1, l2 = pattern_cell(rng)
    codes = plant(rng, 12, cell)
    rows, ref = rows_and_oracle(pyqadc, po, ("patterns",), [codes], qt, np.zeros((3, 1), np.int32))
    return codes, qt, rows, ref, l1, l2


@path_independent
@pytest.mark.parametrize("opts", [dict(wgs_per_item=1), dict(wgs_per_item=2), dict()], ids=["one-workgroup", "two-workgroups", "default-grid"])
@pytest.mark.parametrize("W", [1, 2], ids=["W1", "W2"])
@pytest.mark.parametrize("nsp", NSPS)
def test_skip_patterns_across_the_ring(pyqadc, patterns, nsp, W, opts):
    codes, qt, rows, ref, l1, l2 = patterns
    assign = np.zeros((3, 1), np.int32)
    out, (copy,) = run_all(pyqadc, [codes], nsp, qt, assign, variant=0x0d, W=W * TILE, **opts)
    # the plant is what the docstring says: wave w of tile t of the copy keeps exactly as its sequence tells, for this NSP's terms.
    # W = two tiles: the copy begins at the list's tile 2 (level 1's second tile) and the wide form runs level 2 alone
    keep = keep_matrix(copy, qt[0, 0], nsp).any(axis=1).reshape(-1, 16)         # [tile of the copy][wave]
    lo = W - 1                                                                  # tiles of the list before the copy's first, less one
    assert len(keep) == 12 - lo
    for w, seq in l1.items():
        assert keep[0:3 - lo, w].tolist() == seq[lo:], (w, keep[0:3 - lo, w])
    for w, seq in l2.items():
        assert keep[3 - lo:11 - lo, w].tolist() == seq, (w, keep[3 - lo:11 - lo, w])
    assert keep[11 - lo].tolist() == [K] + [S] * 15                            # the 37: wave 0 kept after eight skipped tiles
    lanes11 = np.nonzero(keep_matrix(copy, qt[0, 0], nsp)[(11 - lo) * 16])[0].tolist()
    assert lanes11 == ([0, 1] if nsp % 2 else [0]), lanes11                    # n4 = 15: kept only where row 4 is fused (id4 = 15)
    per_table = [tl.expected_counters(copy, lo, qt[q, 0], nsp) for q in range(3)]
    nwaves = (int(copy["off"][-1]) - int(copy["off"][lo])) // WAVE             # of the octaves the wide form launches
    assert per_table[1] == (nwaves, 0, 64 * nwaves, 0) and per_table[2] == (0, nwaves, 0, 0)     # all skipped; none skipped
    check_all(out, rows, ref, np.sum(per_table, axis=0), 3, 3 - W)


@path_independent
@pytest.mark.parametrize("nsp", NSPS)
def test_profile_on_and_off_on_one_index(pyqadc, patterns, nsp):
    codes, qt, rows, ref, _, _ = patterns
    assign = np.zeros((3, 1), np.int32)
    idx = wide.make_index(pyqadc, [codes], nsp, cap=LOOSE, variant=0x0d, wgs_per_item=2)
    try:
        copy = idx.bktw_copy(0)
        want = tuple(np.sum([tl.expected_counters(copy, 0, qt[q, 0], nsp) for q in range(3)], axis=0).tolist())
        seen = {}
        for profile in (1, 0, 1):
            idx.set_option("profile", profile)
            idx.profile_reset()
            heaps = idx.scan_i8(assign, qt, R_ALL)
            pr = idx.profile()
            streams = idx.scan_i8_candidates(assign, qt, R_ALL)
            narrow.assert_rows(heaps, rows, 3)
            narrow.assert_reference_i8(heaps, ref)
            assert tl.counters(pr) == (want if profile else (0, 0, 0, 0)), (profile, tl.counters(pr), want)
            if seen:
                for q in range(3):
                    assert np.array_equal(streams[q][0], seen["streams"][q][0]) and np.array_equal(streams[q][1], seen["streams"][q][1]), (profile, q)
            seen["streams"] = streams
            assert sum(len(s[0]) for s in streams) > 0
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("opts", [dict(variant=0x0d, wgs_per_item=1), dict(variant=0x0d, wgs_per_item=3)], ids=["one-workgroup", "three-workgroups"])
@pytest.mark.parametrize("nsp", NSPS)
def test_float_tables_over_tightening_levels(pyqadc, planted, nsp, opts):  # noqa: F811
    codes, tables, rows, oracle = planted
    idx = wide.make_index(pyqadc, [codes], nsp, cap=wide.CAP, **opts)
    try:
        run = lambda ix: ix.query_scan(np.zeros((3, 1), np.int32), tables.copy(), wide.R)      # noqa: E731
        out = tl.all_combos(idx, run)
        plain = unprofiled(idx, run)
    finally:
        idx.close()
    for got in plain:
        assert np.array_equal(got["status"], rows["status"])
        for q in range(3):
            assert heaps_equal(got["heaps"][q], rows["heaps"][q]), q
    for combo in COMBOS:
        got, pr = out[combo]
        wide.check_profile(pr, nsp)
        assert np.array_equal(got["status"], rows["status"])
        for q in range(3):
            assert heaps_equal(got["heaps"][q], rows["heaps"][q]), (combo, q)
            assert np.array_equal(got["heaps"][q][0], oracle[q]["keys"]) and np.array_equal(got["heaps"][q][1], oracle[q]["values"]), (combo, q)
    tl.check_combos_agree(out)


@path_independent
@pytest.mark.parametrize("wgs", [1, 3, 4])
@pytest.mark.parametrize("nsp", NSPS)
def test_labels_and_two_runs_of_different_tile_counts_in_one_launch(pyqadc, nsp, wgs):
    """tests/test_gpu_bkt_tiles_lanes.py's two labelled partitions, whose level-1 runs have 3 and 5 tiles in ONE launch: under 4
    workgroups per run the shorter run's last workgroup has no tile and the others one each (fewer than the ring is deep), the longer
    run's get 2, 1, 1, 1 strided and 2, 2, 1, 0 in chunks; under 3: 1, 1, 1 and 2, 2, 1; under 1: 3 and 5."""
    rng = np.random.default_rng(1523)
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
    rows = narrow.once(("prefetch-labels", "rows"), rows_result)
    idx = wide.make_index(pyqadc, parts, nsp, labels, variant=0x0d, wgs_per_item=wgs)
    try:
        tiles = [int(idx.bktw_copy(p)["off"][-1]) // TILE for p in range(2)]
        run = lambda ix: ix.query_scan(assign, tables.copy(), wide.R)       # noqa: E731
        out = tl.all_combos(idx, run)
        plain = unprofiled(idx, run)
    finally:
        idx.close()
    assert tiles == [3, 5], tiles
    for got in plain:
        for q in range(2):
            assert np.all(got["status"] == 0) and heaps_equal(got["heaps"][q], rows["heaps"][q]), q
    for combo in COMBOS:
        got, pr = out[combo]
        assert pr["bktw_launches"] == 1 and np.all(got["status"] == 0), pr
        for q in range(2):
            assert heaps_equal(got["heaps"][q], rows["heaps"][q]), (combo, q)
    tl.check_combos_agree(out)


@path_independent
@pytest.mark.parametrize("wgs", [1, 3])
@pytest.mark.parametrize("nsp", NSPS)
def test_range_shard_whose_first_pos_is_2_mod_16_with_a_key_base(pyqadc, nsp, wgs):
    rng = np.random.default_rng(1553)
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
    b = narrow.once(("prefetch-shard", "rows"), rows_result)
    idx = shard_index(nsp, variant=0x0d, wgs_per_item=wgs)
    try:
        out = tl.all_combos(idx, streams)
        plain = unprofiled(idx, streams)
    finally:
        idx.close()
    assert first % 16 == 2
    for combo, (a, pr) in list(out.items()) + [(None, (a, None)) for a in plain]:
        assert pr is None or pr["bktw_launches"] == 2, pr
        assert np.all(a["status"] == 0) and np.array_equal(a["offsets"], b["offsets"])
        for q in range(2):
            lo, hi = int(a["offsets"][q]), int(a["offsets"][q + 1])
            sa = np.lexsort((a["vals"][lo:hi], a["keys"][lo:hi], a["slots"][lo:hi]))
            sb = np.lexsort((b["vals"][lo:hi], b["keys"][lo:hi], b["slots"][lo:hi]))
            for k in ("keys", "vals", "slots"):
                assert np.array_equal(a[k][lo:hi][sa], b[k][lo:hi][sb]), (combo, q, k)
            assert a["keys"][lo:hi].min() >= 1000 + first
    tl.check_combos_agree(out)
