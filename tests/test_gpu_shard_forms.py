"""GPU: range shards of a partition scanned in every form of the 16x4 level scan (DESIGN.md sections 3.1 and 5): row-major, the
7-, 6- and 5-plane byte copy, the nibble form (8, 9, 10 planes) and the bucket form (NSP 4 to 7, blocks of one and of two tiles),
on virtual ranks: one Index per rank on one GPU, Index.query_scan_shard_streams, pyqadc.replay_i8 and pyqadc.dist_merge_blocks
(device and host), as tests/test_gpu_parity.py::test_dist_merge_kernel_on_virtual_ranks.  Every comparison is an equality, array
for array, with the UNSHARDED CPU oracle (po.query_scan; the reference build's scan where it is there).

What a shard changes: keys are key_base + first_pos + local position (the bucket form: the position from the copy's perm), only
the last shard replays the partition's last code in the padding lanes and it does so (16 - global_n % 16) % 16 times, the
pre-scan reads the starts replica, a rank may hold nothing or less than a tile, the copies are built from the local codes (whose
first one may sit anywhere in the partition), and the ranks' streams must replay, in (assign slot, rank, position) order, to the
unsharded heap.

The flat list (dist_cases.shard_forms_list; tests/test_shard_forms_inputs_host.py pins it on a CPU): 12 tiles + 37 codes, 1024
distinct keys.  Query 0's best code is the partition's last code (in the heap with its 11 replays) and, for every cut set, rank
0's last local code (a shard that does not end the partition must emit it once) and rank 1's first (key == first_pos).  The cut
sets (dist_cases.shard_forms_cuts): on a tile; pyqadc.sharded.shard_ranges(n, 2) (first_pos 98 320: a multiple of 16, not of the
tile); three ranks cut at 4 tiles + 16 and 8 tiles + 48; four ranks of 12 tiles, 32 codes, 5 codes (the ragged end and dup_pos)
and none (the starts replica only); and first_pos = 6 tiles + 18, which is 2 mod 16 (any even position keeps a 16x4 shard
16-byte aligned): there alone the last shard's local size and the partition's differ mod 16, so the replay count shows where it
is taken from, and rank 0 ends on a code that is no multiple of 16 from its start without replaying it.

Levels: TINY (level_base = one tile): [0, 16 Ki), [16 Ki, 64 Ki), [64 Ki, 256 Ki) of the rank's LOCAL scan order, so every run
starts on a tile of the rank's copies and the whole shard is scanned in the form (split_codes == scan_codes).  Blocks of two
tiles: level_base = two tiles (as test_gpu_bkt_scan's two-tile lists), so that every cut falls on a block and every rank of two
tiles has bucket launches; the same blocks under one-tile levels are the form "bkt5/2-tiles/mixed": there the levels [0, 16 Ki)
and [16 Ki, 64 Ki) miss the blocks and take the nibble form from a nibble copy that nib_still_needed must grant a sharded lone
partition, and only [64 Ki, ...) is a bucket launch (ranks above four tiles).

A rank below one tile that holds codes: the thresholds here are 1, so it gets its (one-tile) copies and scans its few codes in
the form like any other rank; only the rank that holds no code has no copy and no launch.

Every test sets wgq = 0 and head_level = 0 itself, so the scan path conftest.py would select makes no difference: each runs once."""
from collections import namedtuple

import numpy as np
import pytest

import bkt_model
from dist_cases import shard_forms_cuts, shard_forms_list, shard_ranges, start_size
from helpers import float_tables, heaps_equal, path_independent, rand_codes
from test_gpu_bkt_scan import ONE_QUERY_PER_PASS, TILE, TINY, best_code

pytestmark = pytest.mark.gpu
M = 16
R = 100
KEEPS = (0.01, 0.05)
CAPACITY = 1 << 18                                               # Index.query_scan_shard_streams' default

Form = namedtuple("Form", "kind arg block level_base")
ROWS = Form("rows", 0, TILE, TILE)
PLANES = [Form("planes", p, TILE, TILE) for p in (7, 6, 5)]
NIBS = [Form("nib", ns, TILE, TILE) for ns in (8, 9, 10)]
BKTS = [Form("bkt", nsp, t * TILE, t * TILE) for t in (1, 2) for nsp in (4, 5, 6, 7)]
MIXED = Form("bkt", 5, 2 * TILE, TILE)
FLAT_FORMS = [ROWS] + PLANES + NIBS + BKTS + [MIXED]
IVF_FORMS = [ROWS, PLANES[0], PLANES[2], NIBS[1], BKTS[0], BKTS[3]]
PER_FORM = ("bkt_launches", "nib_launches", "nib8_launches", "split5_launches", "split6_launches")


def form_id(f):
    if f.kind == "rows":
        return "rows"
    if f.kind != "bkt":
        return "%s%d" % (f.kind, f.arg)
    return "bkt%d/%d-tile%s%s" % (f.arg, f.block // TILE, "s" if f.block > TILE else "", "/mixed" if f.level_base != f.block else "")


def counter_of(f):
    """The profile's launch counter of the form (7 planes have none of their own: split_launches, with every other one 0)."""
    return {"planes": {7: "split_launches", 6: "split6_launches", 5: "split5_launches"}.get(f.arg),
            "nib": "nib8_launches" if f.arg == 8 else "nib_launches", "bkt": "bkt_launches"}[f.kind]


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


Shard = namedtuple("Shard", "codes first global_n labels starts")


def make_rank(pyqadc, form, shards, keep, key_base=None):
    """One rank's Index: the options and every set_split* call first, then the rank's shards (an empty partition: global_n 0),
    then finalize.  form.kind "rows": no copy; "planes": the byte copy alone (7) with the 6- and 5-plane thresholds at 1;
    "nib": 8 (the 8-plane threshold at 1) or 9 / 10 (ns); "bkt": NSP, as test_gpu_bkt_scan.make_index (runs the blocks do not
    fit: 9 nibble planes)."""
    idx = pyqadc.Index(M)
    for k, v in dict(ONE_QUERY_PER_PASS, **dict(TINY, level_base=form.level_base)).items():
        idx.set_option(k, v)
    rows, planes = form.kind == "rows", form.arg if form.kind == "planes" else 0
    idx.set_split(0 if rows else 1, 1)
    idx.set_split6(0 if rows or planes == 7 else 1)
    idx.set_split5(0 if rows or planes in (7, 6) else 1)
    if form.kind == "nib":
        idx.set_split_nib(0 if form.arg == 8 else 1, 1 if form.arg == 8 else 0, 10 if form.arg == 10 else 9)
    elif form.kind == "bkt":
        idx.set_split_nib(1, 0, 9)
        idx.set_split_bkt(1, form.block, int(form.arg == 6), int(form.arg == 5), int(form.arg == 4), 1e6)
    else:
        idx.set_split_nib(0, 0, 9)
        idx.set_split_bkt(0)
    for s in shards:
        if s.global_n == 0:
            idx.add_partitions([np.zeros((0, M // 2), np.uint8)], None if s.labels is None else [np.zeros(0, np.uint32)])
        else:
            idx.add_partition_shard(s.codes, s.first, s.global_n, labels=s.labels if len(s.codes) else None, starts=s.starts)
    if key_base is not None:
        idx.set_key_base(0, key_base)
    idx.finalize(keep)
    idx.set_option("profile", 1)
    return idx


def rank_streams(pyqadc, form, shards, keep, assign, tables, key_base=None):
    """-> (the rank's streams of one batch, its profile)"""
    idx = make_rank(pyqadc, form, shards, keep, key_base)
    try:
        out = idx.query_scan_shard_streams(assign, tables.copy(), R, capacity=CAPACITY)
        return out, idx.profile()
    finally:
        idx.close()


def stream_of(out, q):
    a, b = int(out["offsets"][q]), int(out["offsets"][q + 1])
    return out["keys"][a:b], out["vals"][a:b], out["slots"][a:b]


def check_streams(out, nq):
    """status 0 everywhere, and the streams fit the buffer they were collected into"""
    assert np.all(out["status"][:nq] == 0), out["status"]
    assert int(out["offsets"][nq]) < CAPACITY, out["offsets"]


def copy_tiles(n):
    return (n + TILE - 1) // TILE


def check_flat_profile(pr, form, ln):
    """One unlabelled partition of ln local codes: which launches ran and which copies finalize made."""
    split_counters = ("split_launches", "split_codes") + PER_FORM
    if form.kind == "rows" or ln == 0:
        assert all(pr[k] == 0 for k in split_counters), pr
        assert pr["split_copy_bytes"] == pr["bkt_copy_bytes"] == pr["nib_copy_bytes"] == 0, pr
        return
    assert pr["split_copy_failed"] == pr["nib_copy_failed"] == pr["bkt_copy_failed"] == pr["bkt_copy_padded_out"] == 0, pr
    # every run starts on a tile of the rank's local order: nothing is scanned row-major
    assert pr["split_launches"] == pr["scan_launches"] > 0 and pr["split_codes"] == pr["scan_codes"] > 0, pr
    assert pr["split_copy_bytes"] == copy_tiles(ln) * 7 * TILE, pr
    own = sum(pr[k] for k in PER_FORM)
    if form.kind == "planes" and form.arg == 7:
        assert own == 0, pr
    else:
        assert own == pr["split_launches"], pr
    mixed = form.kind == "bkt" and form.level_base != form.block
    if not mixed:
        assert pr[counter_of(form)] == pr["split_launches"], pr           # (a rank of two tiles and more, and the smaller ones too)
    if form.kind == "bkt":
        assert pr["bkt%d_launches" % form.arg] == pr["bkt_launches"] and pr["bkt_copy_bytes"] > 0 and pr["bkt_codes"] <= pr["bkt_slots"], pr
        if mixed:
            # blocks of two tiles under levels [0, T), [T, 4 T), [4 T, ...): a lone run [0, ln) ends the partition (bucket); else
            # the first two levels miss the blocks (nibble form, from the copy nib_still_needed grants) and the third is on them
            assert (pr["bkt_launches"] > 0) == (ln <= TILE or ln > 4 * TILE), pr
            assert (pr["nib_launches"] > 0) == (ln > TILE) and pr["nib_copy_bytes"] == (copy_tiles(ln) * 8 * TILE if ln > TILE else 0), pr
        else:
            assert pr["nib_copy_bytes"] == 0, pr                          # every cut on a block: the nibble copy would never be read
    else:
        assert pr["bkt_copy_bytes"] == 0 and pr["nib_copy_bytes"] == (copy_tiles(ln) * 8 * TILE if form.kind == "nib" else 0), pr


# ---- a. one flat list, range-sharded ---------------------------------------------------------------------------------------------

def flat_inputs(po):
    """The list, its tables, the cut sets and, per keep, the unsharded oracle's results (and the reference build's heaps over the
    oracle's int8 tables)."""
    codes, tables = shard_forms_list()
    n = len(codes)
    want, ref = {}, {}
    for keep in KEEPS:
        want[keep] = [po.query_scan(M, [codes], None, keep, [0], tables[q].copy(), R) for q in range(3)]
        if po.have_ref():
            inter = po.ref_interleave(codes)
            ref[keep] = [po.ref_scan_interleaved(M, [inter], [n], None, want[keep][q]["qtables"][0], R) for q in range(3)]
    return codes, tables, shard_forms_cuts(), want, ref


@pytest.fixture(scope="module")
def flat(po):
    return flat_inputs(po)                                       # computed once, never changed


_rows = {}


def flat_shard(codes, cut, r, keep):
    first, ln = cut[r]
    return Shard(codes[first:first + ln], first, len(codes), None, codes[:start_size(len(codes), keep)])


def rows_streams(pyqadc, codes, tables, cut_name, cut, r, keep, level_base):
    """The row-major index's streams of the same shard and options: once per (cut, rank, keep, levels)."""
    key = (cut_name, r, keep, level_base)
    if key not in _rows:
        form = ROWS._replace(level_base=level_base)
        _rows[key] = rank_streams(pyqadc, form, [flat_shard(codes, cut, r, keep)], keep, np.zeros((3, 1), np.int32), tables)[0]
    return _rows[key]


@path_independent
def test_cut_sets_are_the_planned_ones(pyqadc):
    from pyqadc import sharded
    n = 12 * TILE + 37
    cuts = shard_forms_cuts()
    assert cuts["shard-ranges-2"] == sharded.shard_ranges(n, 2) == [(0, 98320), (98320, n - 98320)] and 98320 % 16 == 0 and 98320 % TILE
    assert cuts["tile-aligned"] == [(0, 6 * TILE), (6 * TILE, 6 * TILE + 37)]
    assert cuts["three-ranks"] == [(0, 4 * TILE + 16), (4 * TILE + 16, 4 * TILE + 32), (8 * TILE + 48, 4 * TILE - 11)]
    assert cuts["four-ranks"] == [(0, 12 * TILE), (12 * TILE, 32), (12 * TILE + 32, 5), (0, 0)]
    assert cuts["first-pos-2-mod-16"][1] == (6 * TILE + 18, 6 * TILE + 19) and (n - 6 * TILE - 18) % 16 != n % 16
    for cut in cuts.values():                                    # contiguous in rank order, 16-byte aligned
        assert sum(ln for _, ln in cut) == n and all(first % 2 == 0 for first, _ in cut)
        assert all(a[0] + a[1] == b[0] for a, b in zip(cut[:-1], cut[1:]) if b[1])



@path_independent
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("form", FLAT_FORMS, ids=form_id)
@pytest.mark.parametrize("cut_name", sorted(shard_forms_cuts()))
def test_flat_shards_merge_to_the_unsharded_oracle(pyqadc, po, flat, cut_name, form, keep):
    """The checks, numbered as in the loop.  7 (the rank's replay equals po.scan_i8 over the shard's own codes, keyed by global
    position) holds for ranks of four tiles and more whose CPU scan replays what the shard replays: po.scan_i8 replays the last of
    the codes it is given (16 - ln % 16) % 16 times, the library the PARTITION's last code, on the last shard only and
    (16 - n % 16) % 16 times.  So both ranks of "first-pos-2-mod-16" are left out of that one comparison (rank 0: 6 tiles + 18
    codes and no replay; rank 1: 6 tiles + 19 codes, 13 replays against the partition's 11; the row-major form differs there in
    the same way); it holds on every other rank of four tiles and more."""
    codes, tables, cuts, wants, refs = flat
    cut, want, n = cuts[cut_name], wants[keep], len(codes)
    assign = np.zeros((3, 1), np.int32)
    outs = []
    for r, (first, ln) in enumerate(cut):
        out, pr = rank_streams(pyqadc, form, [flat_shard(codes, cut, r, keep)], keep, assign, tables)
        check_streams(out, 3)                                                                  # 5.
        check_flat_profile(pr, form, ln)
        outs.append(out)
    first1 = cut[1][0]
    for q in range(3):
        w = want[q]
        assert w["rc"] == 0
        heap = (w["keys"], w["values"])
        if refs:
            assert heaps_equal(refs[keep][q], heap), q
        per_rank = [stream_of(o, q) for o in outs]
        got = pyqadc.replay_i8(np.concatenate([s[0] for s in per_rank]), np.concatenate([s[1] for s in per_rank]), R, sentinel=True)
        assert heaps_equal(got, heap), q                                                       # 1.
        for r, (first, ln) in enumerate(cut):
            assert outs[r]["qmax"][q] == np.float32(w["qmax"]), (q, r)                         # 3.
            mine = pyqadc.replay_i8(per_rank[r][0], per_rank[r][1], R, sentinel=True)
            base = stream_of(rows_streams(pyqadc, codes, tables, cut_name, cut, r, keep, form.level_base), q)
            assert heaps_equal(mine, pyqadc.replay_i8(base[0], base[1], R, sentinel=True)), (q, r)     # 6.
            if ln >= 4 * TILE and ln % 16 == (n % 16 if first + ln == n else 0):                           # 7.
                alone = po.scan_i8(M, [codes[first:first + ln]], [np.arange(first, first + ln, dtype=np.uint32)], w["qtables"], R)
                assert heaps_equal(mine, alone), (q, r)
    for host in (False, True):                                                                 # 2.
        merged = pyqadc.dist_merge_blocks(outs, 3, 1, R, host=host)
        for q in range(3):
            assert heaps_equal(merged[q], (want[q]["keys"], want[q]["values"])), (q, host)
    keys0 = want[0]["keys"]                                                                    # 4.
    assert np.count_nonzero(keys0 == n - 1) == 1 + (16 - n % 16) % 16 == 12
    assert np.count_nonzero(keys0 == first1 - 1) == 1 and np.count_nonzero(keys0 == first1) == 1



@path_independent
@pytest.mark.parametrize("form", [BKTS[1], BKTS[6], MIXED], ids=form_id)
def test_bkt_copy_of_a_shard_is_the_model_of_its_local_codes(pyqadc, flat, form):
    """The copy of a shard whose first code sits off the partition's tiles (first_pos = 6 tiles + 18): blocks from the shard's
    first local code, perm = local positions; the last block of two tiles is ragged (6 tiles + 19 codes)."""
    codes, _, cuts, _, _ = flat
    cut = cuts["first-pos-2-mod-16"]
    first, ln = cut[1]
    idx = make_rank(pyqadc, form, [flat_shard(codes, cut, 1, 0.01)], 0.01)
    try:
        copy = idx.bkt_copy(0)
    finally:
        idx.close()
    assert copy is not None and copy["block"] == form.block and ln % form.block not in (0, form.block)
    bkt_model.check_copy(copy, codes[first:first + ln], form.block)



# ---- b. sharded IVF: several labelled partitions -----------------------------------------------------------------------------------

IVF_SIZES = [8 * TILE + 53, 37, 16, 6 * TILE + 9, 0]
IVF_KEEP, IVF_WORLD = 0.05, 3
# partition 0 first (queries 0 and 3) and behind others (1 and 2), partition 3 first (1) and behind others (0, 2); partition 4 is empty
IVF_ASSIGN = np.array([[0, 1, 3], [3, 2, 0], [1, 0, 3], [2, 4, 0]], np.int32)


def ivf_inputs(po):
    rng = np.random.default_rng(4302)
    parts = [rand_codes(rng, s, M) for s in IVF_SIZES]
    for p in parts:
        p[:, 1] &= 3
    labels = [rng.integers(0, 1 << 32, s, dtype=np.uint32) for s in IVF_SIZES]
    nq, ma = IVF_ASSIGN.shape
    tables = float_tables(rng, nq, ma, M)
    parts[0][-1] = best_code(tables[0, 0])                       # a candidate with its replays behind the last rank's ragged end
    parts[0][shard_ranges(IVF_SIZES[0], IVF_WORLD)[1][0] - 1] = parts[0][-1]      # ... and rank 0's last code of it: once, no replay
    want = [po.query_scan(M, parts, labels, IVF_KEEP, IVF_ASSIGN[q], tables[q].copy(), R) for q in range(nq)]
    return parts, labels, tables, want


@pytest.fixture(scope="module")
def ivf(po):
    return ivf_inputs(po)


@path_independent
@pytest.mark.parametrize("form", IVF_FORMS, ids=form_id)
def test_ivf_shards_of_every_form_merge_by_assign_slot(pyqadc, po, ivf, form):
    """Three ranks by shard_ranges: ranks 0 and 1 hold 43 696 codes of partition 0 and two tiles of partition 3 and nothing of
    the small ones, rank 2 the ragged ends and the small partitions.  A partition probed first is cut on its tiles; behind
    another one its first run still starts on a tile (its first code) and the next one does not: that one keeps the row-major
    form inside a split index.  On ranks 0 and 1 every query's level-0 run is the first tile of a large partition, so level 0 is
    one launch of the form."""
    parts, labels, tables, want = ivf
    nq, ma = IVF_ASSIGN.shape
    outs = []
    for r in range(IVF_WORLD):
        shards = []
        for p, s in enumerate(IVF_SIZES):
            first, ln = shard_ranges(s, IVF_WORLD)[r] if s else (0, 0)
            shards.append(Shard(parts[p][first:first + ln], first, s, labels[p][first:first + ln], parts[p][:start_size(s, IVF_KEEP)]))
        held = [len(s.codes) for s in shards]
        assert held == ([43696, 0, 0, 2 * TILE, 0] if r < 2 else [43733, 37, 16, 2 * TILE + 9, 0])
        out, pr = rank_streams(pyqadc, form, shards, IVF_KEEP, IVF_ASSIGN, tables)
        check_streams(out, nq)
        if form.kind == "rows":
            assert pr["split_codes"] == pr["split_launches"] == 0 and pr["split_copy_bytes"] == 0, pr
        else:
            assert 0 < pr["split_codes"] < pr["scan_codes"] and 0 < pr["split_launches"] < pr["scan_launches"], pr
            own = sum(pr[k] for k in PER_FORM)
            assert own == (0 if form == PLANES[0] else pr["split_launches"]), pr
            if r < 2:
                assert pr[counter_of(form)] > 0, pr
        outs.append(out)
    for q in range(nq):
        w = want[q]
        assert w["rc"] == 0
        ks, vs = [], []
        for slot in range(ma):
            for o in outs:
                assert o["qmax"][q] == np.float32(w["qmax"])
                k, v, s = stream_of(o, q)
                ks.append(k[s == slot])
                vs.append(v[s == slot])
        got = pyqadc.replay_i8(np.concatenate(ks), np.concatenate(vs), R, sentinel=True)
        assert heaps_equal(got, (w["keys"], w["values"])), q
    for host in (False, True):
        merged = pyqadc.dist_merge_blocks(outs, nq, ma, R, host=host)
        for q in range(nq):
            assert heaps_equal(merged[q], (want[q]["keys"], want[q]["values"])), (q, host)
    reps = (16 - IVF_SIZES[0] % 16) % 16
    assert reps and np.count_nonzero(want[0]["keys"] == labels[0][-1]) >= 1 + reps
    assert np.count_nonzero(want[0]["keys"] == labels[0][43695]) >= 1



# ---- c. a partition held from the middle, with a key base ------------------------------------------------------------------------

KEY_BASE = 3_000_000_000                                         # keys above 2^31: key_base + first_pos + position in 32 bits


@path_independent
@pytest.mark.parametrize("form", FLAT_FORMS, ids=form_id)
def test_middle_shard_keys_are_key_base_plus_first_pos_plus_position(pyqadc, po, flat, form):
    """Rank 1 of the three-rank cut: [4 tiles + 16, 8 tiles + 48), a multiple of 16 codes and not the partition's end, so the CPU
    scan of these codes alone, labelled key_base + first_pos + position, is what the rank must replay to (no padding-lane
    replay on either side).  Its first code is query 0's best one: key_base + first_pos itself is in the heap."""
    codes, tables, cuts, wants, _ = flat
    keep = KEEPS[0]
    first, ln = cuts["three-ranks"][1]
    assert ln % 16 == 0 and first % TILE and first + ln < len(codes) and KEY_BASE + first + ln < 1 << 32
    shard = Shard(codes[first:first + ln], first, len(codes), None, codes[:start_size(len(codes), keep)])
    out, pr = rank_streams(pyqadc, form, [shard], keep, np.zeros((3, 1), np.int32), tables, key_base=KEY_BASE)
    check_streams(out, 3)
    check_flat_profile(pr, form, ln)
    keys = (KEY_BASE + np.arange(first, first + ln, dtype=np.uint64)).astype(np.uint32)
    for q in range(3):
        k, v, _ = stream_of(out, q)
        got = pyqadc.replay_i8(k, v, R, sentinel=True)
        alone = po.scan_i8(M, [shard.codes], [keys], wants[keep][q]["qtables"], R)
        assert heaps_equal(got, alone), q
        assert len(k) and k.min() >= KEY_BASE + first and k.max() < KEY_BASE + first + ln, q
    k0 = pyqadc.replay_i8(*stream_of(out, 0)[:2], R, sentinel=True)[0]
    assert np.count_nonzero(k0 == KEY_BASE + first) == 1

