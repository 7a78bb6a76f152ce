"""CPU: the planner of the int8 level path (quick-adc_amd/host/level_plan.hpp, driver tests/cpp/level_plan_host.cpp).

Every exactness argument of DESIGN.md section 4 rests on what plan_levels emits: which codes land in which bound level,
that every run is 16-byte aligned and at most 2^31 codes long, the padding replay fields, which runs may read the byte-plane
copy, the pre-scan items, and kernel and grid of every launch.  Each case below is planned by the header as the library compiles
it, with fake partition base addresses (nothing is dereferenced), and the whole plan is checked here, query by query; the level
edges are recomputed from level_base / level_growth, not taken from the plan."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "level_plan_host")
REFUSAL = "assign[] names a partition that does not exist"
U64, NONE = (1 << 64) - 1, 0xffffffff
TILE, PLANES, LEVELS = 16384, 7, 16
OPTS = dict(M=16, level_base=512, level_growth=4, head_level=5, small_run=1 << 17, wgs_per_item=0, share_variant=0x41, mq=1,
            prescan_sample=1 << 16, split_min_run=1 << 23, split6_min_run=1 << 25)          # the index's defaults
BATCH = dict(R=100, mode=0, float_path=1, full_prescan=0, pre_slice=0, pre_nslices=1, inj_n=0)
ITEM = ("codes", "labels", "n", "pos0", "key_base", "table", "query", "order", "dup_pos", "dup_reps", "split")
START = ("codes", "n", "table", "query", "out_off", "filter")
LAUNCH = ("first", "nitems", "wgs", "codes", "small", "shared", "mq", "split", "split6", "maxn")


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "level_plan_host.cpp"), EXE, link=False)
    return EXE


def part(n, global_n=None, first_pos=0, labels=False, starts=False, split=False, start_n=None, key_base=0):
    """a partition descriptor; the fake base addresses are filled in by `plan` from the partition's index"""
    global_n = n if global_n is None else global_n
    start_n = (max(1, global_n // 100) if global_n else 0) if start_n is None else start_n
    return dict(n=n, global_n=global_n, first_pos=first_pos, start_n=start_n, key_base=key_base, has=(labels, starts, split))


def plan(exe, tmp_path, parts, assign, **kw):
    """-> (options, batch, partitions with their fake addresses, the plan as a dict of arrays or the refusal's message)"""
    o = dict(OPTS, **{k: v for k, v in kw.items() if k in OPTS})
    b = dict(BATCH, **{k: v for k, v in kw.items() if k in BATCH})
    assert set(kw) <= set(o) | set(b)
    assign = np.ascontiguousarray(assign, np.int32)
    nq, ma = assign.shape
    parts = [dict(p) for p in parts]
    for i, p in enumerate(parts):                       # bases 2^40 apart: the longest partition has 2^32 x 16 = 2^36 bytes
        p["d_codes"] = (4 * i + 1) << 40
        p["d_labels"], p["d_starts"], p["d_split"] = (((4 * i + 2 + j) << 40) if p["has"][j] else 0 for j in range(3))
    fin, fout = str(tmp_path / "plan.in"), str(tmp_path / "plan.out")
    with open(fin, "wb") as f:
        np.array([o[k] for k in OPTS] + [nq, ma] + [b[k] for k in BATCH] + [len(parts)], np.int64).tofile(f)
        np.array([[p[k] for k in ("d_codes", "d_labels", "d_starts", "d_split", "n", "global_n", "first_pos", "start_n", "key_base")]
                  for p in parts], np.uint64).tofile(f)
        assign.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    text = out.stdout.decode().strip()
    assert out.returncode == 0, out.stderr.decode()
    if text.startswith("refused: "):
        return o, b, parts, text[len("refused: "):]
    assert text == "ok"
    w = [int(x) for x in np.fromfile(fout, np.uint64)]
    assert w[:3] == [TILE, PLANES, LEVELS]
    n_items, na, nb, nl = w[3:7]
    p = dict(fc_stride=w[7], head_codes=w[8], start_codes=w[9])
    at = 10
    for name, fields, count in (("items", ITEM, n_items), ("a", START, na), ("b", START, nb), ("fc_init", ("sample", "cap"), nq),
                                ("launches", LAUNCH, nl)):
        rows = [w[at + i * len(fields):at + (i + 1) * len(fields)] for i in range(count)]
        p[name] = [dict(zip(fields, r)) for r in rows]
        at += count * len(fields)
    assert at == len(w)
    return o, b, parts, p


def level_edges(o):
    L, e = [0], max(o["level_base"], 16)
    for _ in range(1, LEVELS):
        L.append(e)
        e = U64 if e > (U64 >> 8) else e * max(o["level_growth"], 2)
    return L + [U64]


def check_scan_items(o, b, parts, assign, p):
    """tiling, order, addressing, padding replay and split form of every query's runs"""
    cs = o["M"] // 2
    cpl = 16 // cs
    L = level_edges(o)
    k0 = o["head_level"] if b["mode"] != 1 and o["head_level"] > 0 else 0
    assert p["head_codes"] == (L[k0] if k0 else 0)
    nq, ma = assign.shape
    for it in p["items"]:
        it["level"], it["slot"] = it["order"] >> 16, it["order"] & 0xffff
        assert it["query"] < nq and it["slot"] < ma and it["table"] == it["query"] * ma + it["slot"]
    if b["mode"] == 1:
        assert not p["items"] and not p["launches"]
    for q in range(nq):
        mine = [it for it in p["items"] if it["query"] == q]
        assert [it["level"] for it in sorted(mine, key=lambda it: (it["slot"], it["pos0"]))] == \
            [it["level"] for it in sorted(mine, key=lambda it: (it["level"], it["slot"], it["pos0"]))]     # never decreases along the scan
        c = 0                                                                    # scan position of the partition's first code
        for a in range(ma):
            pt = parts[assign[q, a]]
            runs = sorted((it for it in mine if it["slot"] == a), key=lambda it: (it["level"], it["pos0"]))
            if pt["global_n"] == 0 or pt["n"] == 0 or b["mode"] == 1:
                assert not runs
                continue
            n = pt["n"]
            # the head's share [0, h): the codes below edge L[k0], cut back to a 16-byte boundary unless the partition ends first
            h = n if c + n <= L[k0] else max(L[k0] - c, 0) // cpl * cpl
            at = h
            for i, it in enumerate(runs):
                k, end = it["level"], it["pos0"] + it["n"]
                assert it["pos0"] == at and 1 <= it["n"] <= 1 << 31 and k >= k0       # covered exactly once, in order
                assert c + end <= L[k + 1]                                            # every code lies below the level's upper edge
                assert c + it["pos0"] > L[k] - cpl or k == 0                          # ... and none was left to a later level than its own
                if end < n:
                    nxt = runs[i + 1]["level"]
                    assert (nxt == k and it["n"] == 1 << 31) or (nxt > k and L[k + 1] - cpl < c + end)   # the 2^31 cut / a level cut
                    assert end % cpl == 0
                assert it["codes"] == pt["d_codes"] + it["pos0"] * cs and it["pos0"] * cs % 16 == 0
                assert it["labels"] == pt["d_labels"] and it["key_base"] == pt["key_base"] + pt["first_pos"]
                assert it["dup_pos"] == (n - 1 if pt["first_pos"] + n == pt["global_n"] else NONE)
                assert it["dup_reps"] == (16 - pt["global_n"] % 16) % 16
                may_split = pt["d_split"] and it["pos0"] % TILE == 0 and it["n"] >= max(o["split_min_run"], o["small_run"])
                assert it["split"] == (pt["d_split"] + it["pos0"] // TILE * PLANES * TILE if may_split else 0)
                at = end
            assert at == n
            c += n


def expected_wgs(o, ll, cpl):
    nvec, cnt, wpi = -(-ll["maxn"] // cpl), ll["nitems"], o["wgs_per_item"]
    if ll["mq"]:
        w = wpi if wpi > 0 else -(-ll["maxn"] // (1 << 16))
        w = max(w, -(-4096 // (-(-cnt // 8))))
        w = min(w, 65536, max(max(-(-nvec // 256), 1) // 4, 1))
    elif ll["shared"]:
        w = min(max(wpi if wpi > 0 else -(-ll["maxn"] // (1 << 20)), 64), 512, max(-(-nvec // 4096), 1))
    elif ll["small"]:
        return min(max(-(-nvec // 512), 1), max(1, 4096 // cnt))
    else:
        units = -(-ll["maxn"] // TILE) if ll["split"] else -(-nvec // 4096)
        return min(max(units, 1), wpi if wpi > 0 else (1024 if o["M"] == 16 else 512), max(1, 8192 // cnt))
    return w & ~7 if w >= 8 else w


def check_launches(o, p):
    """the launches partition the item array: per level small runs, long runs, long runs with a byte-plane copy"""
    cpl = 16 // (o["M"] // 2)
    at, prev = 0, (-1, -1)
    for ll in p["launches"]:
        assert ll["first"] == at and ll["nitems"] >= 1
        its = p["items"][at:at + ll["nitems"]]
        at += ll["nitems"]
        cls = {(it["level"], 0 if it["n"] < o["small_run"] else 2 if it["split"] else 1) for it in its}
        assert len(cls) == 1                                                      # one level, one class
        (level, c), = cls
        assert (level, c) > prev                                                  # levels ascend; within one: small, long, long with copy
        prev = (level, c)
        order = [(it["query"], it["slot"], it["pos0"]) for it in its]
        assert order == sorted(order)                                             # query by query in scan order
        same = all(all(it[f] == its[0][f] for f in ("codes", "n", "pos0", "labels", "key_base", "dup_pos", "dup_reps")) for it in its)
        assert ll["small"] == (c == 0)
        assert ll["shared"] == (len(its) >= 2 and same and o["share_variant"] != 0 and c != 0)
        assert ll["mq"] == (ll["shared"] and o["mq"] != 0)
        assert ll["split"] == (c == 2 and not ll["shared"])
        assert ll["split6"] == (ll["split"] and o["split6_min_run"] != 0 and min(it["n"] for it in its) >= o["split6_min_run"])
        assert ll["maxn"] == max(it["n"] for it in its) and ll["codes"] == sum(it["n"] for it in its)
        assert ll["wgs"] >= 1 and ll["wgs"] == expected_wgs(o, ll, cpl)
        if (ll["shared"] or ll["mq"]) and ll["wgs"] >= 8:
            assert ll["wgs"] % 8 == 0
    assert at == len(p["items"])


def check_prescan(o, b, parts, assign, p):
    """phase A + phase B items tile the start range of every probed partition; sample, capacity, stride"""
    cs = o["M"] // 2
    nq, ma = assign.shape
    for si in p["a"] + p["b"]:
        assert si["table"] // ma == si["query"] < nq                           # (table % ma = the assign slot, checked below)
    total, stride = 0, 1
    for q in range(nq):
        ranges = []                                                               # (slot, first address, length) of what is pre-scanned
        for a in range(ma):
            pt = parts[assign[q, a]]
            lo, ln = 0, pt["start_n"]
            if b["mode"] == 1 and b["pre_nslices"] > 1:
                lo = pt["start_n"] * b["pre_slice"] // b["pre_nslices"] & ~15
                hi = pt["start_n"] if b["pre_slice"] + 1 == b["pre_nslices"] else pt["start_n"] * (b["pre_slice"] + 1) // b["pre_nslices"] & ~15
                ln = max(hi - lo, 0)
            if b["mode"] == 2 or not b["float_path"] or pt["global_n"] == 0:
                ln = 0
            if ln:
                ranges.append((a, (pt["d_starts"] or pt["d_codes"]) + lo * cs, ln))
        stotal = sum(r[2] for r in ranges)
        one_phase = b["full_prescan"] or stotal <= 2 * o["prescan_sample"]
        sample = stotal if one_phase else o["prescan_sample"]
        A = [si for si in p["a"] if si["query"] == q]
        B = [si for si in p["b"] if si["query"] == q]
        assert (not B) == bool(one_phase)
        got = sorted(((si["table"] % ma, si["filter"], si["codes"], si["n"]) for si in A + B))
        for a, addr, ln in ranges:                                                # each range: its A part, then its B part, nothing else
            mine = [g for g in got if g[0] == a]
            assert [g[1] for g in mine] in ([0], [1], [0, 1]) and mine[0][2] == addr and sum(g[3] for g in mine) == ln
            assert len(mine) == 1 or mine[1][2] == addr + mine[0][3] * cs
        assert len(got) == sum(len([g for g in got if g[0] == r[0]]) for r in ranges) and len({r[0] for r in ranges}) == len(ranges)
        off = 0
        for si in A:                                                              # in slot order: consecutive in the value buffer
            assert si["filter"] == 0 and si["out_off"] == off and si["n"] >= 1
            off += si["n"]
        assert all(si["filter"] == 1 and si["out_off"] == 0 and si["n"] >= 1 for si in B)
        cap = sample
        if sample < stotal:
            cap += min(stotal - sample, max(16 * b["R"] * -(-stotal // sample), 4096))
        if b["mode"] == 2:
            assert not A and not B
            off = sample = cap = b["inj_n"]
        assert off == sample and p["fc_init"][q] == dict(sample=sample, cap=cap)
        stride = max(stride, cap)
        total += stotal
    assert p["fc_stride"] == stride and p["start_codes"] == total


def run(driver, tmp_path, parts, assign, **kw):
    o, b, parts, p = plan(driver, tmp_path, parts, assign, **kw)
    assert isinstance(p, dict), p
    assign = np.asarray(assign, np.int64)
    check_scan_items(o, b, parts, assign, p)
    check_launches(o, p)
    check_prescan(o, b, parts, assign, p)
    return p


EDGES = [512 * 4 ** (k - 1) for k in range(1, 7)]                                   # L[1] .. L[6] of the default options


@pytest.mark.parametrize("small_run", [1, 1 << 17, 1 << 20])                         # every run long / both kinds / every run small
@pytest.mark.parametrize("head_level", [0, 5])
@pytest.mark.parametrize("M", [16, 32])
def test_one_partition_one_query_around_every_edge(driver, tmp_path, M, head_level, small_run):
    for n in [0, 1, 15, 16, 17] + [e + d for e in EDGES for d in (-1, 0, 1)]:
        p = run(driver, tmp_path, [part(n)], [[0]], M=M, head_level=head_level, small_run=small_run)
        edges = [0] + EDGES + [U64]
        levels = [k for k in range(7) if n > edges[k]]                               # the levels [L[k], L[k + 1]) the partition reaches
        assert [it["level"] for it in p["items"]] == [k for k in levels if k >= head_level], n
        assert all(ll["nitems"] == 1 and ll["small"] == (ll["maxn"] < small_run) and not ll["shared"] for ll in p["launches"])


@pytest.mark.parametrize("share_variant,mq", [(0x41, 1), (0, 1), (0x41, 0)])
@pytest.mark.parametrize("nq", [8, 4, 3])
def test_queries_over_one_flat_list_share_their_launches(driver, tmp_path, nq, share_variant, mq):
    p = run(driver, tmp_path, [part(2247152)], [[0]] * nq, share_variant=share_variant, mq=mq)
    assert [ll["nitems"] for ll in p["launches"]] == [nq] * 3                         # levels 5, 6, 7 behind the head
    assert p["launches"][2]["wgs"] == (72 if p["launches"][2]["mq"] else 16 if share_variant else 19)    # 150000 codes: 19 units of 4096 vectors
    assert all(ll["shared"] == (share_variant != 0) and ll["mq"] == (share_variant != 0 and mq == 1) for ll in p["launches"])
    p = run(driver, tmp_path, [part(2247152)], [[0]] * nq, share_variant=share_variant, mq=mq, wgs_per_item=24)
    assert all(ll["wgs"] % 8 == 0 for ll in p["launches"] if ll["shared"])


SIZES = [0, 700, 0, 9000, 3, 140000]
ROWS = [[1, 3, 5, 4], [5, 5, 0, 2], [0, 2, 0, 2], [4, 1, 3, 3], [3, 5, 1, 5]]         # unequal rows, partitions probed twice, only empty ones


@pytest.mark.parametrize("float_path", [1, 0])
@pytest.mark.parametrize("head_level", [0, 5])
@pytest.mark.parametrize("M", [16, 32])
def test_ma4_over_unequal_partitions(driver, tmp_path, M, head_level, float_path):
    parts = [part(n, labels=i % 2 == 1, key_base=1000 * i) for i, n in enumerate(SIZES)]
    p = run(driver, tmp_path, parts, ROWS, M=M, head_level=head_level, float_path=float_path, small_run=5000)
    assert not [it for it in p["items"] if it["query"] == 2]                          # a query that probes only empty partitions
    assert bool(p["a"]) == bool(float_path)
    run(driver, tmp_path, parts, ROWS, M=M, head_level=head_level, float_path=float_path, small_run=5000, wgs_per_item=3)


@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("opts", [dict(level_base=1 << 40, head_level=0), dict(level_base=16, level_growth=2)])
def test_a_run_is_cut_at_2_31_codes(driver, tmp_path, opts, M):
    """one bound level over all of the partition / a last level [2^18, inf) behind the head: its run is longer than 2^31 codes"""
    n = (1 << 31) + (1 << 20) + 6
    p = run(driver, tmp_path, [part(n)], [[0]], M=M, **opts)
    assert [it["n"] for it in p["items"]][-2] == 1 << 31 and sum(it["n"] for it in p["items"]) == n - p["head_codes"]
    assert p["items"][-1]["level"] == p["items"][-2]["level"] == (0 if "head_level" in opts else 15)


COPY = [part(1000), part(600000, split=True), part(0), part(50000, split=True)]


@pytest.mark.parametrize("small_run", [1 << 14, 1 << 17])
def test_runs_of_a_partition_with_a_byte_plane_copy(driver, tmp_path, small_run):
    """query 0 meets partition 1 at scan position 0 (cuts on tile boundaries from level 4 on), query 1 behind 1000 other codes (cuts off
    them); lengths 17232 / 98304 / 393216 / 75712 against split_min_run 40000, split6_min_run 100000 and small_run"""
    kw = dict(head_level=0, small_run=small_run, split_min_run=40000, split6_min_run=100000)
    p = run(driver, tmp_path, COPY, [[1, 2], [0, 1], [3, 2]], **kw)
    split = {(it["query"], it["level"]): it["split"] != 0 for it in p["items"] if it["slot"] == (1 if it["query"] == 1 else 0)}
    assert [split[0, k] for k in (3, 4, 5, 6)] == [False, small_run <= 98304, True, small_run <= 75712]
    assert not any(v for (q, _), v in split.items() if q == 1) and not split[2, 4]   # off the tiles / on a tile, but 17232 codes
    assert [(ll["split"], ll["split6"]) for ll in p["launches"] if ll["split"]] == \
        [(True, False)] * (small_run <= 98304) + [(True, True)] + [(True, False)] * (small_run <= 75712)
    p = run(driver, tmp_path, COPY, [[1, 2], [0, 1]], **dict(kw, split6_min_run=0))
    assert any(ll["split"] for ll in p["launches"]) and not any(ll["split6"] for ll in p["launches"])
    p = run(driver, tmp_path, COPY + [part(196608, split=True)], [[1, 2], [4, 2]], **kw)
    assert [ll["split6"] for ll in p["launches"] if ll["split"] and ll["maxn"] == 393216] == [small_run > 65536]   # beside a long run of 65536 codes: not
    p = run(driver, tmp_path, COPY, [[1, 2], [1, 2]], **kw)                           # two queries over the same runs: shared, not split
    assert all(ll["shared"] and not ll["split"] and not ll["split6"] for ll in p["launches"] if not ll["small"])
    assert any(it["split"] for it in p["items"])


@pytest.mark.parametrize("M", [16, 32])
def test_a_sharded_partition(driver, tmp_path, M):
    """local ranges [40000, 70000) and [70000, 100003) of a partition of 100003 codes (the second holds the global end), and a partition
    of which only the starts replica is here"""
    parts = [part(30000, global_n=100003, first_pos=40000, starts=True, key_base=7),
             part(30003, global_n=100003, first_pos=70000, starts=True, labels=True), part(0, global_n=5000, starts=True)]
    p = run(driver, tmp_path, parts, [[0, 1, 2], [2, 1, 0]], M=M, head_level=2, small_run=4000)
    assert {it["dup_pos"] for it in p["items"] if it["table"] % 3 == it["query"]} == {NONE, 30002}     # (slot == query: partitions 0 / 1)
    assert all(it["dup_reps"] == 13 for it in p["items"])
    assert not [it for it in p["items"] if (it["query"], it["slot"]) in ((0, 2), (1, 0))]             # starts only
    assert sorted(si["n"] for si in p["a"]) == [50, 50, 1000, 1000, 1000, 1000]


@pytest.mark.parametrize("full_prescan", [0, 1])
def test_prescan_phases_by_the_number_of_starts(driver, tmp_path, full_prescan):
    """sample 100: rows of 60, 150, 200 (one phase), 201 and 450 starts (two, unless the batch pre-scans everything)"""
    parts = [part(6000, start_n=60), part(9000, start_n=90), part(30000, start_n=300), part(0), part(20000, start_n=200),
             part(20100, start_n=201)]
    rows = [[0, 3, 3], [0, 1, 3], [4, 3, 3], [3, 5, 3], [0, 1, 2], [2, 1, 0]]
    p = run(driver, tmp_path, parts, rows, prescan_sample=100, full_prescan=full_prescan, R=10)
    assert sorted({si["query"] for si in p["b"]}) == ([] if full_prescan else [3, 4, 5])
    assert [c["sample"] for c in p["fc_init"]] == ([60, 150, 200, 201, 450, 450] if full_prescan else [60, 150, 200, 100, 100, 100])


@pytest.mark.parametrize("start_n", [1, 47, 48, 1000])
def test_prescan_only_batches_slice_the_starts_at_16_codes(driver, tmp_path, start_n):
    parts = [part(100 * start_n, start_n=start_n, starts=True), part(0)]
    seen = 0
    for sl in range(3):
        p = run(driver, tmp_path, parts, [[0, 1], [1, 0]], mode=1, pre_slice=sl, pre_nslices=3)
        assert p["head_codes"] == 0 and not p["b"]
        assert sl == 2 or all(si["n"] % 16 == 0 for si in p["a"])
        seen += sum(si["n"] for si in p["a"] if si["query"] == 0)
    assert seen == start_n                                                            # the slices together: every start once
    assert run(driver, tmp_path, parts, [[0, 1]], mode=1)["start_codes"] == start_n   # (one slice: all of them)


def test_injected_prescan_values_stand_in_for_the_start_items(driver, tmp_path):
    parts = [part(n) for n in SIZES]
    p = run(driver, tmp_path, parts, ROWS, mode=2, inj_n=7, head_level=0)
    assert not p["a"] and not p["b"] and p["fc_stride"] == 7 and p["start_codes"] == 0 and p["items"]


@pytest.mark.parametrize("bad", [-1, len(SIZES)])
@pytest.mark.parametrize("float_path", [1, 0])
def test_an_assign_entry_outside_the_partition_table_is_refused(driver, tmp_path, bad, float_path):
    rows = [ROWS[0], [5, bad, 0, 2]]
    assert plan(driver, tmp_path, [part(n) for n in SIZES], rows, float_path=float_path)[3] == REFUSAL
