"""CPU: the launch geometry of the exact range search (quick-adc_amd/host/refine_range_plan.hpp, driver
tests/cpp/refine_range_plan_host.cpp).  The launches of qadc_refine_range and qadc_refine_rerank_range do
what the header plans and the kernels index by it, so the header as the library compiles it is held here to what the kernels rely
on: every row is in exactly one (launch, group, slice, wave), every query in one (pass, tile), the candidate chunks cover every
segment exactly once (empty segments and segments of one candidate included), the regions lie one behind the other, a second run
has regions of exactly the counted sizes, and the QADC_REFINE_RANGE_MAX_ENTRIES refusal and the argument refusals, as pure
functions."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_range_plan_host")
NAMES = ("qt", "jregs", "dist_lds_bytes", "pass_nq", "passes", "region_rows", "chunk_rows", "groups", "slice_rows", "slices", "launches",
         "fewest_visits", "most_visits")
TILES = {(32, 1), (32, 2), (16, 3), (16, 4), (4, 1), (4, 2), (4, 3), (4, 4), (32, 0), (16, 0), (8, 0), (4, 0)}   # the instantiated (QT, J)
REG_BUDGET, LDS_DEFAULT, DEFAULT_CHUNK, DEFAULT_REGION, SCRATCH, MAX_ENTRIES = 64, 64 * 1024, 7168, 4096, 256 << 20, 1 << 31
MAX_CANDS_PER_WG, IN_FLIGHT, WG_FLOOR, PASS_CANDS = 64, 4, 1024, 1 << 24

NQ = (1, 3, 4, 5, 31, 32, 33, 65, 1000, 100000)
DIM = (1, 63, 64, 65, 128, 129, 192, 256, 257, 512, 960, 1024, 1025, 2048, 4096)
ROWS = (0, 1, 63, 64, 65, 600, 7167, 7168, 7169, 21505, 57344, 57345, 60001)


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def run(exe, tmp_path, what, data, dtype=np.int64, out_dtype=np.int64):
    fin, fout = str(tmp_path / (what + ".in")), str(tmp_path / (what + ".out"))
    np.asarray(data, dtype).reshape(-1).tofile(fin)
    out = subprocess.run([exe, what, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", (out.returncode, out.stderr.decode())
    return np.fromfile(fout, out_dtype)


def plans(exe, tmp_path, shapes):
    got = run(exe, tmp_path, "plans", shapes).reshape(len(shapes), 14)
    return [None if not g[0] else dict(zip(NAMES, (int(v) for v in g[1:]))) for g in got]


def test_the_plan_covers_rows_and_queries_once_and_fits_the_chip(driver, tmp_path):
    shapes = [(nq, rows, dim, region, chunk, pass_nq) for nq in NQ for dim in DIM for region in (0, 64) for chunk in (0, 100) for pass_nq in (0, 33)
              for rows in (600, 7169)]
    shapes += [(nq, rows, 65, region, chunk, 0) for nq in (1, 33) for region in (0, 1, 64, 5000, 10 ** 6) for chunk in (0, 1, 64, 7168, 20000)
               for rows in ROWS]
    got = plans(driver, tmp_path, shapes)
    for shape, p in zip(shapes, got):
        nq, rows, dim, region, chunk, pass_nq = shape
        assert p is not None, "an admitted shape is refused: %s" % (shape,)
        chunk = chunk or DEFAULT_CHUNK
        assert p["fewest_visits"] == 1 and p["most_visits"] == 1, (shape, p)
        assert p["chunk_rows"] == chunk and p["launches"] == -(-rows // (p["groups"] * chunk)) and p["slices"] == -(-chunk // p["slice_rows"]), (shape, p)
        assert 1 <= p["groups"] * p["slices"] <= 65535, (shape, p)                              # the distance grid's second dimension
        assert p["region_rows"] == max(1, min(region or DEFAULT_REGION, rows)), (shape, p)
        assert p["pass_nq"] >= 1 and p["passes"] == -(-nq // p["pass_nq"]) and (p["passes"] - 1) * p["pass_nq"] < nq, (shape, p)
        if pass_nq:
            assert p["pass_nq"] == min(nq, pass_nq), (shape, p)
        else:                                                                                   # the first run's regions stay within the scratch
            assert p["pass_nq"] * p["region_rows"] * 8 <= max(SCRATCH, p["region_rows"] * 8), (shape, p)
        assert p["pass_nq"] * p["region_rows"] <= MAX_ENTRIES or pass_nq, (shape, p)
        assert (p["qt"], p["jregs"]) in TILES, (shape, p)
        if p["jregs"]:
            assert p["jregs"] == -(-dim // 64) and p["qt"] * p["jregs"] <= REG_BUDGET and p["dist_lds_bytes"] == 0, (shape, p)
        else:
            assert dim > 256 and p["dist_lds_bytes"] == p["qt"] * dim * 4 <= LDS_DEFAULT, (shape, p)
    assert {(p["qt"], p["jregs"]) for p in got} == TILES
    assert any(p["passes"] > 1 for p in got) and any(p["launches"] > 1 for p in got) and {p["slice_rows"] for p in got} >= {16, 512}


def test_the_plan_refuses_what_the_kernels_do_not_take(driver, tmp_path):
    bad = [(0, 10, 8, 0, 0, 0), (-1, 10, 8, 0, 0, 0), (1, 10, 0, 0, 0, 0), (1, 10, 4097, 0, 0, 0), (1, 10, 8, 0, 0, -1), (1, 10, 8, 0, (1 << 24) + 1, 0)]
    assert plans(driver, tmp_path, bad) == [None] * len(bad)


def cand_passes(exe, tmp_path, lims, pass_nq=0, max_entries=MAX_ENTRIES):
    nq = len(lims) - 1
    out = run(exe, tmp_path, "chunks", [nq, pass_nq, max_entries] + [int(x) for x in lims]).tolist()
    if not out[0]:
        return None
    passes, at = [], 2
    for _ in range(out[1]):
        q0, q1, cpw, n = out[at:at + 4]
        table = np.array(out[at + 4:at + 4 + 3 * n], np.int64).reshape(n, 3)
        passes.append((q0, q1, cpw, table))
        at += 4 + 3 * n
    assert at == len(out)
    return passes


@pytest.mark.parametrize("pass_nq", [0, 1, 3])
def test_the_candidate_chunks_cover_every_segment_exactly_once(driver, tmp_path, pass_nq):
    rng = np.random.default_rng(3 + pass_nq)
    shapes = [[0], [1], [0, 0, 0], [0, 1, 0, 63, 64, 65, 0, 8193, 1, 0], [5] * 40, [70000, 3, 0, 1 << 17],
              rng.integers(0, 300, 500).tolist(), [PASS_CANDS - 10, 20, 5], [PASS_CANDS + 1, 1], [3, PASS_CANDS + 7, 0, 2]]
    for sizes in shapes:
        lims = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        passes = cand_passes(driver, tmp_path, lims, pass_nq)
        assert passes is not None
        nq, at = len(sizes), 0
        for q0, q1, cpw, table in passes:                                                       # whole queries, in order, each once
            assert q0 == at and q0 < q1 <= nq and (not pass_nq or q1 - q0 <= pass_nq), (sizes[:12], q0, q1)
            entries = int(lims[q1] - lims[q0])
            assert q1 - q0 == 1 or entries <= PASS_CANDS
            assert cpw in (4, 8, 16, 32, 64) and cpw % IN_FLIGHT == 0
            if cpw > IN_FLIGHT:                                                                 # cut finer only while the pass has few workgroups
                assert len(table) >= WG_FLOOR or cpw == MAX_CANDS_PER_WG
            seen = np.zeros(entries, np.int64)
            for q, first, count in table.tolist():
                assert 1 <= count <= cpw and 0 <= q < q1 - q0
                lo, hi = int(lims[q0 + q] - lims[q0]), int(lims[q0 + q + 1] - lims[q0])
                assert lo <= first and first + count <= hi, "a chunk leaves its query's segment"
                seen[first:first + count] += 1
            assert (seen == 1).all()
            assert (np.diff(table[:, 1]) > 0).all() if len(table) > 1 else True
            at = q1
        assert at == nq


def test_one_query_above_the_limit_is_refused(driver, tmp_path):
    assert cand_passes(driver, tmp_path, [0, 5, 106, 107], 0, 100) is None                       # 101 candidates in one query
    assert cand_passes(driver, tmp_path, [0, 5, 105, 107], 0, 100) is not None
    assert cand_passes(driver, tmp_path, [0, MAX_ENTRIES + 1], 0) is None and cand_passes(driver, tmp_path, [0, MAX_ENTRIES], 1) is not None


def regions(exe, tmp_path, cap, count, max_entries=MAX_ENTRIES):
    n = len(cap)
    out = run(exe, tmp_path, "regions", [n, max_entries] + list(cap) + list(count)).tolist()
    return dict(ok=out[0], entries=out[1], base=out[2:2 + n], rerun=out[2 + n], cap=out[3 + n:3 + 2 * n], ok2=out[3 + 2 * n], entries2=out[4 + 2 * n])


def test_the_regions_and_the_rerun(driver, tmp_path):
    r = regions(driver, tmp_path, [64] * 5, [0, 1, 63, 64, 64])
    assert r["ok"] and r["entries"] == 320 and r["base"] == [0, 64, 128, 192, 256] and not r["rerun"] and r["cap"] == [64] * 5
    r = regions(driver, tmp_path, [64] * 5, [0, 1, 65, 64, 300])
    assert r["rerun"] and r["cap"] == [0, 1, 65, 64, 300] and r["ok2"] and r["entries2"] == 430   # exactly the counted sizes
    r = regions(driver, tmp_path, [], [])
    assert r["ok"] and r["entries"] == 0 and not r["rerun"]


def test_the_max_entries_refusal_is_a_pure_function(driver, tmp_path):
    assert regions(driver, tmp_path, [4096] * 4, [0] * 4, 4 * 4096)["ok"] and not regions(driver, tmp_path, [4096] * 4, [0] * 4, 4 * 4096 - 1)["ok"]
    r = regions(driver, tmp_path, [4096] * 2, [MAX_ENTRIES, 1])                                    # the counted sizes pass the limit
    assert r["ok"] and r["rerun"] and not r["ok2"]
    r = regions(driver, tmp_path, [4096] * 2, [MAX_ENTRIES - 1, 1])
    assert r["rerun"] and r["ok2"] and r["entries2"] == MAX_ENTRIES
    assert not regions(driver, tmp_path, [2 ** 63 - 1, 2 ** 63 - 1, 2], [0, 0, 0])["ok"]           # no wrap of the sum
    import re
    with open(os.path.join(ROOT, "include", "qadc.h")) as f:
        assert re.search(r"#define QADC_REFINE_RANGE_MAX_ENTRIES \(1ull << 31\)", f.read())


def test_the_scratch_size_and_the_limit_on_a_calls_whole_result(driver, tmp_path):
    """the radix scratch: as many words as the run's regions where one region exceeds the LDS sort, else none; the held result of a
    call, summed over its passes, stays within QADC_REFINE_RANGE_MAX_ENTRIES rows"""
    U = 2 ** 63 - 1
    rows = [(0, 0, 0, 0, MAX_ENTRIES), (4096, 4096, 0, MAX_ENTRIES, MAX_ENTRIES), (4097, 4097, 0, MAX_ENTRIES + 1, MAX_ENTRIES),
            (10 ** 6, 4096, MAX_ENTRIES - 5, 5, MAX_ENTRIES), (10 ** 6, 4097, MAX_ENTRIES - 5, 6, MAX_ENTRIES), (MAX_ENTRIES, 1, 10, 0, 9),
            (MAX_ENTRIES, MAX_ENTRIES, U, U, U), (5, 5000, 7, 3, 10), (5, 5000, 7, 4, 10)]
    got = run(driver, tmp_path, "sizes", rows).reshape(len(rows), 2).tolist()
    assert got == [[0, 1], [0, 1], [4097, 0], [0, 1], [10 ** 6, 0], [0, 0], [MAX_ENTRIES, 0], [5, 1], [5, 0]]


def test_the_limit_word(driver, tmp_path):
    radii = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1.0, 3.4028234663852886e38], np.float32)
    radii = np.concatenate([radii, np.array([1, 0x007FFFFF, 0x00800000, 0x80000001], np.uint32).view(np.float32)])
    got = run(driver, tmp_path, "limits", radii, np.float32, np.uint64)
    u = radii.view(np.uint32)
    want = np.where((u != 0) & (u <= 0x7F800000), u.astype(np.uint64) << np.uint64(32), np.uint64(0))   # positive and not NaN, by the bits
    assert np.array_equal(got, want) and got[2] == 0x7F800000 << 32 and got[9] == 1 << 32 and (got[[0, 1, 3, 4, 5, 6, 12]] == 0).all()


def test_the_argument_refusals(driver, tmp_path):
    #        call store nq q  rad lims in_lims keys chunk pass
    rows = [(0, 1, 3, 1, 1, 1, 0, 0, 0, 0, False), (0, 0, 3, 1, 1, 1, 0, 0, 0, 0, True), (0, 1, -1, 1, 1, 1, 0, 0, 0, 0, True),
            (0, 1, 3, 0, 1, 1, 0, 0, 0, 0, True), (0, 1, 3, 1, 0, 1, 0, 0, 0, 0, True), (0, 1, 3, 1, 1, 0, 0, 0, 0, 0, True),
            (0, 1, 0, 0, 0, 0, 0, 0, 0, 0, False),
            (1, 1, 3, 1, 1, 1, 1, 1, 0, 0, False), (1, 0, 3, 1, 1, 1, 1, 1, 0, 0, True), (1, 1, -2, 1, 1, 1, 1, 1, 0, 0, True),
            (1, 1, 3, 1, 1, 1, 0, 1, 0, 0, True), (1, 1, 3, 1, 1, 1, 2, 1, 0, 0, True), (1, 1, 3, 1, 1, 1, 3, 1, 0, 0, True),
            (1, 1, 3, 1, 1, 1, 1, 0, 0, 0, True), (1, 1, 3, 1, 1, 1, 4, 0, 0, 0, False), (1, 1, 3, 0, 1, 1, 1, 1, 0, 0, True),
            (1, 1, 3, 1, 0, 1, 1, 1, 0, 0, True), (1, 1, 3, 1, 1, 0, 1, 1, 0, 0, True), (1, 1, 0, 0, 0, 0, 0, 0, 0, 0, False),
            (2, 1, 0, 0, 0, 0, 0, 0, 0, 0, False), (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, True), (2, 1, 0, 0, 0, 0, 0, 0, 1 << 24, 5, False),
            (2, 1, 0, 0, 0, 0, 0, 0, (1 << 24) + 1, 0, True), (2, 1, 0, 0, 0, 0, 0, 0, 0, -1, True)]
    got = run(driver, tmp_path, "refusals", [r[:10] for r in rows])
    assert got.astype(bool).tolist() == [r[10] for r in rows]
