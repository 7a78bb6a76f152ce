"""CPU: the launch geometry of the exhaustive search (quick-adc_amd/host/refine_knn_plan.hpp, driver
tests/cpp/refine_knn_plan_host.cpp).  The launches of qadc_refine_knn do what the header plans and the
kernels index by it, so the header as the library compiles it is held here, over a sweep of (nq, rows, dim, dtype, R, chunk_rows,
pass_nq), to what the kernels rely on: every row is in exactly one (launch, group, slice, wave), every query in exactly one (pass,
tile), a group never appends more than chunk_rows words between two selects, the tile fits its registers or its LDS, every sort is
at most 8192 words, and the scratch is bounded and independent of the rows."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_knn_plan_host")
NAMES = ("qt", "jregs", "dist_lds_bytes", "pass_nq", "passes", "chunk_rows", "groups", "slice_rows", "slices", "launches", "buf_cap",
         "mid_sort_n", "final_sort_n", "select_threads", "select_lds_bytes", "scratch_bytes", "fewest_visits", "most_visits", "most_in_group")
TILES = {(32, 1), (32, 2), (16, 3), (16, 4), (4, 1), (4, 2), (4, 3), (4, 4), (32, 0), (16, 0), (8, 0), (4, 0)}   # the instantiated (QT, J)
REG_BUDGET, LDS_DEFAULT, MAX_SORT, DEFAULT_CHUNK, SCRATCH = 64, 64 * 1024, 8192, 7168, 256 << 20

NQ = (1, 3, 4, 5, 31, 32, 33, 65, 1000, 100000)
DIM = (1, 63, 64, 65, 128, 129, 192, 256, 257, 512, 513, 960, 1024, 1025, 2048, 2049, 4096)
RS = (1, 7, 100, 1023, 1024)
CHUNKS = (0, 1, 64, 100, 7168)
PASSES = (0, 1, 33)
ROWS = (0, 1, 63, 64, 65, 7167, 7168, 7169, 21505, 57344, 57345, 60001)


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def plans(exe, tmp_path, shapes):
    fin, fout = str(tmp_path / "plans.in"), str(tmp_path / "plans.out")
    np.asarray(shapes, np.int64).reshape(-1, 7).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok %d" % len(shapes), out.stderr.decode()
    got = np.fromfile(fout, np.int64).reshape(len(shapes), 20)
    return [None if not g[0] else dict(zip(NAMES, (int(v) for v in g[1:]))) for g in got]


def check(shape, p):
    nq, rows, dim, dtype, R, chunk_rows, pass_nq = shape
    assert p is not None, "an admitted shape is refused: %s" % (shape,)
    chunk = chunk_rows or DEFAULT_CHUNK
    # rows: each in exactly one (launch, group, slice, wave); what a group takes in between two selects fits its buffer
    assert p["fewest_visits"] == 1 and p["most_visits"] == 1, (shape, p)
    assert p["chunk_rows"] == chunk and p["most_in_group"] <= chunk and p["buf_cap"] == R + chunk <= MAX_SORT, (shape, p)
    assert p["launches"] == -(-rows // (p["groups"] * chunk)) and p["slices"] == -(-chunk // p["slice_rows"]), (shape, p)
    assert 1 <= p["groups"] * p["slices"] <= 65535, (shape, p)                                  # the distance grid's second dimension
    # queries: passes of whole queries, tiles of a pass: [0, nq) once
    assert p["pass_nq"] >= 1 and p["passes"] == -(-nq // p["pass_nq"]) and (p["passes"] - 1) * p["pass_nq"] < nq, (shape, p)
    if pass_nq:
        assert p["pass_nq"] == min(nq, pass_nq), (shape, p)
    for n in {p["pass_nq"], nq - (p["passes"] - 1) * p["pass_nq"]}:                           # a full pass and the last one
        tiles = -(-n // p["qt"])                                                               # the distance grid's first dimension
        assert 1 <= n <= p["pass_nq"] and (tiles - 1) * p["qt"] < n <= tiles * p["qt"] and tiles < 2 ** 31, (shape, p)
    # the tile: registers within the budget, or LDS within the default limit
    assert (p["qt"], p["jregs"]) in TILES, (shape, p)
    if p["jregs"]:
        assert p["jregs"] == -(-dim // 64) and p["qt"] * p["jregs"] <= REG_BUDGET and p["dist_lds_bytes"] == 0, (shape, p)
    else:
        assert dim > 256 and p["dist_lds_bytes"] == p["qt"] * dim * 4 <= LDS_DEFAULT, (shape, p)
    # the sorts
    assert p["buf_cap"] <= p["mid_sort_n"] <= MAX_SORT and p["groups"] * R <= p["final_sort_n"] <= MAX_SORT, (shape, p)
    assert p["select_lds_bytes"] == 8 * max(p["mid_sort_n"], p["final_sort_n"]) <= LDS_DEFAULT, (shape, p)
    assert 64 <= p["select_threads"] <= 1024 and p["select_threads"] <= max(p["mid_sort_n"], p["final_sort_n"]), (shape, p)
    # the scratch of a pass: buffers, counters, bounds
    per_query = p["groups"] * (p["buf_cap"] * 8 + 12)
    assert p["scratch_bytes"] == p["pass_nq"] * per_query, (shape, p)
    if not pass_nq:
        assert p["scratch_bytes"] <= max(SCRATCH, per_query), (shape, p)


def test_the_plan_covers_rows_and_queries_once_and_fits_the_chip(driver, tmp_path):
    shapes = [(nq, rows, dim, 0, R, chunk, pass_nq) for nq in NQ for dim in DIM for R in RS for chunk in CHUNKS for pass_nq in PASSES
              for rows in (0, 7169)]
    shapes += [(nq, rows, dim, dtype, R, chunk, 0) for nq in (1, 33, 1000) for dim in (65, 128, 4096) for dtype in (0, 1) for R in (1, 100, 1024)
               for chunk in (0, 64, 100) for rows in ROWS]
    got = plans(driver, tmp_path, shapes)
    for shape, p in zip(shapes, got):
        check(shape, p)
    # the scratch does not depend on the rows, nor on the element type
    by_args = {}
    for shape, p in zip(shapes, got):
        by_args.setdefault((shape[0], shape[2]) + shape[4:], set()).add((p["scratch_bytes"], p["pass_nq"], p["qt"], p["groups"]))
    assert all(len(v) == 1 for v in by_args.values())
    # the sweep reaches what it is there for
    assert {(p["qt"], p["jregs"]) for p in got} == TILES
    assert any(p["passes"] > 1 for p in got) and any(p["launches"] > 1 for p in got) and any(p["groups"] > 1 for p in got)
    assert {p["slice_rows"] for p in got} >= {16, 512}


def test_the_plan_refuses_what_the_kernels_do_not_take(driver, tmp_path):
    bad = [(0, 10, 8, 0, 1, 0, 0), (-1, 10, 8, 0, 1, 0, 0), (1, 10, 0, 0, 1, 0, 0), (1, 10, 4097, 0, 1, 0, 0), (1, 10, 8, 0, 0, 0, 0),
           (1, 10, 8, 0, 1025, 0, 0), (1, 10, 8, 0, 1024, 7169, 0), (1, 10, 8, 0, 2, 8191, 0), (1, 10, 8, 0, 1, 0, -1)]
    assert plans(driver, tmp_path, bad) == [None] * len(bad)
