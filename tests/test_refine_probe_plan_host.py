"""CPU: the launch geometry of the probed exact search (quick-adc_amd/host/refine_probe_plan.hpp, driver
tests/cpp/refine_probe_plan_host.cpp).  The launches of qadc_refine_knn_probed do what the header plans and
the kernels index by it, so the header as the library compiles it is held here, over a sweep of probe lists, partition sizes, dims,
R, chunk_rows and pass_nq, to what the kernels rely on: every (query, probed partition, row) lies in exactly one (launch, item, wave
slot) and nothing else does; between two selects a (query, group) buffer is offered at most chunk_rows rows; grid.y is at most 65535;
the scratch does not depend on the rows; and a refusal is a refusal, not a bad plan."""
import subprocess

import numpy as np
import pytest

import refine_probe_cases as pc

NAMES = ("qt", "jregs", "dist_lds_bytes", "pass_nq", "passes", "chunk_rows", "groups", "per_group", "launch_rows", "buf_cap", "mid_sort_n",
         "final_sort_n", "select_threads", "select_lds_bytes", "scratch_bytes", "visits", "repeats", "strays", "most_offered", "most_y",
         "most_items", "most_slots", "launches")
TILES = {(32, 1), (32, 2), (16, 3), (16, 4), (4, 1), (4, 2), (4, 3), (4, 4), (32, 0), (16, 0), (8, 0), (4, 0)}   # the instantiated (QT, J)
MAX_SORT, DEFAULT_CHUNK, LDS_DEFAULT, ITEM_BYTES = 8192, 7168, 64 * 1024, 16
BUDGET = 1500000                 # (query, partition, row) triples of a scenario, about


@pytest.fixture(scope="module")
def driver():
    return pc.build_plan_driver()


def plans(exe, tmp_path, scenarios):
    fin, fout = str(tmp_path / "plans.in"), str(tmp_path / "plans.out")
    with open(fin, "wb") as f:
        for (nq, K, ma, dim, R, chunk, pass_nq), sizes, assign in scenarios:
            np.array([nq, K, ma, dim, R, chunk, pass_nq], np.int64).tofile(f)
            np.asarray(sizes, np.int64).tofile(f)
            np.asarray(assign, np.int64).tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok %d" % len(scenarios), (out.returncode, out.stderr.decode())
    got = np.fromfile(fout, np.int64).reshape(len(scenarios), 24)
    return [None if not g[0] else dict(zip(NAMES, (int(v) for v in g[1:]))) for g in got]


def sizes_of(rng, K, kind, mean):
    if kind == "even":
        return np.full(K, mean, np.int64)
    if kind == "skewed":                                                     # a few long partitions, many short ones, empty ones
        s = (rng.pareto(1.0, K) * mean / 3).astype(np.int64)
        s[rng.random(K) < 0.3] = 0
        return np.minimum(s, 40 * mean + 1)
    s = np.zeros(K, np.int64)                                                # one partition holds everything
    s[rng.integers(K)] = mean * K
    return s


def assign_of(rng, nq, ma, K, kind):
    if kind == "distinct":
        return np.stack([rng.permutation(K)[:ma] for _ in range(nq)])
    if kind == "hot":                                                        # every query probes partition 0 first
        a = np.stack([rng.permutation(K)[:ma] for _ in range(nq)])
        a[:, 0] = 0
        return a
    return rng.integers(-2, K + 2, (nq, ma))                                 # repeats, and numbers that are no partition


def expected_visits(sizes, assign):
    K = len(sizes)
    return sum(int(sum(sizes[p] for p in set(int(x) for x in row) if 0 <= p < K)) for row in assign)


def check(args, sizes, assign, p):
    nq, K, ma, dim, R, chunk_rows, pass_nq = args
    chunk = chunk_rows or DEFAULT_CHUNK
    assert p["groups"] == max(1, min(8, MAX_SORT // R, ma)) and p["per_group"] == -(-ma // p["groups"]), (args, p)
    assert p["chunk_rows"] == chunk and p["launch_rows"] == chunk // p["per_group"] >= 1 and p["buf_cap"] == R + chunk <= MAX_SORT, (args, p)
    # every (query, probed partition, row) once, and nothing else
    assert p["visits"] == expected_visits(sizes, assign) and p["repeats"] == 0 and p["strays"] == 0, (args, p)
    # the invariant of the selection, and the grid
    assert p["most_offered"] <= chunk and p["most_y"] <= 65535, (args, p)
    longest = max([int(sizes[x]) for row in assign for x in row if 0 <= x < K] + [0])
    per_pass = -(-longest // p["launch_rows"])
    assert p["launches"] <= p["passes"] * per_pass, (args, p)
    # queries and tiles
    assert p["pass_nq"] >= 1 and p["passes"] == -(-nq // p["pass_nq"]), (args, p)
    if pass_nq:
        assert p["pass_nq"] == min(nq, pass_nq), (args, p)
    assert (p["qt"], p["jregs"]) in TILES and p["dist_lds_bytes"] == (0 if p["jregs"] else p["qt"] * dim * 4) <= LDS_DEFAULT, (args, p)
    # sorts and scratch
    assert p["buf_cap"] <= p["mid_sort_n"] <= MAX_SORT and p["groups"] * R <= p["final_sort_n"] <= MAX_SORT, (args, p)
    sort_n = max(p["mid_sort_n"], p["final_sort_n"])
    assert p["select_lds_bytes"] == 8 * sort_n <= LDS_DEFAULT and 64 <= p["select_threads"] <= 1024, (args, p)
    assert sort_n <= 8 * p["select_threads"] and 4 * p["select_threads"] <= p["select_lds_bytes"], (args, p)   # probe_distinct's segments and scan
    assert p["most_items"] <= p["pass_nq"] * ma and p["most_slots"] <= p["pass_nq"] * ma, (args, p)
    assert p["scratch_bytes"] == p["pass_nq"] * (p["groups"] * (p["buf_cap"] * 8 + 12) + ma * (ITEM_BYTES + 4)), (args, p)


def test_the_plan_covers_every_probed_row_once_and_keeps_the_selects_invariant(driver, tmp_path):
    rng = np.random.default_rng(2024)
    scenarios = []
    for nq in (1, 3, 4, 5, 31, 32, 33, 65, 257, 2049):
        for K in (1, 2, 5, 33, 300):
            for ma in sorted({1, min(2, K), min(9, K), (K + 1) // 2, K}):
                for kind in ("even", "skewed", "one"):
                    mean = max(1, min(4000, BUDGET // (nq * ma)))
                    sizes = sizes_of(rng, K, kind, mean if kind != "one" else max(1, mean // K))
                    dim = int(rng.choice((1, 63, 64, 65, 128, 129, 256, 257, 1024, 4096)))
                    R = int(rng.choice((1, 7, 100, 1023, 1024)))
                    per_group = -(-ma // max(1, min(8, MAX_SORT // R, ma)))
                    chunk = int(rng.choice([c for c in (0, 1, 64, 100, 1000, 7168) if (c or DEFAULT_CHUNK) >= per_group and (c or DEFAULT_CHUNK) + R <= MAX_SORT]))
                    pass_nq = int(rng.choice((0, 0, 1, 3, 33)))
                    assign = assign_of(rng, nq, ma, K, str(rng.choice(("distinct", "hot", "wild"))))
                    if chunk and chunk // per_group < 8 and kind != "even":           # (thin launches: keep the walk short)
                        sizes = np.minimum(sizes, 300)
                    scenarios.append(((nq, K, ma, dim, R, chunk, pass_nq), sizes, assign))
    got = plans(driver, tmp_path, scenarios)
    for (args, sizes, assign), p in zip(scenarios, got):
        assert p is not None, "an admitted shape is refused: %s" % (args,)
        check(args, sizes, assign, p)
    # the sweep reaches what it is there for
    assert {(p["qt"], p["jregs"]) for p in got} >= {(32, 1), (32, 2), (16, 4), (4, 1), (4, 0), (32, 0)}
    assert any(p["passes"] > 1 for p in got) and any(p["launches"] > p["passes"] for p in got) and any(p["per_group"] > 1 for p in got)
    assert any(p["visits"] == 0 for p in got) and max(p["most_offered"] for p in got) > 1000


def test_the_scratch_does_not_depend_on_the_rows(driver, tmp_path):
    rng = np.random.default_rng(5)
    scenarios = []
    for nq, K, ma, dim, R, chunk, pass_nq in ((65, 33, 9, 128, 100, 0, 0), (1000, 5, 5, 4096, 1024, 64, 0), (33, 300, 300, 65, 7, 100, 3)):
        assign = assign_of(rng, nq, ma, K, "distinct")
        for mean in (0, 1, 50, 900):
            scenarios.append(((nq, K, ma, dim, R, chunk, pass_nq), sizes_of(rng, K, "even", mean), assign))
    got = plans(driver, tmp_path, scenarios)
    fixed = NAMES[:15]
    for i in range(0, len(got), 4):
        assert all(p is not None for p in got[i:i + 4])
        assert len({tuple(p[k] for k in fixed) for p in got[i:i + 4]}) == 1


def test_the_plan_refuses_what_the_kernels_do_not_take(driver, tmp_path):
    def scen(nq, K, ma, dim, R, chunk, pass_nq):
        return ((nq, K, ma, dim, R, chunk, pass_nq), np.ones(max(K, 0), np.int64), np.zeros((max(nq, 0), max(ma, 0)), np.int64))
    bad = [scen(0, 5, 1, 8, 1, 0, 0), scen(1, 5, 0, 8, 1, 0, 0), scen(1, 5, 1, 0, 1, 0, 0), scen(1, 5, 1, 4097, 1, 0, 0), scen(1, 5, 1, 8, 0, 0, 0),
           scen(1, 5, 1, 8, 1025, 0, 0), scen(1, 5, 1, 8, 1024, 7169, 0), scen(1, 5, 1, 8, 1, 0, -1),
           scen(1, 40, 9, 8, 1, 1, 0),            # nine probes in eight groups: two share a group, and a chunk of one row cannot hold both
           scen(1, 40, 40, 8, 1024, 4, 0)]        # forty probes in eight groups of five
    assert plans(driver, tmp_path, bad) == [None] * len(bad)
    ok = [scen(1, 40, 8, 8, 1, 1, 0), scen(1, 40, 40, 8, 1024, 5, 0)]
    assert all(p is not None and p["launch_rows"] == 1 for p in plans(driver, tmp_path, ok))
