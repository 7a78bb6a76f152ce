"""CPU: the launch geometry of exact re-ranking (quick-adc_amd/host/refine_plan.hpp, driver tests/cpp/refine_plan_host.cpp).
launch_refine_dist and launch_refine_select launch what the header plans and the kernels index their lists by it, so the header as
the library compiles it is held here, for every (nq, r_in, dim) of a grid, to the invariants the kernels rely on: the candidates
the waves of all workgroups of all passes visit tile [0, nq * r_in) exactly once, the padded sort size is at least r_in and one of
the instantiated ones, and neither kernel asks for more LDS than a CU has (160 KiB)."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_plan_host")
WAVES, IN_FLIGHT = 4, 4                                                # kRefineWaves, kRefineInFlight
NAMES = ("pass_nq", "passes", "cands_per_wg", "chunks", "dist_lds_bytes", "sort_n", "sort_threads", "select_lds_bytes")

NQ = (1, 2, 3, 15, 16, 17, 63, 64, 65, 257, 1024, 2047, 2048, 2049, 4096, 100000, 1 << 24, (1 << 24) + 1)
R_IN = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 100, 255, 256, 257, 400, 511, 512, 513, 1000, 2047, 2048, 2049, 4095, 8191, 8192)
DIM = (1, 63, 64, 65, 96, 128, 960, 4096)


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def plans(exe, tmp_path, shapes):
    fin, fout = str(tmp_path / "plans.in"), str(tmp_path / "plans.out")
    np.asarray(shapes, np.int64).reshape(-1, 3).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok %d" % len(shapes), out.stderr.decode()
    got = np.fromfile(fout, np.int64).reshape(len(shapes), 9)
    return [None if not g[0] else dict(zip(NAMES, (int(v) for v in g[1:]))) for g in got]


def list_cover(r_in, cpw, chunks):
    """how often the waves of a query's `chunks` workgroups visit every candidate of its list, by the kernel's loops: c0 = chunk * cpw,
    c1 = min(r_in, c0 + cpw), for (base = c0 + wave * IN_FLIGHT; base < c1; base += WAVES * IN_FLIGHT) the candidates base + 0 .. 3
    below c1"""
    count = np.zeros(r_in, np.int64)
    for chunk in range(chunks):
        c0 = chunk * cpw
        c1 = min(r_in, c0 + cpw)
        assert c0 < c1, "workgroup %d of %d has no candidate (r_in %d, %d per workgroup)" % (chunk, chunks, r_in, cpw)
        for wave in range(WAVES):
            for base in range(c0 + wave * IN_FLIGHT, c1, WAVES * IN_FLIGHT):
                for i in range(base, min(base + IN_FLIGHT, c1)):
                    count[i] += 1
    return count


def test_the_plan_tiles_the_candidates_and_fits_the_chip(driver, tmp_path):
    shapes = [(nq, r_in, dim) for nq in NQ for r_in in R_IN for dim in DIM]
    seen = set()
    got = plans(driver, tmp_path, shapes)
    for shape, p in zip(shapes, got):
        nq, r_in, dim = shape
        assert p is not None, "an admitted shape is refused: %s" % (shape,)
        # passes of whole queries: [0, nq) once, the scratch of a pass bounded
        assert p["pass_nq"] >= 1 and p["passes"] == -(-nq // p["pass_nq"]) and (p["passes"] - 1) * p["pass_nq"] < nq, (shape, p)
        assert p["pass_nq"] * r_in <= max(r_in, 1 << 24) and p["pass_nq"] * p["chunks"] < 2 ** 31, (shape, p)
        # workgroups of a list
        assert p["cands_per_wg"] % IN_FLIGHT == 0 and IN_FLIGHT <= p["cands_per_wg"] <= 64, (shape, p)
        assert p["chunks"] == -(-r_in // p["cands_per_wg"]), (shape, p)
        key = (r_in, p["cands_per_wg"], p["chunks"])
        if key not in seen:
            seen.add(key)
            assert (list_cover(*key) == 1).all(), (shape, p)
        # LDS and the sort
        assert p["dist_lds_bytes"] == 4 * dim <= 64 * 1024, (shape, p)
        assert p["sort_n"] in (512, 2048, 8192) and p["sort_n"] >= r_in, (shape, p)
        assert all(s < r_in for s in (512, 2048, 8192) if s < p["sort_n"]), "a smaller instantiation would do: %s %s" % (shape, p)
        assert p["sort_threads"] in (256, 1024) and p["sort_n"] % p["sort_threads"] == 0 and p["sort_threads"] <= p["sort_n"] // 2, (shape, p)
        assert p["select_lds_bytes"] == 8 * p["sort_n"] + 4 * p["sort_threads"] <= 160 * 1024, (shape, p)
    # the sweep reaches what it is there for: lists cut finer on small batches, whole chunks on large ones, more than one pass,
    # and the instantiation that needs the raised LDS limit
    assert {p["cands_per_wg"] for p in got} == {4, 8, 16, 32, 64}
    assert any(p["passes"] > 1 for p in got) and any(p["select_lds_bytes"] > 64 * 1024 for p in got)


def test_the_plan_refuses_what_the_kernels_do_not_take(driver, tmp_path):
    bad = [(0, 10, 8), (-1, 10, 8), (1, 0, 8), (1, 8193, 8), (1, 10, 0), (1, 10, 4097)]
    assert plans(driver, tmp_path, bad) == [None] * len(bad)
