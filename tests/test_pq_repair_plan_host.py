"""CPU: the launch geometry and the scratch of the empty-cluster repair (quick-adc_amd/host/pq_repair_plan.hpp, driver
tests/cpp/pq_repair_plan_host.cpp), swept over every legal (sq_count, sq_bits, dim, n) edge: every code unit and every vector is
owned by exactly one thread, the grids fit the launch limits, the LDS tables fit their budget, the scratch is what include/qadc.h
names (sq_count * n keys of 8 bytes plus the per-centroid tables), and every illegal shape is refused."""
import os
import subprocess

import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "pq_repair_plan_host")
FIELDS = ("n dim sq_count sq_bits dsub K units_per_row unit_bytes units row_blocks unit_blocks count_in_lds count_lds_bytes ctl hist "
          "count first empties blockcnt key total ctl_size").split()
WG, ROW_TILE, UNIT_TILE, MAX_SQ, LDS = 256, 1024, 4096, 32, 32768
EDGE_N = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 70000, 10 ** 6, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def plans():
    _compile(os.path.join(ROOT, "tests", "cpp", "pq_repair_plan_host.cpp"), EXE, link=False)

    def run(shapes):
        text = "".join("%d %d %d %d\n" % s for s in shapes)
        out = subprocess.run([EXE], input=text.encode(), stdout=subprocess.PIPE, check=True, timeout=120).stdout.decode().splitlines()
        assert len(out) == len(shapes)
        return [None if line == "refused" else dict(zip(FIELDS, map(int, line.split()))) for line in out]
    return run


def legal_shapes():
    for bits in (4, 8, 16):
        for nsq in range(1, MAX_SQ + 1):
            if bits == 4 and nsq % 2:
                continue
            for ds in (1, 2, 3, 128):
                for n in EDGE_N:
                    yield n, nsq * ds, nsq, bits


def test_every_legal_shape(plans):
    shapes = list(legal_shapes())
    for (n, dim, nsq, bits), p in zip(shapes, plans(shapes)):
        assert p is not None, (n, dim, nsq, bits)
        assert (p["n"], p["dim"], p["sq_count"], p["sq_bits"]) == (n, dim, nsq, bits)
        K = 1 << bits
        assert p["K"] == K and p["dsub"] * nsq == dim
        upr = nsq // 2 if bits == 4 else nsq
        assert p["units_per_row"] == upr and p["unit_bytes"] == (2 if bits == 16 else 1) and p["units"] == n * upr
        # the row kernels: grid (row_blocks, sq_count); a workgroup owns ROW_TILE vectors, the last one is cut by i < n
        assert (p["row_blocks"] - 1) * ROW_TILE < n <= p["row_blocks"] * ROW_TILE
        assert p["row_blocks"] < 2 ** 31 and nsq <= 65535                   # grid.x and grid.y limits
        # the unit kernels: a workgroup owns UNIT_TILE code units
        assert (p["unit_blocks"] - 1) * UNIT_TILE < p["units"] <= p["unit_blocks"] * UNIT_TILE and p["unit_blocks"] < 2 ** 31
        assert ROW_TILE % WG == 0 and UNIT_TILE % WG == 0
        # the count tables in LDS: both tables of every sub-space, or none
        tables = nsq * K * 2 * 4
        assert p["count_in_lds"] == (tables <= LDS) and p["count_lds_bytes"] == (tables if tables <= LDS else 0)
        # the scratch
        assert p["ctl_size"] == 32 and p["ctl"] == MAX_SQ * p["ctl_size"]
        assert p["hist"] == nsq * 256 * 4 and p["count"] == p["first"] == p["empties"] == nsq * K * 4
        assert p["blockcnt"] == nsq * p["row_blocks"] * 4 and p["key"] == nsq * n * 8
        assert p["total"] == sum(p[k] for k in ("ctl", "hist", "count", "first", "empties", "blockcnt", "key"))


def test_the_trainers_shapes_keep_their_tables_in_lds_at_4_and_8_bits(plans):
    shapes = [(1000, 32, 16, 4), (1000, 64, 32, 4), (1000, 8, 4, 8), (1000, 8, 8, 8), (1000, 16, 16, 8), (1000, 4, 2, 16), (1000, 16, 8, 16)]
    got = plans(shapes)
    assert [p["count_in_lds"] for p in got] == [1, 1, 1, 1, 1, 0, 0]


def test_illegal_shapes_are_refused(plans):
    bad = [(0, 32, 16, 4), (2 ** 32, 32, 16, 4), (10, 32, 16, 5), (10, 32, 16, 0), (10, 32, 16, 32), (10, 33, 16, 4), (10, 0, 16, 4),
           (10, -32, 16, 4), (10, 32, 0, 8), (10, 32, -1, 8), (10, 33, 33, 8), (10, 30, 15, 4), (10, 3, 3, 4), (10, 66, 33, 16)]
    assert plans(bad) == [None] * len(bad)
