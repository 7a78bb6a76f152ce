"""CPU: the geometry of the OPQ cross-matrix kernels (quick-adc_amd/host/opq_plan.hpp; driver tests/cpp/opq_plan_host.cpp) for every
(sq_count, bits, dim <= 1024) the trainers admit: every (a, b) of the matrix is owned by exactly one register of one lane of one
workgroup per block, the register tile and the staged windows fit, the block counts are right around QADC_OPQ_BLOCK."""
import os
import subprocess

import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "opq_plan_host")
SHAPES = [(16, 4), (32, 4), (4, 8), (8, 8), (16, 8)]
BLOCK = 2048


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "opq_plan_host.cpp"), EXE, link=False)
    return EXE


def _parse(line):
    return None if line == "refused" else dict((k, int(x)) for k, x in (t.split("=") for t in line.split()))


def plan(exe, nsq, bits, dim, n):
    out = subprocess.run([exe, "plan", str(nsq), str(bits), str(dim), str(n)], stdout=subprocess.PIPE, timeout=60)
    assert out.returncode == 0
    return _parse(out.stdout.decode().strip())


def test_the_header_and_the_planner_agree_on_the_block():
    hdr = open(os.path.join(ROOT, "include", "qadc.h")).read()
    assert "#define QADC_OPQ_BLOCK 2048" in hdr
    assert "constexpr int kOpqBlock = 2048;" in open(os.path.join(ROOT, "quick-adc_amd", "host", "opq_plan.hpp")).read()


@pytest.mark.parametrize("nsq,bits", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_cell_is_owned_once_and_the_windows_fit(driver, nsq, bits):
    n = 5 * BLOCK + 1
    out = subprocess.run([driver, "sweep", str(nsq), str(bits), str(n)], stdout=subprocess.PIPE, timeout=300)
    assert out.returncode == 0
    lines = out.stdout.decode().splitlines()
    assert len(lines) == 1024 // nsq
    regs = set()
    for k, line in enumerate(lines, 1):
        p = _parse(line.strip())
        dim = nsq * k
        assert p is not None, dim
        assert p["wg"] == 256 == p["lanes"] ** 2 and p["block"] == BLOCK and p["max_dim"] == 1024
        assert p["dim"] == dim and p["dsub"] == k and p["K"] == 1 << bits and p["code_bytes"] == (nsq // 2 if bits == 4 else nsq)
        assert p["reg"] in (1, 2, 4) and p["reg"] ** 2 <= 16                       # chains a lane keeps in registers
        assert p["tile"] == p["lanes"] * p["reg"]
        assert p["tiles"] * p["tile"] >= dim > (p["tiles"] - 1) * p["tile"]
        assert p["reg"] == 4 or p["tiles"] == 1                                    # a small tile only where it covers the matrix
        assert p["stage"] >= 1 and BLOCK % p["stage"] == 0                         # a block is a whole number of steps
        assert (p["stage"] * p["tile"]) % p["wg"] == 0                             # every lane stages the same number of entries
        assert p["lds"] == 2 * 4 * p["stage"] * p["tile"] <= 48 * 1024
        assert p["blocks"] == 6 and p["grid"] == p["blocks"] * p["tiles"] ** 2 < 2 ** 31
        assert p["partial_bytes"] == p["blocks"] * dim * dim * 4
        assert p["reduce_grid"] * p["reduce_wg"] >= dim * dim > (p["reduce_grid"] - 1) * p["reduce_wg"]
        assert p["owned"] == 1, dim
        regs.add(p["reg"])
    assert regs == ({1, 2, 4} if nsq <= 16 else {2, 4})


@pytest.mark.parametrize("n,blocks", [(1, 1), (BLOCK - 1, 1), (BLOCK, 1), (BLOCK + 1, 2), (2 ** 32 - 1, 2 ** 21)])
def test_block_counts(driver, n, blocks):
    for nsq, bits, dim in ((16, 4, 32), (4, 8, 200), (8, 8, 1024)):
        p = plan(driver, nsq, bits, dim, n)
        assert p is not None and p["blocks"] == blocks and p["grid"] == blocks * p["tiles"] ** 2


def test_refusals(driver):
    assert plan(driver, 16, 4, 32, 0) is None and plan(driver, 16, 4, 32, 2 ** 32) is None
    assert plan(driver, 16, 4, 1040, 100) is None and plan(driver, 4, 8, 1028, 100) is None      # dim > 1024
    assert plan(driver, 16, 4, 33, 100) is None and plan(driver, 8, 4, 32, 100) is None and plan(driver, 32, 8, 64, 100) is None
    assert plan(driver, 4, 16, 32, 100) is None and plan(driver, 16, 5, 32, 100) is None
    assert plan(driver, 8, 8, 1024, 100) is not None
