"""CPU: the 16-bit code shapes (2,16) (4,16) (8,16) of the float-ADC path, pinned to the reference.

tests/golden/ref_scan_standard_u16_cases.npz holds the heaps the reference's own scanner_simple + scan_standard<uint16_t, NSQ>
leave, as g++ compiles them with the reference's flags (tools/gen_golden_adc16.py).  Against it:
1. the host twin (host/scanner_simple.hpp, driver tests/cpp/scan_standard16_host.cpp) under float_sum_mode() == 1, bit for bit;
2. the composition of tests/adc16_compose.py, the oracle of the GPU tests (tests/test_gpu_adc16*.py)."""
import os
import subprocess

import numpy as np
import pytest

import adc16_compose as a16
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "scan_standard16_host")


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def run_driver(exe, tmp_path, c, sum_mode):
    fin, fout = str(tmp_path / "case.in"), str(tmp_path / "case.out")
    with open(fin, "wb") as f:
        np.array([c["nsq"], len(c["parts"]), c["labelled"], c["R"], sum_mode], np.int32).tofile(f)
        np.array([len(p) for p in c["parts"]], np.uint32).tofile(f)
        for i, p in enumerate(c["parts"]):
            np.ascontiguousarray(p, "<u2").tofile(f)
            if c["labelled"]:
                np.ascontiguousarray(c["labels"][i], np.uint32).tofile(f)
        np.ascontiguousarray(c["tables"], np.float32).tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    with open(fout, "rb") as f:
        n = int(np.fromfile(f, np.int32, 1)[0])
        keys, vals = np.fromfile(f, np.uint32, n), np.fromfile(f, np.float32, n)
        assert f.read() == b""
    return keys, vals


def same(got, c):
    return len(got[0]) == c["R"] and np.array_equal(got[0], c["keys"]) and \
        np.array_equal(got[1].view(np.uint32), c["vals"].view(np.uint32))


def test_the_fixture_covers_what_it_is_for():
    cases = a16.fixture()
    assert {(c["nsq"], c["kind"], c["labelled"], c["R"]) for c in cases} == \
        {(n, k, l, r) for n in (2, 4, 8) for k in ("mixed", "ties", "negzero") for l in (False, True) for r in (1, 7, 100)}
    assert "g++" in cases[0]["compiler"]
    for c in cases:
        codes = np.concatenate(c["parts"])
        assert len(codes) == 1000 and codes.dtype == np.uint16
        for m in range(c["nsq"]):
            assert set(a16.SPECIAL) <= set(codes[:, m].tolist())
        t = a16.gather(c["nsq"], c["parts"][0], c["tables"][0])
        assert (t.view(np.uint32) == 0x80000000).any()                               # -0.0 among the entries the codes read
        if c["kind"] == "mixed":
            assert (t < 0).any() and (t > 0).any()
            e = np.frexp(t[t != 0])[1]
            assert int(e.max()) - int(e.min()) >= 20                                 # binades
        if c["kind"] == "negzero":
            assert (c["vals"].view(np.uint32)[:min(c["R"], 1000)] == 0x80000000).all()   # no leading "0 +" in any shape


@pytest.mark.parametrize("nsq", [2, 4, 8])
def test_host_twin_scan_standard_u16_reproduces_the_reference(driver, tmp_path, nsq):
    cases = [c for c in a16.fixture() if c["nsq"] == nsq]
    assert len(cases) == 18
    for c in cases:
        assert same(run_driver(driver, tmp_path, c, 1), c), c["cid"]


def test_host_twin_source_order_is_another_sum(po, driver, tmp_path):
    """float_sum_mode() == 0 keeps the sequential sum from +0: on the mixed tables it does not reproduce the reference as compiled"""
    for nsq in (4, 8):
        c = next(c for c in a16.fixture() if c["nsq"] == nsq and c["kind"] == "mixed" and c["R"] == 100 and not c["labelled"])
        got = run_driver(driver, tmp_path, c, 0)
        assert not same(got, c)
        want = a16.heap(po, c["nsq"], c["parts"], None, c["tables"], c["R"], 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_the_composition_reproduces_the_reference(po):
    for c in a16.fixture():
        want = a16.heap(po, c["nsq"], c["parts"], c["labels"], c["tables"], c["R"], 1)
        assert same(want, c), c["cid"]
