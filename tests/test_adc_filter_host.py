"""CPU: the host twin's key filter (host/scanner_simple.hpp key_filter, scanner_simple::set_filter; driver
tests/cpp/adc_filter_host.cpp) — the written definition of qadc_adc_index_set_filter.

A filtered scan must leave the heap the reference's scan leaves on the database from which the dropped rows have been deleted, the
surviving rows' keys given as labels.  The expected arrays are the oracle's on that reduced database (tests/adc_filter_compose.py:
the helpers of the unfiltered GPU tests), compared bit for bit, for one shape of each code width, labelled and unlabelled sources,
both modes, an empty set and the set of every key."""
import os
import subprocess

import numpy as np
import pytest

import adc_filter_compose as fc
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_filter_host")
MODES = {"exclude": 0, "allow": 1, None: -1}


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def run_driver(exe, tmp_path, cases):
    """cases: dicts of shape, parts, labels (None: unlabelled), tables, R, mode, S -> [(keys, vals)]"""
    fin, fout = str(tmp_path / "filter.in"), str(tmp_path / "filter.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            nsq, bits = c["shape"]
            S = np.asarray(c["S"], np.uint32)
            np.array([nsq, bits, len(c["parts"]), c["labels"] is not None, c["R"], 1, MODES[c["mode"]], len(S)], np.int32).tofile(f)
            np.array([len(p) for p in c["parts"]], np.uint32).tofile(f)
            for i, p in enumerate(c["parts"]):
                np.ascontiguousarray(p, "<u2" if bits == 16 else np.uint8).tofile(f)
                if c["labels"] is not None:
                    np.ascontiguousarray(c["labels"][i], np.uint32).tofile(f)
            np.ascontiguousarray(c["tables"], np.float32).tofile(f)
            S.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        for _ in cases:
            n = int(np.fromfile(f, np.int32, 1)[0])
            got.append((np.fromfile(f, np.uint32, n), np.fromfile(f, np.float32, n)))
        assert f.read() == b""
    return got


def sets_of(rng, keys):
    """name -> S over the keys the database holds: random 30 %, with keys no row holds and duplicates; nothing; everything"""
    some = rng.permutation(keys)[:len(keys) * 3 // 10]
    absent = np.array([int(keys.max()) + 1, int(keys.max()) + 1000], np.uint32)
    return {"random": np.concatenate([some, absent, some[:5]]).astype(np.uint32), "empty": np.zeros(0, np.uint32),
            "everything": keys.astype(np.uint32)}


@pytest.mark.parametrize("shape", [(8, 8), (16, 4), (4, 16)], ids=fc.shape_id)
@pytest.mark.parametrize("labelled", [True, False], ids=["labelled", "unlabelled"])
def test_the_twin_with_a_filter_equals_the_oracle_on_the_reduced_database(po, driver, tmp_path, shape, labelled):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + labelled)
    sizes = [700, 0, 1, 1300]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    total = sum(sizes)
    perm = rng.permutation(3 * total)[:total].astype(np.uint32) + np.uint32(50)
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))] if labelled else None
    tables = fc.rand_tables(rng, shape, 1, len(parts))[0]
    held = np.unique(np.concatenate(fc.keys_of(parts, labels)))
    cases, wants = [], []
    for R in (1, 100):
        plain = fc.unfiltered(po, shape, parts, fc.keys_of(parts, labels), tables, R)
        cases.append(dict(shape=shape, parts=parts, labels=labels, tables=tables, R=R, mode=None, S=[]))
        wants.append(("no filter R=%d" % R, plain))
        for name, S in sets_of(rng, held).items():
            for mode in ("exclude", "allow"):
                cases.append(dict(shape=shape, parts=parts, labels=labels, tables=tables, R=R, mode=mode, S=S))
                want = fc.expected(po, shape, parts, labels, tables, R, S, mode)
                wants.append(("%s %s R=%d" % (mode, name, R), want))
                if (name, mode) in (("empty", "exclude"), ("everything", "allow")):      # nothing is dropped: the unfiltered heap
                    assert np.array_equal(want[0], plain[0]) and np.array_equal(want[1].view(np.uint32), plain[1].view(np.uint32))
                elif name != "random":                                                   # everything is dropped: the R sentinels
                    assert np.array_equal(want[0], np.zeros(R, np.uint32)) and (want[1] >= np.float32(3e38)).all()
                elif R == 100:
                    assert not np.array_equal(want[0], plain[0]), "the random set leaves the heap as it was: the case is vacuous"
    for (what, want), got in zip(wants, run_driver(driver, tmp_path, cases)):
        assert len(got[0]) == len(want[0]), what
        assert np.array_equal(got[0], want[0]), what + ": keys differ"
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what + ": values differ"


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(po, tmp_path):
    """the twin and its filter, stand-alone, built with -fsanitize=address,undefined: one labelled case of each width and an empty
    set, no report, the same heaps"""
    exe = str(tmp_path / "adc_filter_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(8)
    cases, wants = [], []
    for shape in [(8, 8), (16, 4), (4, 16)]:
        parts = [fc.rand_codes(rng, shape, n) for n in (300, 0, 77)]
        labels = [np.arange(300, dtype=np.uint32) * 3, np.zeros(0, np.uint32), (np.arange(77, dtype=np.uint64) + (2 ** 32 - 77)).astype(np.uint32)]
        tables = fc.rand_tables(rng, shape, 1, 3)[0]
        for mode, S in (("exclude", np.arange(0, 900, 6)), ("allow", np.array([2 ** 32 - 1, 3, 3, 5])), ("allow", [])):
            cases.append(dict(shape=shape, parts=parts, labels=labels, tables=tables, R=10, mode=mode, S=S))
            wants.append(fc.expected(po, shape, parts, labels, tables, 10, S, mode))
    for want, got in zip(wants, run_driver(exe, tmp_path, cases)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
