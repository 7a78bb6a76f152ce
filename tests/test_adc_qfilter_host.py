"""CPU: the host twin under two composed key filters (host/scanner_simple.hpp: key_filter::also, scanner_simple::set_query_filter;
driver tests/cpp/adc_qfilter_host.cpp) — the written definition of the qadc_adc_*_filtered calls.

A row is emitted iff it passes the index's filter and its query's.  The expected arrays are the oracle's on the database reduced by
the first filter and then by the second (tests/adc_filter_compose.py, the surviving keys given as labels), compared bit for bit, for
one shape of each code width, all four mode pairs and empty sets; with the second filter absent the twin must return what the
one-filter twin of tests/cpp/adc_filter_host.cpp returns."""
import os
import subprocess

import numpy as np
import pytest

import adc_filter_compose as fc
import test_adc_filter_host as one
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_qfilter_host")
MODES = one.MODES


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


@pytest.fixture(scope="module")
def one_filter_driver():
    _compile(one.EXE + ".cpp", one.EXE, link=False)
    return one.EXE


def run_driver(exe, tmp_path, cases):
    """cases: dicts of shape, parts, labels (None: unlabelled), tables, R, first = (mode, S), second = (mode, S) -> [(keys, vals)]"""
    fin, fout = str(tmp_path / "qfilter.in"), str(tmp_path / "qfilter.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            nsq, bits = c["shape"]
            (m1, S1), (m2, S2) = c["first"], c["second"]
            S1, S2 = np.asarray(S1, np.uint32), np.asarray(S2, np.uint32)
            np.array([nsq, bits, len(c["parts"]), c["labels"] is not None, c["R"], 1, MODES[m1], len(S1), MODES[m2], len(S2)],
                     np.int32).tofile(f)
            np.array([len(p) for p in c["parts"]], np.uint32).tofile(f)
            for i, p in enumerate(c["parts"]):
                np.ascontiguousarray(p, "<u2" if bits == 16 else np.uint8).tofile(f)
                if c["labels"] is not None:
                    np.ascontiguousarray(c["labels"][i], np.uint32).tofile(f)
            np.ascontiguousarray(c["tables"], np.float32).tofile(f)
            S1.tofile(f)
            S2.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        for _ in cases:
            n = int(np.fromfile(f, np.int32, 1)[0])
            got.append((np.fromfile(f, np.uint32, n), np.fromfile(f, np.float32, n)))
        assert f.read() == b""
    return got


def expected_both(po, shape, parts, labels, tables, R, first, second):
    """the oracle on the database reduced by `first` = (mode, S), then by `second`; a mode of None reduces nothing"""
    keys = fc.keys_of(parts, labels)
    for mode, S in (first, second):
        if mode is not None:
            parts, keys = fc.reduce(parts, keys, S, mode)
    return fc.unfiltered(po, shape, parts, keys, tables, R)


def same(a, b):
    return len(a[0]) == len(b[0]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def database(rng, shape, labelled):
    sizes = [700, 0, 1, 1300]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    total = sum(sizes)
    perm = rng.permutation(3 * total)[:total].astype(np.uint32) + np.uint32(50)
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))] if labelled else None
    tables = fc.rand_tables(rng, shape, 1, len(parts))[0]
    return parts, labels, tables, np.unique(np.concatenate(fc.keys_of(parts, labels)))


@pytest.mark.parametrize("shape", [(8, 8), (16, 4), (4, 16)], ids=fc.shape_id)
@pytest.mark.parametrize("labelled", [True, False], ids=["labelled", "unlabelled"])
def test_the_twin_under_two_filters_equals_the_oracle_on_the_database_reduced_by_both(po, driver, tmp_path, shape, labelled):
    rng = np.random.default_rng(2000 * shape[0] + shape[1] + labelled)
    parts, labels, tables, held = database(rng, shape, labelled)
    A = rng.permutation(held)[:len(held) * 4 // 10].astype(np.uint32)          # two overlapping sets over the keys the database holds
    B = np.concatenate([A[:len(A) // 2], rng.permutation(held)[:len(held) * 3 // 10], [held.max() + 7]]).astype(np.uint32)
    empty = np.zeros(0, np.uint32)
    cases, wants = [], []
    for R in (1, 100):
        plain = fc.unfiltered(po, shape, parts, fc.keys_of(parts, labels), tables, R)
        pairs = [((m1, A), (m2, B)) for m1 in ("exclude", "allow") for m2 in ("exclude", "allow")]          # all four mode pairs
        pairs += [((m1, S1), (m2, S2)) for m1, S1, m2, S2 in (("exclude", empty, "exclude", empty), ("exclude", empty, "allow", B),
                                                              ("allow", A, "exclude", empty), ("allow", empty, "exclude", B),
                                                              ("exclude", A, "allow", empty), ("allow", empty, "allow", empty))]
        for first, second in pairs:
            cases.append(dict(shape=shape, parts=parts, labels=labels, tables=tables, R=R, first=first, second=second))
            want = expected_both(po, shape, parts, labels, tables, R, first, second)
            what = "%s[%d] then %s[%d] R=%d" % (first[0], len(first[1]), second[0], len(second[1]), R)
            wants.append((what, want))
            if (first[0], second[0]) == ("exclude", "exclude") and not len(first[1]) and not len(second[1]):
                assert same(want, plain), "two EXCLUDEs of nothing drop nothing"
            elif any(mode == "allow" and not len(S) for mode, S in (first, second)):
                assert np.array_equal(want[0], np.zeros(R, np.uint32)) and (want[1] >= np.float32(3e38)).all()   # ALLOW of nothing: the sentinels
            elif R == 100 and len(first[1]) and len(second[1]):
                for alone in (first, second):                    # neither filter alone gives this heap: the case needs both applied
                    assert not same(want, expected_both(po, shape, parts, labels, tables, R, alone, (None, empty))), what + ": vacuous"
    for (what, want), got in zip(wants, run_driver(driver, tmp_path, cases)):
        assert len(got[0]) == len(want[0]), what
        assert np.array_equal(got[0], want[0]), what + ": keys differ"
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what + ": values differ"


@pytest.mark.parametrize("shape", [(8, 8), (16, 4), (4, 16)], ids=fc.shape_id)
def test_with_the_second_filter_absent_the_twin_is_the_one_filter_twin(po, driver, one_filter_driver, tmp_path, shape):
    """first filter only, second filter only (the same heap: one filter is one filter wherever it is set), and none"""
    rng = np.random.default_rng(77 + shape[0])
    parts, labels, tables, held = database(rng, shape, True)
    S = rng.permutation(held)[:len(held) // 3].astype(np.uint32)
    none = (None, np.zeros(0, np.uint32))
    two, single = [], []
    for R in (1, 100):
        for mode in ("exclude", "allow", None):
            base = dict(shape=shape, parts=parts, labels=labels, tables=tables, R=R)
            single.append(dict(base, mode=mode, S=S if mode else []))
            two.append((dict(base, first=(mode, S if mode else []), second=none), dict(base, first=none, second=(mode, S if mode else []))))
    want = one.run_driver(one_filter_driver, tmp_path, single)
    got_first = run_driver(driver, tmp_path, [a for a, _ in two])
    got_second = run_driver(driver, tmp_path, [b for _, b in two])
    for i, c in enumerate(single):
        what = "%s R=%d" % (c["mode"], c["R"])
        assert same(got_first[i], want[i]), what + ": the index's filter alone"
        assert same(got_second[i], want[i]), what + ": the query's filter alone"
        assert same(want[i], fc.expected(po, shape, parts, labels, tables, c["R"], c["S"], c["mode"]) if c["mode"] else
                    fc.unfiltered(po, shape, parts, labels, tables, c["R"])), what


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(po, tmp_path):
    """the twin and its chained filters, stand-alone, built with -fsanitize=address,undefined: no report, the same heaps"""
    exe = str(tmp_path / "adc_qfilter_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(9)
    cases, wants = [], []
    for shape in [(8, 8), (16, 4), (4, 16)]:
        parts = [fc.rand_codes(rng, shape, n) for n in (300, 0, 77)]
        labels = [np.arange(300, dtype=np.uint32) * 3, np.zeros(0, np.uint32), (np.arange(77, dtype=np.uint64) + (2 ** 32 - 77)).astype(np.uint32)]
        tables = fc.rand_tables(rng, shape, 1, 3)[0]
        for first, second in ((("exclude", np.arange(0, 900, 6)), ("allow", np.arange(0, 900, 9))),
                              (("allow", np.array([2 ** 32 - 1, 3, 3, 5])), ("exclude", np.array([3]))),
                              ((None, []), ("allow", [])), (("exclude", []), (None, []))):
            cases.append(dict(shape=shape, parts=parts, labels=labels, tables=tables, R=10, first=first, second=second))
            wants.append(expected_both(po, shape, parts, labels, tables, 10, first, second))
    for want, got in zip(wants, run_driver(exe, tmp_path, cases)):
        assert same(got, want)
