"""CPU: the host twin's range search (host/scanner_simple.hpp: scanner_simple::range_scan over range_standard / range_4f; driver
tests/cpp/adc_range_host.cpp) — the written definition of the qadc_adc_range_* calls — against the numpy
restatement tests/adc_range_cases.py, keys and value bit patterns compared exactly.

Shapes 8x8, 16x4 (nibbles) and 4x16; labelled and unlabelled partitions; all four filter mode pairs and empty filter sets; the radii
NaN, -inf, +inf, FLT_MAX, a value present in the data (the strict compare excludes it) and its nextafter (which includes it); tables
holding NaN, +inf, -0 and +0; and the cases tests/test_gpu_adc_range_edges.py runs on the device (digit_case, signed_case, nonfinite_case), so that
the twin is held to the restatement on them before a GPU is."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adc_filter_compose as fc
import adc_range_cases as rc
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_range_host")
MODES = {"exclude": 0, "allow": 1, None: -1}
SHAPES = [(8, 8), (16, 4), (4, 16)]
FLT_MAX = np.float32(np.finfo(np.float32).max)
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def run_driver(exe, tmp_path, cases):
    """cases: dicts of shape, parts, labels (None: unlabelled), tables, radius, first = (mode, S), second = (mode, S), sum_mode"""
    fin, fout = str(tmp_path / "range.in"), str(tmp_path / "range.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            nsq, bits = c["shape"]
            (m1, S1), (m2, S2) = c.get("first", (None, [])), c.get("second", (None, []))
            S1, S2 = np.asarray(S1, np.uint32), np.asarray(S2, np.uint32)
            rbits = int(np.array([c["radius"]], np.float32).view(np.int32)[0])
            np.array([nsq, bits, len(c["parts"]), c["labels"] is not None, rbits, c.get("sum_mode", 1), MODES[m1], len(S1), MODES[m2], len(S2)],
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


def want_of(c):
    filters = [None if m is None else (S, m) for m, S in (c.get("first", (None, [])), c.get("second", (None, [])))]
    return rc.expected(c["shape"], c["parts"], c["labels"], c["tables"], c["radius"], filters, c.get("sum_mode", 1))


def check(exe, tmp_path, cases):
    got = run_driver(exe, tmp_path, cases)
    for c, g in zip(cases, got):
        w = want_of(c)
        what = "%s radius %r %s %s" % (fc.shape_id(c["shape"]), c["radius"], c.get("first", ""), c.get("second", ""))
        assert len(g[0]) == len(w[0]), "%s: %d rows, expected %d" % (what, len(g[0]), len(w[0]))
        assert np.array_equal(g[0], w[0]), what + ": keys differ"
        assert np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)), what + ": values differ"
    return got


def database(rng, shape, labelled, quarter=False):
    sizes = [700, 0, 1, 1300]
    parts = [fc.rand_codes(rng, shape, n) for n in sizes]
    total = sum(sizes)
    perm = rng.permutation(3 * total)[:total].astype(np.uint32) + np.uint32(50)
    labels = [perm[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))] if labelled else None
    tables = (rc.quarter_tables if quarter else fc.rand_tables)(rng, shape, 1, len(parts))[0]
    return parts, labels, tables


def all_candidates(shape, parts, tables, sum_mode=1):
    return np.concatenate([rc.candidates(shape, p, tables[a], sum_mode) for a, p in enumerate(parts)])


@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
@pytest.mark.parametrize("labelled", [True, False], ids=["labelled", "unlabelled"])
def test_the_twin_equals_the_restatement_at_every_radius(driver, tmp_path, shape, labelled):
    rng = np.random.default_rng(3000 * shape[0] + shape[1] + labelled)
    parts, labels, tables = database(rng, shape, labelled)
    v = np.sort(all_candidates(shape, parts, tables))
    present = v[len(v) // 10]
    cases = [dict(shape=shape, parts=parts, labels=labels, tables=tables, radius=r, sum_mode=sm)
             for sm in (1, 0) for r in (np.float32(np.nan), -INF, INF, FLT_MAX, present, np.nextafter(present, INF), v[0], np.float32(0))]
    got = check(driver, tmp_path, cases)
    n = len(v)
    assert [len(g[0]) for g in got[:7]] == [0, 0, n, n, int((v < present).sum()), int((v <= present).sum()), 0], "the radii do not cut where they are meant to"
    assert len(got[5][0]) > len(got[4][0]), "nextafter of a present value includes it"
    for g in got:                                                # ascending by (candidate, key)
        w = rc.words(g[0], g[1])
        assert (w[1:] >= w[:-1]).all()


@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
@pytest.mark.parametrize("labelled", [True, False], ids=["labelled", "unlabelled"])
def test_the_twin_under_both_filters_all_mode_pairs_and_empty_sets(driver, tmp_path, shape, labelled):
    rng = np.random.default_rng(4000 * shape[0] + shape[1] + labelled)
    parts, labels, tables = database(rng, shape, labelled)
    held = np.unique(np.concatenate(fc.keys_of(parts, labels)))
    A = rng.permutation(held)[:len(held) * 4 // 10].astype(np.uint32)
    B = np.concatenate([A[:len(A) // 2], rng.permutation(held)[:len(held) * 3 // 10], [held.max() + 7]]).astype(np.uint32)
    empty = np.zeros(0, np.uint32)
    v = np.sort(all_candidates(shape, parts, tables))
    pairs = [((m1, A), (m2, B)) for m1 in ("exclude", "allow") for m2 in ("exclude", "allow")]
    pairs += [(("exclude", empty), ("exclude", empty)), (("exclude", empty), ("allow", B)), (("allow", A), ("exclude", empty)),
              (("allow", empty), ("exclude", B)), (("exclude", A), ("allow", empty)), (("allow", empty), ("allow", empty)),
              ((None, empty), ("allow", B)), (("exclude", A), (None, empty))]
    cases = [dict(shape=shape, parts=parts, labels=labels, tables=tables, radius=r, first=f, second=s)
             for r in (v[len(v) // 2], INF) for f, s in pairs]
    got = check(driver, tmp_path, cases)
    base = len(pairs)
    assert len(got[base + 4][0]) == len(v), "two EXCLUDEs of nothing under radius +inf keep every row"
    assert all(len(got[base + i][0]) == 0 for i in (7, 8, 9)), "an ALLOW of nothing keeps nothing"
    sizes = [len(got[base + i][0]) for i in range(4)]
    assert len(set(sizes)) == 4 and 0 < min(sizes), "the four mode pairs keep four different row counts: %s" % sizes


@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_tables_with_nan_inf_and_signed_zeros_and_tied_rows(driver, tmp_path, shape):
    """NaN and +inf candidates are never kept (+inf not even under radius +inf); -0 sorts before +0; rows with the same key and the
    same candidate are all present"""
    nsq, bits = shape
    rng = np.random.default_rng(5000 + shape[0])
    parts, _, tables = database(rng, shape, True, quarter=True)
    labels = [rng.integers(0, 40, len(p)).astype(np.uint32) for p in parts]     # few keys, few sums: equal (key, candidate) rows abound
    tables = tables.reshape(len(parts), nsq, 1 << bits).copy()
    tables[0, :, :] = np.float32(0.0)                           # partition 0 sums signed zeros: -0 for the rows whose every digit is 0
    tables[0, :, 0] = np.float32(-0.0)
    parts[0][:350] = 0
    tables[3, 0, ::5] = np.nan
    tables[3, 1, 1::5] = np.inf
    tables[3, 2, 2::7] = -np.inf
    tables = tables.reshape(len(parts), -1)
    v = all_candidates(shape, parts, tables)
    assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
    zeros = v[v == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all(), "both zeros occur among the candidates"
    cases = [dict(shape=shape, parts=parts, labels=labels, tables=tables, radius=r, sum_mode=sm)
             for sm in (1, 0) for r in (INF, FLT_MAX, np.float32(0.0), np.float32(-0.0), rc.TINY, np.float32(2.0), np.float32(np.nan))]
    got = check(driver, tmp_path, cases)
    keys, vals = got[0]
    assert len(keys) == int((v < INF).sum()) and not np.isnan(vals).any() and not np.isposinf(vals).any()
    w = rc.words(keys, vals)
    assert (w[1:] == w[:-1]).any(), "no two rows share key and candidate: the case is vacuous"
    sign = np.signbit(vals[vals == 0])
    assert sign.any() and not sign.all() and (sign[:-1] >= sign[1:]).all(), "every -0 sorts before every +0"
    assert np.array_equal(got[2][0], got[3][0]), "radius +0 and -0 compare alike"
    assert len(got[2][0]) and (got[2][1] < 0).all(), "radius 0 keeps the negative candidates and neither zero"


# ---- the builders the GPU edge tests share: the twin on their inputs -------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_the_twin_on_segments_that_differ_in_chosen_sort_digits(driver, tmp_path, shape):
    """every mask, at the length that takes the device's radix passes and at the one that sorts in LDS, under both groupings"""
    cases = [c for mask in rc.DIGIT_MASKS for n in (6000, 3000) for sm in (1, 0) for c in rc.queries_of(rc.digit_case(shape, mask, n), sm)]
    got = check(driver, tmp_path, cases)
    assert [len(g[0]) for g in got] == [6000, 6000, 3000, 3000] * len(rc.DIGIT_MASKS), "radius +inf keeps every row"
    masks = [rc.active_digits(rc.words(g[0], g[1])) for g in got[::4]]
    assert masks == rc.DIGIT_MASKS, "the twin's own rows differ in the digits %s" % [hex(m) for m in masks]


@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_the_twin_on_candidates_of_both_signs_signed_zeros_and_subnormals(driver, tmp_path, shape):
    case = rc.signed_case(shape)
    got = check(driver, tmp_path, rc.queries_of(case, 1) + rc.queries_of(case, 0))
    assert len(got[0][0]) > rc.RANGE_SORT_LDS > len(got[1][0])
    for keys, vals in got[:3]:                                   # sum_mode 1: the all -0 row before the all +0 row of the same label
        twins = vals[(vals.view(np.uint32) << 1 == 0) & (keys == rc.SIGNED_TWIN)]   # (bits: a process may compare subnormals equal to 0)
        assert list(np.signbit(twins)) == [True, False]
        assert (vals[:-1] <= vals[1:]).all() and vals[0] < 0 < vals[-1]


@pytest.mark.parametrize("shape", SHAPES, ids=fc.shape_id)
def test_the_twin_on_nan_infinite_and_flt_max_candidates_at_every_radius(driver, tmp_path, shape):
    case = rc.nonfinite_case(shape)
    batch = rc.nonfinite_batch(case, case["radii"])
    got = check(driver, tmp_path, rc.queries_of(batch, 1) + rc.queries_of(batch, 0))
    n = len(case["radii"])
    for sm in (0, 1):
        rows = dict(zip(["inf", "max", "below", "nan", "-inf", "0", "-0", "tiny"], got[sm * n:(sm + 1) * n]))
        assert (rows["inf"][1] == FLT_MAX).sum() == 1 and (rows["max"][1] == FLT_MAX).sum() == 0, "FLT_MAX passes under +inf alone"
        assert len(rows["inf"][0]) == len(rows["max"][0]) + 1 == len(rows["below"][0]) + 1
        assert len(rows["nan"][0]) == 0 and len(rows["-inf"][0]) == 0
        assert np.isneginf(rows["0"][1]).any() and (rows["0"][1] < 0).all() and np.array_equal(rows["0"][0], rows["-0"][0])
        assert len(rows["tiny"][0]) > len(rows["0"][0]) and (rows["tiny"][1] <= 0).all(), "1e-45 keeps the zeros too"


def test_the_restatement_keeps_subnormals_after_a_fast_math_library_is_loaded(tmp_path):
    """a shared library linked with -ffast-math turns on flush-to-zero in the thread that loads it (the reference build does, in the
    test process); rc.ieee keeps the restatement's sums and compares IEEE 754 all the same, and leaves the caller's mode as it was"""
    so = str(tmp_path / "libfast.so")
    src = tmp_path / "fast.c"
    src.write_text("int qadc_test_fast_math_marker(void) { return 1; }\n")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O2", "-ffast-math", str(src), "-o", so])
    script = """
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
import adc_range_cases as rc
one = np.array([1, 0x80000003], np.uint32).view(np.float32)              # 2^-149 and -3 x 2^-149
table = np.zeros((2, 256), np.float32)
table[0, :2] = one
codes = np.array([[0, 5], [1, 5]], np.uint8)
plain = lambda: (one + np.float32(0)).view(np.uint32).tolist()
before = plain()
ctypes.CDLL(%r)
flushed = plain()
for sum_mode in (1, 0):
    v = rc.candidates((2, 8), codes, table, sum_mode)
    assert v.view(np.uint32).tolist() == [1, 0x80000003], v
    keys, vals = rc.expected((2, 8), [codes], [np.array([8, 9], np.uint32)], table, rc.TINY, sum_mode=sum_mode)
    assert keys.tolist() == [9] and vals.view(np.uint32).tolist() == [0x80000003], (keys, vals)
assert plain() == flushed, "the caller's mode is restored"
print(before == [1, 0x80000003], flushed != before)
""" % (os.path.join(ROOT, "tests"), so)
    out = subprocess.run([sys.executable, "-W", "ignore", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    ieee_before, _library_flushes = out.stdout.decode().split()           # (a toolchain whose library does not flush: the asserts above hold anyway)
    assert ieee_before == "True", "a fresh process adds subnormals as IEEE 754 does"


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "adc_range_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(9)
    cases = []
    for shape in SHAPES:
        parts = [fc.rand_codes(rng, shape, n) for n in (300, 0, 77)]
        labels = [np.arange(300, dtype=np.uint32) * 3, np.zeros(0, np.uint32), (np.arange(77, dtype=np.uint64) + (2 ** 32 - 77)).astype(np.uint32)]
        tables = fc.rand_tables(rng, shape, 1, 3)[0]
        for first, second in ((("exclude", np.arange(0, 900, 6)), ("allow", np.arange(0, 900, 9))), ((None, []), (None, [])),
                              (("allow", np.array([2 ** 32 - 1, 3, 3, 5])), ("exclude", np.array([3])))):
            for r in (INF, np.float32(20.0), -INF):
                cases.append(dict(shape=shape, parts=parts, labels=labels, tables=tables, radius=r, first=first, second=second))
    check(exe, tmp_path, cases)
