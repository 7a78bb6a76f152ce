"""CPU: the append planner of the float-ADC engine (quick-adc_amd/host/adc_append_plan.hpp, driver
tests/cpp/adc_append_plan_host.cpp).

qadc_adc_index_add_vectors writes rows behind a partition's last one and the scan kernels read whole 16-byte words up to a
partition's end; both are legal only while the layout keeps the invariants checked here after every append of a sequence, planned
by the header as the library compiles it."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_append_plan_host")
LIMIT = 2 ** 32 - 1
REFUSAL = "partition %d would hold %d codes: at most 2^32 - 1 per partition"


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "adc_append_plan_host.cpp"), EXE, link=False)
    return EXE


def align16(v):
    return (np.asarray(v, np.int64) + 15) // 16 * 16


def run(exe, tmp_path, code_size, sizes, caps, steps):
    """steps: (add [parts], floor [parts] or None, grow) -> per step ('refused', message) or a dict of the plan"""
    parts = len(sizes)
    fin, fout = str(tmp_path / "append.in"), str(tmp_path / "append.out")
    with open(fin, "wb") as f:
        np.array([code_size, parts, len(steps)], np.int32).tofile(f)
        np.asarray(sizes, np.uint32).tofile(f)
        np.asarray(caps, np.uint32).tofile(f)
        for add, floor, grow in steps:
            np.array([int(grow), int(floor is not None)], np.int32).tofile(f)
            np.asarray(add, np.uint64).tofile(f)
            np.asarray(floor if floor is not None else np.zeros(parts), np.uint32).tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().splitlines()
    assert lines[0] == "ok"
    refusals = dict((int(l.split(":")[0].split()[1]), l.split(": ", 1)[1]) for l in lines[1:])
    plans = []
    with open(fout, "rb") as f:
        for s in range(len(steps)):
            status = int(np.fromfile(f, np.int32, 1)[0])
            if status == 2:
                plans.append(("refused", refusals[s]))
                continue
            p = dict(moved=status == 1, cap=np.fromfile(f, np.uint32, parts).astype(np.int64),
                     off=np.fromfile(f, np.uint64, parts).astype(np.int64), lab_off=np.fromfile(f, np.uint64, parts).astype(np.int64))
            p["code_bytes"], p["label_count"] = (int(x) for x in np.fromfile(f, np.uint64, 2))
            plans.append(p)
        assert f.read() == b""
    return plans


def layout(code_size, caps):
    """regions of the given capacities back to back: (off, lab_off)"""
    caps = np.asarray(caps, np.int64)
    ends = np.cumsum(align16(caps * code_size))
    return np.concatenate([[0], ends[:-1]])[:len(caps)], np.concatenate([[0], np.cumsum(caps)[:-1]])[:len(caps)]


def check_sequence(code_size, sizes, caps, steps, plans):
    """every invariant after every step; returns the number of relocations"""
    sizes, caps = np.asarray(sizes, np.int64).copy(), np.asarray(caps, np.int64).copy()
    off, lab_off = layout(code_size, caps)
    moves = 0
    for (add, floor, grow), p in zip(steps, plans):
        add = np.asarray(add, dtype=object)
        total = np.array([int(s) + int(a) for s, a in zip(sizes, add)], dtype=object)
        if any(t > LIMIT for t in total):
            first = [i for i, t in enumerate(total) if t > LIMIT][0]
            assert p == ("refused", REFUSAL % (first, total[first]))
            continue                                                             # a refused step changes nothing
        assert isinstance(p, dict), p
        total = total.astype(np.int64)
        want = np.zeros(len(sizes), np.int64) if floor is None else np.asarray(floor, np.int64)
        fits = bool((total <= caps).all() and (want <= caps).all())
        assert p["moved"] == (not fits)
        if fits:                                                                 # in place: nothing moves
            assert np.array_equal(p["cap"], caps) and np.array_equal(p["off"], off) and np.array_equal(p["lab_off"], lab_off)
        else:
            moves += 1
            assert (p["cap"] >= caps).all() and (p["cap"] >= want).all()       # never shrinks, honours the reserve
            if grow:
                assert (2 * p["cap"] >= np.minimum(3 * total, 2 * LIMIT)).all()   # at least 1.5 times the new size (a capacity is 32-bit too)
        assert (p["cap"] >= total).all() and (p["cap"] <= LIMIT).all()
        assert (p["off"] % 16 == 0).all()
        region = align16(p["cap"] * code_size)
        assert (region >= p["cap"] * code_size).all()
        assert np.array_equal(p["off"][1:], (p["off"] + region)[:-1]) and (len(sizes) == 0 or p["off"][0] == 0)     # back to back: no overlap
        assert p["code_bytes"] == int((p["off"] + region)[-1]) if len(sizes) else p["code_bytes"] == 0   # the 16 bytes of padding follow
        assert np.array_equal(p["lab_off"][1:], (p["lab_off"] + p["cap"])[:-1])
        assert p["label_count"] == int(p["cap"].sum())
        # a scan reads whole 16-byte words up to the partition's last row: inside the region
        assert (align16(total * code_size) <= region).all()
        sizes, caps, off, lab_off = total, p["cap"], p["off"], p["lab_off"]
    return moves


@pytest.mark.parametrize("code_size", [4, 8, 16])
def test_random_append_sequences_keep_the_layout(driver, tmp_path, code_size):
    rng = np.random.default_rng(code_size)
    for parts in (1, 3, 8, 300):
        sizes = rng.integers(0, 50, parts)
        sizes[rng.random(parts) < 0.5] = 0
        caps = sizes.copy()                                                      # add_partitions: capacity = size
        steps = []
        for s in range(60):
            add = rng.integers(0, 1 + int(rng.choice([1, 4, 40, 3000])), parts)
            add[rng.random(parts) < rng.random()] = 0                            # many partitions untouched
            floor = rng.integers(0, 5000, parts) if s % 17 == 5 else None
            grow = not (floor is not None and s % 2)                             # a reserve (exact) or an append with a floor
            if floor is not None and not grow:
                add[:] = 0
            steps.append((add, floor, grow))
        plans = run(driver, tmp_path, code_size, sizes, caps, steps)
        assert check_sequence(code_size, sizes, caps, steps, plans) >= 1


@pytest.mark.parametrize("code_size", [4, 8, 16])
def test_hand_made_sequences(driver, tmp_path, code_size):
    z = [0, 0, 0]
    steps = [([0, 0, 0], None, True),            # nothing to add to an empty database: in place
             ([1, 0, 0], None, True),            # the first row relocates
             ([1, 0, 0], None, True),
             ([0, 0, 7], None, True),
             (z, [100, 0, 9], False),            # a reserve: exact capacities
             ([98, 0, 0], None, True),           # fits the reserve exactly: in place
             ([1, 0, 0], None, True),            # one more does not
             (z, [1, 1, 1], False),              # a smaller reserve changes nothing
             ([0, 5, 0], [0, 400, 0], True)]     # an append with a floor above 1.5 times the size
    plans = run(driver, tmp_path, code_size, z, z, steps)
    check_sequence(code_size, z, z, steps, plans)
    moved = [p["moved"] for p in plans]
    assert moved == [False, True, False, True, True, False, True, False, True]   # (the first relocation leaves room for a second row)
    assert plans[4]["cap"][0] >= 100 and plans[5]["cap"][0] == plans[4]["cap"][0]
    assert plans[8]["cap"][1] >= 400


@pytest.mark.parametrize("code_size", [4, 8, 16])
def test_single_appends_relocate_logarithmically(driver, tmp_path, code_size):
    """N single-code appends to one partition: a relocation leaves room for half as many rows again, so at most
    ceil(log_1.5 N) + 2 of them"""
    N = 5000
    steps = [([1], None, True)] * N
    plans = run(driver, tmp_path, code_size, [0], [0], steps)
    moves = check_sequence(code_size, [0], [0], steps, plans)
    assert 1 <= moves <= math.ceil(math.log(N, 1.5)) + 2


@pytest.mark.parametrize("code_size", [4, 8, 16])
def test_totals_over_2_32_minus_1_are_refused(driver, tmp_path, code_size):
    sizes = [LIMIT - 5, 7, 0]
    steps = [([5, 0, 0], None, True),            # exactly 2^32 - 1: taken
             ([1, 0, 0], None, True),            # one more: refused, partition 0 named
             ([0, LIMIT - 6, 2 ** 33], None, True),   # partitions 1 and 2 over the limit: the first is named
             ([0, 0, LIMIT], None, True)]        # an empty partition may take 2^32 - 1
    plans = run(driver, tmp_path, code_size, sizes, sizes, steps)
    check_sequence(code_size, sizes, sizes, steps, plans)
    assert isinstance(plans[0], dict) and plans[0]["cap"][0] == LIMIT
    assert plans[1] == ("refused", REFUSAL % (0, LIMIT + 1))
    assert plans[2][0] == "refused"
    assert isinstance(plans[3], dict) and plans[3]["moved"]


def bases(exe, sizes, counts):
    out = subprocess.run([exe, "bases", ",".join(map(str, sizes)), ",".join(map(str, counts))], stdout=subprocess.PIPE, timeout=60)
    assert out.returncode == 0
    return [int(l) for l in out.stdout.decode().split()]


def test_pass_bases_place_every_vector_behind_its_partition_s_rows(driver):
    """append_bases: the vector at position j of a pass's (assign, i) order goes to row base[assign] + j modulo 2^32, which must be
    the next free row of its partition — also where the running sum of the counts, or a base itself, wraps."""
    rng = np.random.default_rng(11)
    cases = [([0, 0, 0], [0, 0, 0]), ([5], [7]), ([3, 0, 9, 1], [2, 0, 0, 4]),
             ([0, 1, 0], [10, 10, 10]),                              # a base below zero: wraps, and comes back with j
             ([LIMIT - 6, 0, 7], [6, LIMIT, 5]),                     # the running sum of the counts passes 2^32
             ([LIMIT - 1, LIMIT - 1], [1, 1])]
    cases += [(rng.integers(0, 2 ** 31, 9).tolist(), rng.integers(0, 2 ** 30, 9).tolist()) for _ in range(4)]
    for sizes, counts in cases:
        got = bases(driver, sizes, counts)
        assert len(got) == len(sizes)
        below = 0
        for p, (n, c) in enumerate(zip(sizes, counts)):
            assert got[p] == (n - below) % 2 ** 32
            assert (got[p] + below) % 2 ** 32 == n                   # the partition's first vector lands on its first free row
            if c:
                assert (got[p] + below + c - 1) % 2 ** 32 == (n + c - 1) % 2 ** 32
            below += c
