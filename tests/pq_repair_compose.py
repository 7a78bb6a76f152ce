"""What the empty-cluster repair of PQ training (qadc_pq_repair_host, qadc_*_train_repair_*; include/qadc.h "Empty-cluster repair",
DESIGN.md section 11.18) must compute: the definition in numpy, the training rounds composed from pq_train_compose /
pq_train16_compose and the repair, the CPU twin through its driver (tests/cpp/pq_repair_host.cpp), and the crafted cases the CPU and
GPU tests share.

The distance is ONE float chain acc = fmaf(t, t, acc), t = x - c.  On integer-valued data it is what kmeans_seed_compose.restate
computes (every difference, square and sum an integer below 2^24: exact without a fused operation) — int_distance below, the form
most crafted cases use.  For the floats a training round produces, chain() restates the fused step exactly: t * t is exact in
float64 (48 bits), the float64 sum acc + t * t is corrected to round-to-odd with the error term of a two-sum, and a round-to-odd
value of 53 bits rounds to float32 as the infinitely precise sum does (53 >= 2 * 24 + 2)."""
import os
import subprocess

import numpy as np

import pq_train_compose as ptc
import pq_train16_compose as pt16
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "pq_repair_host")


def build_driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "pq_repair_host.cpp"), EXE, link=False)
    return EXE


def _fma_sq(t, acc):
    """float32 fmaf(t, t, acc) elementwise"""
    with np.errstate(all="ignore"):
        p = t.astype(np.float64) * t.astype(np.float64)                     # exact
        a = acc.astype(np.float64)
        s = a + p
        bb = s - a
        err = (a - (s - bb)) + (p - bb)                                     # two-sum: a + p = s + err exactly
        odd = (s.view(np.uint64) & np.uint64(1)) == 1
        fix = np.isfinite(s) & (err != 0) & ~odd
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def chain(sub, cen):
    """sub [n][ds], cen [n][ds] (the assigned centroid of every row) -> float32 [n]"""
    sub, cen = np.ascontiguousarray(sub, np.float32), np.ascontiguousarray(cen, np.float32)
    acc = np.zeros(len(sub), np.float32)
    with np.errstate(all="ignore"):
        for d in range(sub.shape[1]):
            acc = _fma_sq(sub[:, d] - cen[:, d], acc)
    return acc


def int_distance(sub, cen):
    """the distance as kmeans_seed_compose.restate computes it, for integer-valued data with every sum below 2^24"""
    return ((sub.astype(np.int64) - cen.astype(np.int64)) ** 2).sum(axis=1).astype(np.float32)


def repair_slice(sub, cbm, assign):
    """One sub-space: sub [n][ds], cbm [K][ds], assign [n] -> (assign repaired, moved)"""
    sub = np.ascontiguousarray(sub, np.float32)
    assign = np.asarray(assign).astype(np.int64)
    n, K = len(sub), len(cbm)
    count = np.bincount(assign, minlength=K)
    empties = np.flatnonzero(count == 0)
    if len(empties) == 0:
        return assign.copy(), 0
    first = np.full(K, n, np.int64)
    np.minimum.at(first, assign, np.arange(n))
    d = chain(sub, cbm[assign])
    with np.errstate(all="ignore"):
        eligible = np.isfinite(d) & (d > 0) & (np.arange(n) != first[assign])
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    keys = np.where(eligible, keys, np.uint64(0))
    take = min(len(empties), int(eligible.sum()))
    chosen = np.sort(np.argsort(keys, kind="stable")[::-1][:take])           # the largest keys (distinct where eligible), ascending index
    assert take == 0 or keys[chosen].min() > 0
    out = assign.copy()
    out[chosen] = empties[:take]
    return out, take


def unpack(codes, bits):
    return np.asarray(codes).astype(np.int64) if bits == 16 else ptc.unpack(codes, bits).astype(np.int64)


def pack(assign, bits):
    return np.ascontiguousarray(assign, np.uint16) if bits == 16 else ptc.pack(assign, bits)


def repair(x, cb, codes):
    """x [n][dim], cb [nsq][K][ds], codes in the encoder's layout -> (codes repaired, moved uint32 [nsq])"""
    x = np.ascontiguousarray(x, np.float32)
    nsq, K, ds = cb.shape
    bits = {16: 4, 256: 8, 65536: 16}[K]
    a = unpack(codes, bits)
    moved = np.zeros(nsq, np.uint32)
    for m in range(nsq):
        a[:, m], moved[m] = repair_slice(x[:, m * ds:(m + 1) * ds], cb[m], a[:, m])
    return pack(a, bits), moved


def train(po, x, seed, iters, div_mode=1, sum_mode=1, repair=True):
    """pq_train_compose.train (4 and 8 bits) or pq_train16_compose.train with every round assign, repair, update
    -> (codebooks, codes of the last round, empty, repaired)"""
    x = np.ascontiguousarray(x, np.float32)
    cb = np.array(seed, np.float32, order="C", copy=True)
    nsq, K, ds = cb.shape
    bits = {16: 4, 256: 8, 65536: 16}[K]
    assign = np.zeros((x.shape[0], nsq), np.int64)
    repaired = 0
    for _ in range(iters):
        if bits == 16:
            import adc16_encode_compose as a16e
            assign = a16e.codes16(po, cb, x, sum_mode).astype(np.int64)
        for m in range(nsq):
            sub = np.ascontiguousarray(x[:, m * ds:(m + 1) * ds])
            if bits != 16:
                assign[:, m] = ptc.assign_slice(po, cb[m], sub, sum_mode)
            if repair:
                assign[:, m], moved = repair_slice(sub, cb[m], assign[:, m])
                repaired += moved
            cb[m] = pt16.update_slice(sub, assign[:, m], div_mode)[0] if bits == 16 else ptc.update_slice(sub, assign[:, m], K, div_mode)
    return cb, pack(assign, bits), ptc.empty_count(cb), repaired


def counts(codes, nsq, bits):
    """-> int64 [nsq][K]"""
    a = unpack(codes, bits)
    return np.stack([np.bincount(a[:, m], minlength=1 << bits) for m in range(nsq)])


def twin(exe, tmp_path, x, cb, codes):
    """host/pq_repair.hpp pq_repair -> (codes, moved uint32 [nsq])"""
    x = np.ascontiguousarray(x, np.float32)
    nsq, K, ds = cb.shape
    bits = {16: 4, 256: 8, 65536: 16}[K]
    c = np.ascontiguousarray(codes, "<u2" if bits == 16 else np.uint8)
    fin, fout = str(tmp_path / "repair.in"), str(tmp_path / "repair.out")
    with open(fin, "wb") as f:
        np.array([x.shape[0], x.shape[1], nsq, bits], np.int64).tofile(f)
        x.tofile(f)
        np.ascontiguousarray(cb, np.float32).tofile(f)
        c.tofile(f)
    out = subprocess.run([exe, "repair", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    with open(fout, "rb") as f:
        got = np.fromfile(f, c.dtype, c.size).reshape(c.shape)
        moved = np.fromfile(f, np.uint32, nsq)
        assert f.read() == b""
    return got.astype(np.uint16, copy=False) if bits == 16 else got, moved


def twin_train(exe, tmp_path, v, seed, iters, repair, div_mode=1):
    """host/db_build.hpp pq_train_iterations / pq_train16_iterations with `repair` -> (codebooks, codes, empty, repaired)"""
    v = np.ascontiguousarray(v, np.float32)
    nsq, K, ds = seed.shape
    bits = {16: 4, 256: 8, 65536: 16}[K]
    fin, fout = str(tmp_path / "rtrain.in"), str(tmp_path / "rtrain.out")
    with open(fin, "wb") as f:
        np.array([v.shape[0], v.shape[1], nsq, bits, iters, div_mode, int(repair)], np.int64).tofile(f)
        v.tofile(f)
        np.ascontiguousarray(seed, np.float32).tofile(f)
    out = subprocess.run([exe, "train", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    dt = np.dtype("<u2") if bits == 16 else np.dtype(np.uint8)
    cols = nsq // 2 if bits == 4 else nsq
    with open(fout, "rb") as f:
        cb = np.fromfile(f, np.float32, seed.size).reshape(seed.shape)
        codes = np.fromfile(f, dt, v.shape[0] * cols).reshape(v.shape[0], cols)
        empty, repaired = (int(t) for t in np.fromfile(f, np.uint64, 2))
        assert f.read() == b""
    return cb, codes.astype(np.uint16, copy=False) if bits == 16 else codes, empty, repaired


def same_codes(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), "%s: codes differ, first at %s" % (what, np.argwhere(got != want)[0])


# ---- the crafted cases: (sq_count, bits, dim) at the smallest dim of each shape ----
SHAPES = [(16, 4, 32), (32, 4, 64), (4, 8, 8), (16, 8, 16), (2, 16, 4), (8, 16, 16)]
PATTERNS = ["one_cluster", "all_alive", "grid_ties", "both_nibbles", "first_last_empty", "farthest_is_first", "zero_distance",
            "nonfinite_rows", "nan_centroid"]


def crafted(pattern, nsq, bits, dim, n, seed=0):
    """-> (x float32 [n][dim], cb float32 [nsq][K][ds], codes in the encoder's layout).  Everything finite is a small integer, so
    int_distance states the distances too; the live clusters are few, so that empties exist at every n."""
    rng = np.random.default_rng(10007 * (PATTERNS.index(pattern) + 1) + 131 * n + 7 * nsq + bits + seed)
    K, ds = 1 << bits, dim // nsq
    x = rng.integers(0, 8, (n, dim)).astype(np.float32)
    cb = rng.integers(0, 8, (nsq, K, ds)).astype(np.float32)
    live = max(2, min(K - 2, n // 3 + 1, 300))                              # clusters that may have members
    a = rng.integers(0, live, (n, nsq))
    if pattern == "one_cluster":                                            # E = K - 1 against at most n - 1 eligible
        a[:] = 3 % K
    elif pattern == "all_alive":                                            # (n >= K: every cluster alive, codes untouched)
        a = np.tile((np.arange(n) % K)[:, None], (1, nsq))
        for m in range(nsq):
            a[:, m] = rng.permutation(a[:, m])
    elif pattern == "grid_ties":                                            # equal distances straddle the selection boundary
        x = rng.integers(0, 2, (n, dim)).astype(np.float32)
        cb = rng.integers(0, 2, (nsq, K, ds)).astype(np.float32)
        a = rng.integers(K - min(K, 5), K, (n, nsq))                        # K - 5 empties at most: fewer than the tied vectors at large n
    elif pattern == "both_nibbles":                                         # the same rows are the farthest in every sub-space
        far = n - 1 - rng.choice(max(1, n // 4), min(3, max(1, n // 4)), replace=False)     # late rows: no cluster's first
        x[far] += np.float32(100) * np.arange(1, len(far) + 1, dtype=np.float32)[:, None]
    elif pattern == "first_last_empty":
        a = rng.integers(1, K - 1, (n, nsq)) if bits != 16 else rng.integers(1, live, (n, nsq))
    elif pattern == "farthest_is_first":                                    # row 0 is the farthest vector and its cluster's first
        x[0] += np.float32(500)
    elif pattern == "zero_distance":                                        # members exactly on their centroid
        on = rng.random(n) < 0.6
        for m in range(nsq):
            x[on, m * ds:(m + 1) * ds] = cb[m][a[on, m]]
    elif pattern == "nonfinite_rows":
        for i, val in zip(rng.choice(n, min(n, 6), replace=False), (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
            x[i, rng.integers(0, dim)] = val
            x[i, rng.integers(0, dim)] = val
    elif pattern == "nan_centroid":                                         # a NaN centroid that has members
        for m in range(nsq):
            cb[m, a[n // 2, m], rng.integers(0, ds)] = np.nan
            cb[m, a[0, m], 0] = np.inf
    else:
        raise ValueError(pattern)
    return x, cb, pack(a, bits)


def train_case(nsq, bits, dim, n, kind):
    """-> (v float32 [n][dim] with a block of identical sub-vectors in sub-space 0, seed [nsq][K][ds]).  kind "repeated": a seed
    holding repeated rows; "nan": the same with a NaN row in the middle, which hides every centroid below it from the first
    assignment.  At 16 bits most of the 65536 centroids lie far from the data, so that the vectors crowd into the few near ones and
    clusters have members to give."""
    rng = np.random.default_rng(17 * n + bits + len(kind))
    K, ds = 1 << bits, dim // nsq
    v = rng.normal(size=(n, dim)).astype(np.float32)
    v[n // 2:n // 2 + 40, :ds] = v[0, :ds]
    if bits == 16:
        seed = (rng.normal(size=(nsq, K, ds)) * 50 + 400).astype(np.float32)
        near = rng.choice(K, 24, replace=False)
        seed[:, near] = v[rng.integers(0, n, 24)].reshape(24, nsq, ds).transpose(1, 0, 2) + np.float32(0.25)
        seed[:, near[1:12:2]] = seed[:, near[:1]]
    else:
        rows = rng.integers(0, n, K)
        rows[1::3] = rows[0]
        seed = np.ascontiguousarray(v[rows].reshape(K, nsq, ds).transpose(1, 0, 2))
    if kind == "nan":
        seed[:, K // 2, 0] = np.nan
    return v, np.ascontiguousarray(seed, np.float32)
