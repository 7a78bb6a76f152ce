"""What k-means++ seeding (qadc_kmeans_seed_host; include/qadc.h "k-means++ seeding") must compute, and the
plumbing its tests share: the CPU twin through its driver (tests/cpp/kmeans_seed_host.cpp), a numpy restatement of the whole
definition for integer-valued data, and the edge-case learning sets."""
import os
import subprocess

import numpy as np

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "kmeans_seed_host")
RADIX = 64
MASK = (1 << 64) - 1
EDGE_N = [1, 63, 64, 65, 4095, 4096, 4097, 262145]


def build_driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "kmeans_seed_host.cpp"), EXE, link=False)
    return EXE


def _run(exe, mode, tmp_path, v, k, sq_count, seed, seeds, coarse, rotation):
    v = np.ascontiguousarray(v, np.float32)
    n, dim = v.shape
    co = np.zeros((0, dim), np.float32) if coarse is None else np.ascontiguousarray(coarse, np.float32)
    rot = np.zeros((0,), np.float32) if rotation is None else np.ascontiguousarray(rotation, np.float32)
    fin, fout = str(tmp_path / ("kseed_%s.in" % mode)), str(tmp_path / ("kseed_%s.out" % mode))
    with open(fin, "wb") as f:
        np.array([n, dim, sq_count, k, len(co), int(rotation is not None), seed, seeds], np.uint64).tofile(f)   # (the seed is unsigned)
        for a in (v, co, rot):
            a.tofile(f)
    out = subprocess.run([exe, mode, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    return fout


def twin(exe, tmp_path, v, k, sq_count=1, seed=0, coarse=None, rotation=None):
    """host/db_build.hpp kmeans_seed -> (centres [sq_count][k][dsub], rows uint32 [sq_count][k], fallbacks)"""
    dim = np.asarray(v).shape[1]
    fout = _run(exe, "seed", tmp_path, v, k, sq_count, seed, 1, coarse, rotation)
    with open(fout, "rb") as f:
        centres = np.fromfile(f, np.float32, k * dim).reshape(sq_count, k, dim // sq_count)
        rows = np.fromfile(f, np.uint32, sq_count * k).reshape(sq_count, k)
        fallbacks = int(np.fromfile(f, np.uint64, 1)[0])
        assert f.read() == b""
    return centres, rows, fallbacks


def twin_rows(exe, tmp_path, v, k, sq_count, seed, seeds):
    """the twin's rows for seeds seed .. seed + seeds - 1 -> uint32 [seeds][sq_count][k]"""
    fout = _run(exe, "rows", tmp_path, v, k, sq_count, seed, seeds, None, None)
    return np.fromfile(fout, np.uint32).reshape(seeds, sq_count, k)


def uniform(seed, m, t):
    """u(m, t) of include/qadc.h, in Python integers"""
    z = (seed + 0x9E3779B97F4A7C15 * (((m << 32) | t) + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return (z >> 11) * 2.0 ** -53


def _level_up(a):
    """the next tree level: balanced binary sums over groups of 64, missing nodes 0.0"""
    pad = np.zeros(-(-len(a) // RADIX) * RADIX, np.float64)
    pad[:len(a)] = a
    g = pad.reshape(-1, RADIX)
    while g.shape[1] > 1:
        g = g[:, 0::2] + g[:, 1::2]
    return g[:, 0]


def _child(level, node, target):
    c, last, last_c = 0.0, -1, 0.0
    for j in range(RADIX):
        idx = node * RADIX + j
        child = float(level[idx]) if idx < len(level) else 0.0
        if child > 0.0:
            last, last_c = j, c
        if target < c + child:
            return j, target - c
        c = c + child
    return last, target - last_c


def restate(x, k, sq_count, seed):
    """The definition in numpy for integer-valued x with entries in [0, 2^10) and dsub <= 16: every difference, square and sum of
    a distance is then an integer below 2^24, exact in float32 without a fused operation, and every tree sum is an exact integer in
    float64.  -> (rows [sq_count][k], fallbacks)"""
    x = np.asarray(x)
    n, dim = x.shape
    ds = dim // sq_count
    assert ds <= 16 and x.min() >= 0 and x.max() < 1024 and np.array_equal(x, np.floor(x))
    xi = x.astype(np.int64)
    rows, fallbacks = np.zeros((sq_count, k), np.uint32), 0
    for m in range(sq_count):
        sub = xi[:, m * ds:(m + 1) * ds]
        mind = np.full(n, np.inf, np.float32)
        picked = np.zeros(n, bool)
        cursor = 0
        for t in range(k):
            u = uniform(seed, m, t)
            if t == 0:
                row = min(n - 1, int(u * float(n)))
            else:
                d = ((sub - sub[rows[m, t - 1]]) ** 2).sum(axis=1).astype(np.float32)
                mind = np.where(d < mind, d, mind)
                levels = [np.where(mind < np.inf, mind, 0).astype(np.float64)]
                while len(levels) < 3 or len(levels[-1]) > 1:
                    levels.append(_level_up(levels[-1]))
                root = float(levels[-1][0])
                if root == 0.0:
                    while picked[cursor]:
                        cursor += 1
                    row = cursor
                    fallbacks += 1
                else:
                    target, row = u * root, 0
                    for lvl in range(len(levels) - 1, 0, -1):
                        j, target = _child(levels[lvl - 1], row, target)
                        row = row * RADIX + j
            picked[row] = True
            rows[m, t] = row
    return rows, fallbacks


def integer_set(n, dim, seed=0):
    """integer-valued float32 vectors in [0, 2^10)"""
    return np.random.default_rng(1000 + n + seed).integers(0, 1024, (n, dim)).astype(np.float32)


def real_set(n, dim, seed=0):
    """clustered float vectors: the rounding of the distance chain and of the tree sums matters"""
    rng = np.random.default_rng(2000 + n + dim + seed)
    centres = rng.normal(size=(7, dim)) * 4.0
    return np.ascontiguousarray(centres[rng.integers(0, 7, n)] + rng.normal(size=(n, dim)), np.float32)


BAD_FIRST = 5      # nonfinite_set keeps rows [0, BAD_FIRST) finite


def nonfinite_set(n=40, dim=8):
    """-> (vectors, bad [n] bool): rows holding a NaN, a +inf, a -inf, or a value whose distance to anything overflows, scattered past
    row BAD_FIRST.  A bad row is never drawn by the D^2 rule; it can only be pick 0 or a fallback pick."""
    v = real_set(n, dim, 7)
    bad = np.zeros(n, bool)
    for i, val in zip((5, 9, 17, 23, 31, 39), (np.nan, np.inf, 3e38, -np.inf, np.nan, -3e38)):
        v[i, (i * 3) % dim] = val
        bad[i] = True
    return v, bad


def check_centres(x, centres, rows, sq_count):
    """centres [sq_count][k][dsub] are the named rows' sub-vectors of x [n][dim], bit for bit"""
    x = np.ascontiguousarray(x, np.float32)
    ds = x.shape[1] // sq_count
    for m in range(sq_count):
        want = x[rows[m].astype(np.int64), m * ds:(m + 1) * ds]
        assert np.array_equal(np.ascontiguousarray(want).view(np.uint32), np.ascontiguousarray(centres[m]).view(np.uint32)), m


def same(got, want):
    """(centres, rows, fallbacks) of the device against the twin's, bit for bit"""
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[1], want[1]), "rows differ, first at %s" % (np.argwhere(got[1] != want[1])[0],)
    assert np.array_equal(np.ascontiguousarray(got[0]).view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32)), "centres differ"
    assert got[2] == want[2], "fallbacks %d, expected %d" % (got[2], want[2])


BIG = dict(n=65600, dim=4, sq_count=2, k=65536, seed=2024)
BIG_GOLDEN = os.path.join(ROOT, "tests", "golden", "kmeans_seed_big.json")


def big_set():
    """the learning set of the k = 65536 case, from integer arithmetic alone (the same floats under every numpy): entry e is the top
    24 bits of splitmix64(e) times 2^-24"""
    from helpers import splitmix64
    e = np.arange(BIG["n"] * BIG["dim"], dtype=np.uint64)
    return np.ascontiguousarray(((splitmix64(e) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(BIG["n"], BIG["dim"]))


def rows_digest(rows):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(rows, "<u4").tobytes()).hexdigest()


def record_big(tmp_path):
    """The twin's answer to the k = 65536 case takes about a minute of one CPU core (65536 passes of std::fmaf calls over 65600 rows
    in two sub-spaces), so its rows are recorded as a digest: python -c "import pathlib, kmeans_seed_compose as ks;
    ks.record_big(pathlib.Path('/tmp'))" from tests/ rewrites tests/golden/kmeans_seed_big.json."""
    import json
    _, rows, fallbacks = twin(build_driver(), tmp_path, big_set(), BIG["k"], BIG["sq_count"], seed=BIG["seed"])
    with open(BIG_GOLDEN, "w") as f:
        json.dump(dict(BIG, rows_sha256=rows_digest(rows), fallbacks=fallbacks, first_rows=rows[:, :8].tolist(),
                       last_rows=rows[:, -8:].tolist()), f, indent=1)
        f.write("\n")
