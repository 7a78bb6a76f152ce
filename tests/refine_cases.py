"""Shared by the re-ranking tests: the driver of the host twin (tests/cpp/refine_host.cpp over
quick-adc_amd/host/refine.hpp), an independent numpy restatement of the definition, and builders of the cases both the CPU and the
GPU tests run.  A case is a dict: dim, dtype ("f32" | "f16"), adds [(first_key, vectors [n][dim])], queries [nq][dim],
keys [nq][r_in] uint32, counts [nq] int32 or None, values [nq][r_in] float32 or None, R."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_host")
FLT_MAX = np.float32(3.4028234663852886e38)
NAN_IMAGE = 0x7FC00000
NO_KEY = 0xFFFFFFFF
DTYPES = {"f32": 0, "f16": 1}
DIMS = (1, 63, 64, 65, 96, 128, 4096)


def build_driver():
    from test_scanner_hip_cpp import _compile
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def case(dim, dtype, adds, queries, keys, R, counts=None, values=None):
    queries = np.ascontiguousarray(queries, np.float32).reshape(-1, dim)
    keys = np.ascontiguousarray(keys, np.uint32).reshape(queries.shape[0], -1)
    return dict(dim=dim, dtype=dtype, adds=[(int(k), np.ascontiguousarray(v, np.float32).reshape(-1, dim)) for k, v in adds], queries=queries,
                keys=keys, R=int(R), counts=None if counts is None else np.ascontiguousarray(counts, np.int32),
                values=None if values is None else np.ascontiguousarray(values, np.float32).reshape(keys.shape))


def run_twin(exe, tmp_path, cases):
    """-> [dict(refused, missing, keys [nq][R], dist [nq][R], sizes [nq])] of the host twin"""
    fin, fout = str(tmp_path / "refine.in"), str(tmp_path / "refine.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            nq, r_in = c["keys"].shape
            np.array([c["dim"], DTYPES[c["dtype"]], len(c["adds"]), nq, r_in, c["R"], c["counts"] is not None, c["values"] is not None],
                     np.int32).tofile(f)
            for first, vec in c["adds"]:
                np.array([first, len(vec)], np.uint32).tofile(f)
                vec.tofile(f)
            c["queries"].tofile(f)
            c["keys"].tofile(f)
            if c["counts"] is not None:
                c["counts"].tofile(f)
            if c["values"] is not None:
                c["values"].tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        for c in cases:
            nq, R = c["keys"].shape[0], c["R"]
            refused = int(np.fromfile(f, np.int32, 1)[0])
            missing = int(np.fromfile(f, np.uint64, 1)[0])
            got.append(dict(refused=refused, missing=missing, keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R),
                            dist=np.fromfile(f, np.float32, nq * R).reshape(nq, R), sizes=np.fromfile(f, np.int32, nq)))
        assert f.read() == b""
    return got


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------

def stored_rows(c):
    """(lo, rows [n][dim] float32 as the store holds them): the adds in order, an f16 store through astype(float16)"""
    lo = c["adds"][0][0] if c["adds"] else 0
    rows = np.concatenate([v for _, v in c["adds"]]) if c["adds"] else np.zeros((0, c["dim"]), np.float32)
    if c["dtype"] == "f16":
        with np.errstate(over="ignore"):
            rows = rows.astype(np.float16).astype(np.float32)
    return lo, rows


def np_distance(q, X):
    """D(q, x) of every row x of X [n][dim] -> float32 [n]: 64 strided partial sums, then the six halvings; float32 throughout"""
    n, dim = X.shape
    with np.errstate(all="ignore"):
        t = q[None, :].astype(np.float32) - X.astype(np.float32)
        tt = t * t
        strips = np.concatenate([tt, np.zeros((n, -dim % 64), np.float32)], axis=1).reshape(n, -1, 64)   # (p + 0 is p)
        p = np.zeros((n, 64), np.float32)
        for j in range(strips.shape[1]):
            p = p + strips[:, j, :]
        for s in (32, 16, 8, 4, 2, 1):
            p = p[:, :s] + p[:, s:2 * s]
    assert p.dtype == np.float32
    return p[:, 0]


def np_rerank(c):
    """the definition, restated: -> dict(missing, keys, dist, sizes)"""
    lo, rows = stored_rows(c)
    nq, r_in = c["keys"].shape
    R = c["R"]
    keys = np.full((nq, R), NO_KEY, np.uint32)
    dist = np.full((nq, R), np.inf, np.float32)
    sizes = np.zeros(nq, np.int32)
    missing = 0
    for q in range(nq):
        count = r_in if c["counts"] is None else int(c["counts"][q])
        k = c["keys"][q, :count].astype(np.int64)
        if c["values"] is not None:
            k = k[c["values"][q, :count] != FLT_MAX]
        held = (k >= lo) & (k < lo + len(rows))
        missing += int((~held).sum())
        k = np.unique(k[held])
        if len(k) == 0:
            continue
        d = np_distance(c["queries"][q], rows[k - lo])
        img = d.view(np.uint32).astype(np.uint64)
        img[np.isnan(d)] = NAN_IMAGE
        words = np.sort((img << np.uint64(32)) | k.astype(np.uint64))[:R]
        n = len(words)
        keys[q, :n] = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        dist[q, :n] = (words >> np.uint64(32)).astype(np.uint32).view(np.float32)
        sizes[q] = n
    return dict(missing=missing, keys=keys, dist=dist, sizes=sizes)


def same(a, b):
    """None where two results agree bit for bit, else what differs"""
    for name in ("sizes", "keys"):
        if not np.array_equal(a[name], b[name]):
            return name
    if not np.array_equal(a["dist"].view(np.uint32), b["dist"].view(np.uint32)):
        return "dist"
    if a["missing"] != b["missing"]:
        return "missing %d != %d" % (a["missing"], b["missing"])
    return None


# ---- case builders ------------------------------------------------------------------------------------------------------------

def random_case(rng, dim, dtype, rows, nq, r_in, R, lo=0, scale=1.0):
    """plain case: random rows, random candidate keys inside the store (duplicates happen)"""
    vec = (rng.normal(size=(rows, dim)) * scale).astype(np.float32)
    q = (rng.normal(size=(nq, dim)) * scale).astype(np.float32)
    keys = (rng.integers(0, rows, (nq, r_in)) + lo).astype(np.uint32)
    return case(dim, dtype, [(lo, vec)], q, keys, R)


def edge_case(rng, dim, dtype):
    """ties straddling R, duplicate keys, skipped and missing entries, count 0, R above the survivors — in one batch of 5 queries"""
    rows, lo, r_in = 40, 50, 24
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[10:20] = vec[10]                                                   # ten identical rows under different keys
    q = rng.normal(size=(5, dim)).astype(np.float32)
    q[0] = vec[10]                                                         # ... all at distance 0 from query 0
    keys = (rng.integers(0, rows, (5, r_in)) + lo).astype(np.uint32)
    keys[0, :10] = np.arange(10, 20)[::-1] + lo
    keys[1, :] = lo + 7                                                    # one key r_in times
    keys[2, 3] = keys[2, 4]                                                # a key twice
    keys[2, 5:9] = (lo - 1, lo + rows, 0, 0xFFFFFFFF)                      # missing: below lo, at lo + rows, far away
    values = rng.random((5, r_in)).astype(np.float32)
    values[2, 10:14] = FLT_MAX                                             # skipped
    values[3, :] = FLT_MAX                                                 # everything skipped
    counts = np.array([r_in, r_in, r_in, r_in, 0], np.int32)
    return case(dim, dtype, [(lo, vec)], q, keys, 6, counts=counts, values=values)


def nonfinite_case(rng, dim, dtype):
    """a NaN and an inf component in a row and in a query: NaN distances last, as 0x7FC00000"""
    rows, r_in = 30, 30
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[3, 0] = np.nan
    vec[4, dim - 1] = np.inf
    vec[5, dim // 2] = -np.inf
    q = rng.normal(size=(4, dim)).astype(np.float32)
    q[1, 0] = np.nan                                                       # every distance NaN
    q[2, dim - 1] = np.inf                                                 # inf - inf = NaN on row 4, inf elsewhere
    q[3, dim // 2] = -np.inf
    keys = np.tile(np.arange(rows, dtype=np.uint32), (4, 1))
    return case(dim, dtype, [(0, vec)], q, keys, r_in + 2)


def half_range_case(rng, dim):
    """f16 rows whose inputs are subnormal as halves, round to the smallest normal, overflow to inf and tie at the last place"""
    special = np.array([5.9604645e-08, 2.9802322e-08, 2.9802326e-08, 8.9406967e-08, 6.0975552e-05, 6.1035156e-05, 6.1005354e-05, 65504.0, 65519.996,
                        65520.0, 70000.0, -65520.0, 1e-10, -1e-10, 1.00048828125, 1.0009765625 + 0.00048828125, 0.333333, 3.0e-6, -4.7e-7, 1e38],
                       np.float32)
    rows = 48
    vec = (rng.normal(size=(rows, dim)) * 1e-5).astype(np.float32)        # mostly subnormal halves
    flat = vec.reshape(-1)
    pos = rng.permutation(flat.size)[:len(special)] if flat.size >= len(special) else np.arange(flat.size)
    flat[pos] = special[:len(pos)]
    q = (rng.normal(size=(3, dim)) * 1e-5).astype(np.float32)
    keys = np.tile(np.arange(rows, dtype=np.uint32), (3, 1))
    return case(dim, "f16", [(0, vec)], q, keys, rows)
