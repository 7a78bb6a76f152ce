"""Shared by the tests of SQ8 refine rows and of the read-back: the driver of the host twin
(tests/cpp/refine_sq_host.cpp over quick-adc_amd/host/refine.hpp), an independent numpy restatement of encode, decode, range and the
clamp count (float32 numpy operations and np.rint; rerank and knn on decoded rows go through refine_cases.np_rerank), and builders of
the scripts both the CPU and the GPU tests run.

A script is a dict: dim, dtype ("f32" | "f16" | "sq8"), keyed, vmin, step (sq8) and ops, a list of tuples:
  ("add", first_key, vectors)  ("put", labels, vectors)  ("remove", labels)  ("get", keys)  ("bytes", keys)  ("info",)
  ("rerank", queries, keys, R, counts | None, values | None)  ("knn", queries, R, mode | None, filter_keys)  ("range", vectors)
A result is a list with one dict of arrays per operation."""
import os
import pickle
import subprocess
import sys

import numpy as np

import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_sq_host")
DTYPES = {"f32": 0, "f16": 1, "sq8": 2}
DIMS = (1, 63, 64, 65, 96, 128, 260, 4096)
NO_KEY = 0xFFFFFFFF
OPS = {"add": 1, "put": 2, "remove": 3, "get": 4, "rerank": 5, "knn": 6, "info": 7, "bytes": 8, "range": 9}
F32 = np.float32


def build_driver():
    from test_scanner_hip_cpp import _compile
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def script(dim, dtype, ops, keyed=False, vmin=None, step=None):
    s = dict(dim=int(dim), dtype=dtype, keyed=bool(keyed), ops=list(ops), vmin=None, step=None)
    if dtype == "sq8":
        s["vmin"] = np.ascontiguousarray(vmin, F32).reshape(dim)
        s["step"] = np.ascontiguousarray(step, F32).reshape(dim)
    return s


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, np.uint64).astype(np.uint32)).reshape(-1)


def _vec(a, dim):
    return np.ascontiguousarray(a, F32).reshape(-1, dim)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------

def run_twin(exe, tmp_path, scripts, flush=False):
    """-> [dict(refused, ops=[...])] of the host twin; flush: its thread flushes subnormals to zero (tests/cpp/refine_sq_host.cpp)"""
    fin, fout = str(tmp_path / "refine_sq.in"), str(tmp_path / "refine_sq.out")
    with open(fin, "wb") as f:
        np.array([len(scripts)], np.int32).tofile(f)
        for s in scripts:
            dim = s["dim"]
            np.array([dim, DTYPES[s["dtype"]], s["keyed"], len(s["ops"])], np.int32).tofile(f)
            if s["dtype"] == "sq8":
                s["vmin"].tofile(f)
                s["step"].tofile(f)
            for op in s["ops"]:
                np.array([OPS[op[0]]], np.int32).tofile(f)
                if op[0] == "add":
                    v = _vec(op[2], dim)
                    np.array([op[1], len(v)], np.uint32).tofile(f)
                    v.tofile(f)
                elif op[0] == "put":
                    v = _vec(op[2], dim)
                    np.array([len(v)], np.uint32).tofile(f)
                    _u32(op[1]).tofile(f)
                    v.tofile(f)
                elif op[0] in ("remove", "get", "bytes"):
                    k = _u32(op[1])
                    np.array([len(k)], np.uint32).tofile(f)
                    k.tofile(f)
                elif op[0] == "rerank":
                    q = _vec(op[1], dim)
                    k = np.ascontiguousarray(op[2], np.uint32).reshape(len(q), -1)
                    np.array([len(q), k.shape[1], op[3], op[4] is not None, op[5] is not None], np.int32).tofile(f)
                    q.tofile(f)
                    k.tofile(f)
                    if op[4] is not None:
                        np.ascontiguousarray(op[4], np.int32).tofile(f)
                    if op[5] is not None:
                        np.ascontiguousarray(op[5], F32).tofile(f)
                elif op[0] == "knn":
                    q = _vec(op[1], dim)
                    fk = _u32(np.sort(np.asarray(op[4], np.uint64))) if op[3] is not None else np.zeros(0, np.uint32)
                    np.array([len(q), op[2], -1 if op[3] is None else op[3], len(fk)], np.int32).tofile(f)
                    fk.tofile(f)
                    q.tofile(f)
                elif op[0] == "range":
                    v = _vec(op[1], dim)
                    np.array([len(v)], np.uint32).tofile(f)
                    v.tofile(f)
    out = subprocess.run([exe, fin, fout] + (["flush"] if flush else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        for s in scripts:
            dim = s["dim"]
            res = dict(refused=int(np.fromfile(f, np.int32, 1)[0]), ops=[])
            for op in s["ops"]:
                if op[0] in ("add", "put"):
                    r = dict(ok=np.fromfile(f, np.int32, 1))
                elif op[0] == "remove":
                    r = dict(removed=np.fromfile(f, np.uint64, 1))
                elif op[0] == "get":
                    n = len(_u32(op[1]))
                    r = dict(rows=np.fromfile(f, F32, n * dim).reshape(n, dim), found=np.fromfile(f, np.uint8, n))
                elif op[0] == "bytes":
                    n = len(_u32(op[1]))
                    r = dict(bytes=np.fromfile(f, np.uint8, n * dim).reshape(n, dim))
                elif op[0] == "rerank":
                    nq, R = len(_vec(op[1], dim)), op[3]
                    r = dict(missing=np.fromfile(f, np.uint64, 1), keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R),
                             dist=np.fromfile(f, F32, nq * R).reshape(nq, R), sizes=np.fromfile(f, np.int32, nq))
                elif op[0] == "knn":
                    nq, R = len(_vec(op[1], dim)), op[2]
                    r = dict(keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R), dist=np.fromfile(f, F32, nq * R).reshape(nq, R),
                             sizes=np.fromfile(f, np.int32, nq))
                elif op[0] == "info":
                    r = dict(clamped=np.fromfile(f, np.uint64, 1), held=np.fromfile(f, np.uint64, 1))
                elif op[0] == "range":
                    r = dict(vmin=np.fromfile(f, F32, dim), step=np.fromfile(f, F32, dim))
                res["ops"].append(r)
            got.append(res)
        assert f.read() == b""
    return got


def same(a, b):
    """None where two results of a script agree bit for bit, else what differs"""
    if a["refused"] != b["refused"]:
        return "refused"
    for i, (x, y) in enumerate(zip(a["ops"], b["ops"])):
        for name in x:
            p, q = np.ascontiguousarray(x[name]), np.ascontiguousarray(y[name])
            if p.dtype == F32:
                p, q = p.view(np.uint32), np.ascontiguousarray(q, F32).view(np.uint32)
            if p.shape != q.shape or not np.array_equal(p, q.astype(p.dtype)):
                return "operation %d: %s" % (i, name)
    return None


# ---- the numpy restatement --------------------------------------------------------------------------------------------------------

def np_inv(step):
    with np.errstate(all="ignore"):
        return np.where(step > 0, F32(1.0) / np.where(step > 0, step, F32(1.0)), F32(0.0)).astype(F32)


def np_encode(x, vmin, step):
    """x [n][dim] float32 -> (bytes uint8 [n][dim], clamped bool [n][dim])"""
    x = np.ascontiguousarray(x, F32)
    inv = np_inv(step)
    with np.errstate(all="ignore"):
        d = x - vmin[None, :]
        u = d * inv[None, :]
        assert d.dtype == F32 and u.dtype == F32
        mid = (u > 0) & ~(u >= F32(255.0))
        c = np.where(mid, np.rint(np.where(mid, u, F32(0.0))), np.where(u >= F32(255.0), F32(255.0), F32(0.0))).astype(np.uint8)
        clamped = np.where(step[None, :] > 0, ~(d >= 0) | ~(u <= F32(255.0)), ~(x == vmin[None, :]))
    return c, clamped


def np_decode(c, vmin, step):
    with np.errstate(all="ignore"):
        m = c.astype(F32) * step[None, :]
        x = vmin[None, :] + m
    assert x.dtype == F32
    return x


def np_range(v, dim):
    v = _vec(v, dim)
    u = v.view(np.uint32)
    finite = (u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    o = np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000))
    lo = np.where(finite, o, np.uint32(0xFFFFFFFF)).min(axis=0, initial=np.uint32(0xFFFFFFFF))
    hi = np.where(finite, o, np.uint32(0)).max(axis=0, initial=np.uint32(0))
    none = lo > hi

    def back(o):
        return np.where((o & np.uint32(0x80000000)) != 0, o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(F32)
    a, b = np.where(none, F32(0.0), back(lo)).astype(F32), np.where(none, F32(0.0), back(hi)).astype(F32)
    with np.errstate(all="ignore"):
        step = ((b - a) / F32(255.0)).astype(F32)
    return a, step


def params_ok(vmin, step):
    return bool(np.isfinite(vmin).all() and np.isfinite(step).all() and (step >= 0).all())


def _convert(s, v):
    """rows as the store decodes them, the bytes (sq8) and the clamped count"""
    if s["dtype"] == "sq8":
        c, cl = np_encode(v, s["vmin"], s["step"])
        return np_decode(c, s["vmin"], s["step"]), c, int(cl.sum())
    if s["dtype"] == "f16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16).astype(F32), None, 0
    return v.copy(), None, 0


def isolated(tmp_path, name, *args):
    """A function of this module, by name, in a fresh interpreter that loads nothing but numpy.  The restatement computes with
    subnormal float32 values (a subnormal step, differences next to vmin), and a test process may have loaded a library built with
    -ffast-math, whose start-up code makes the thread flush subnormals to zero: numpy in that process would restate another
    arithmetic than IEEE's.  A new process starts with the default floating-point environment."""
    fin, fout = str(tmp_path / "isolated.in"), str(tmp_path / "isolated.out")
    with open(fin, "wb") as f:
        pickle.dump((name, args), f)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()
    with open(fout, "rb") as f:
        return pickle.load(f)


def run_numpy_all(scripts):
    return [run_numpy(s) for s in scripts]


def run_numpy(s):
    """the restatement of a script -> dict(refused, ops)"""
    dim = s["dim"]
    if s["dtype"] == "sq8" and not params_ok(s["vmin"], s["step"]):
        return dict(refused=1, ops=[])
    rows, raw, clamped, lo = {}, {}, 0, None      # key -> decoded row / bytes
    out = []
    for op in s["ops"]:
        if op[0] == "add":
            v = _vec(op[2], dim)
            first = int(op[1])
            ok = len(v) == 0 or ((lo is None or first == lo + len(rows)) and first + len(v) <= 1 << 32 and not s["keyed"])
            if ok and len(v):
                lo = first if lo is None else lo
                dec, c, cl = _convert(s, v)
                clamped += cl
                for i in range(len(v)):
                    rows[first + i] = dec[i]
                    if c is not None:
                        raw[first + i] = c[i]
            out.append(dict(ok=np.array([ok], np.int32)))
        elif op[0] == "put":
            v, lab = _vec(op[2], dim), _u32(op[1])
            ok = s["keyed"] and not (lab == NO_KEY).any()
            if ok and len(v):
                last = {int(k): i for i, k in enumerate(lab)}          # the last occurrence of a key wins, and alone reaches a row
                win = np.array(sorted(last.values()), np.int64)
                dec, c, cl = _convert(s, v[win])
                clamped += cl
                for j, i in enumerate(win):
                    rows[int(lab[i])] = dec[j]
                    if c is not None:
                        raw[int(lab[i])] = c[j]
            out.append(dict(ok=np.array([ok], np.int32)))
        elif op[0] == "remove":
            gone = {int(k) for k in _u32(op[1])} & set(rows)
            for k in gone:
                del rows[k]
                raw.pop(k, None)
            out.append(dict(removed=np.array([len(gone)], np.uint64)))
        elif op[0] == "get":
            k = _u32(op[1])
            nan = np.full(dim, 0x7FC00000, np.uint32).view(F32)
            out.append(dict(rows=np.array([rows.get(int(x), nan) for x in k], F32).reshape(len(k), dim),
                            found=np.array([int(x) in rows for x in k], np.uint8)))
        elif op[0] == "bytes":
            out.append(dict(bytes=np.array([raw[int(x)] for x in _u32(op[1])], np.uint8).reshape(-1, dim)))
        elif op[0] == "info":
            out.append(dict(clamped=np.array([clamped], np.uint64), held=np.array([len(rows)], np.uint64)))
        elif op[0] == "range":
            a, b = np_range(op[1], dim)
            out.append(dict(vmin=a, step=b))
        elif op[0] in ("rerank", "knn"):
            held = np.array(sorted(rows), np.int64)
            dense = np.array([rows[int(k)] for k in held], F32).reshape(len(held), dim)
            q = _vec(op[1], dim)
            if op[0] == "rerank":
                keys, R, counts, values = np.ascontiguousarray(op[2], np.uint32).reshape(len(q), -1), op[3], op[4], op[5]
            else:
                R = op[2]
                passing = held
                if op[3] is not None:
                    listed = np.isin(held, np.asarray(op[4], np.int64))
                    passing = held[listed] if op[3] == 1 else held[~listed]
                keys, counts, values = np.tile(passing.astype(np.uint32), (len(q), 1)), None, None
            if keys.shape[1] == 0:
                r = dict(missing=0, keys=np.full((len(q), R), NO_KEY, np.uint32), dist=np.full((len(q), R), np.inf, F32),
                         sizes=np.zeros(len(q), np.int32))
            else:
                # the held keys, ascending, become the dense range [0, n): a monotone map, so (distance, key) orders alike
                pos = np.searchsorted(held, keys.astype(np.int64))
                hit = (pos < len(held)) & (held[np.minimum(pos, max(len(held) - 1, 0))] == keys if len(held) else False)
                mapped = np.where(hit, pos, len(held)).astype(np.uint32)
                r = rc.np_rerank(rc.case(dim, "f32", [(0, dense)] if len(held) else [], q, mapped, R, counts=counts, values=values))
                back = np.where(r["keys"] == NO_KEY, NO_KEY, held[np.minimum(r["keys"], max(len(held) - 1, 0))] if len(held) else NO_KEY)
                r["keys"] = back.astype(np.uint32)
            res = dict(keys=r["keys"], dist=r["dist"], sizes=r["sizes"])
            if op[0] == "rerank":
                res = dict(missing=np.array([r["missing"]], np.uint64), **res)
            out.append(res)
    return dict(refused=0, ops=out)


# ---- script builders --------------------------------------------------------------------------------------------------------------

def all_keys(lo, n):
    return np.arange(lo, lo + n, dtype=np.uint32)


def grid_script(dim):
    """the exact grid: vmin an integer, step a power of two, inputs on the grid points, between them and on the ties k + 0.5: every
    operation of encode and decode is exact"""
    vmin, step = np.full(dim, -3.0, F32), np.full(dim, 0.25, F32)
    k = np.arange(256, dtype=F32)
    fr = np.array([0.0, 0.25, 0.5, 0.75], F32)
    x = (F32(-3.0) + (k[:, None] + fr[None, :]) * F32(0.25)).reshape(-1)               # 1024 values, exact
    x = x[x <= F32(-3.0) + F32(255.0) * F32(0.25)]                                    # (inside the range: nothing is clamped)
    n = -(-len(x) // dim)
    rng = np.random.default_rng(dim)
    v = np.concatenate([x, rng.choice(x, n * dim - len(x))]).astype(F32).reshape(n, dim)
    return script(dim, "sq8", [("add", 7, v), ("get", all_keys(7, n)), ("bytes", all_keys(7, n)), ("info",)], vmin=vmin, step=step), v


def edge_script(dim, keyed=False):
    """both ends of the range and just outside them, +-inf, NaN of either sign, constant dimensions hit and missed, a subnormal step
    (inv = +inf), -0 against +0"""
    rng = np.random.default_rng(100 + dim)
    vmin = rng.normal(size=dim).astype(F32)
    step = (rng.random(dim).astype(F32) + F32(0.01)) / F32(64.0)
    step[::5] = 0.0                                                                   # constant dimensions
    if dim >= 3:
        step[2] = np.array([3], np.uint32).view(F32)[0]                                 # subnormal: inv = +inf
    if dim >= 8:
        vmin[7], step[7] = 0.0, 0.5                                                   # -0 against a +0 vmin
    with np.errstate(all="ignore"):
        top = vmin + F32(255.0) * step
    specials = [vmin, top, np.nextafter(vmin, F32(-np.inf)), np.nextafter(top, F32(np.inf)), np.nextafter(vmin, F32(np.inf)),
                np.full(dim, np.inf, F32), np.full(dim, -np.inf, F32), np.full(dim, np.nan, F32),
                np.full(dim, 0xFFC00001, np.uint32).view(F32), np.full(dim, -0.0, F32), np.zeros(dim, F32),
                (vmin + step * F32(254.5)).astype(F32), (vmin + step * F32(255.49)).astype(F32)]
    body = (vmin[None, :] + rng.random((12, dim)).astype(F32) * F32(300.0) * step[None, :] - F32(20.0) * step[None, :]).astype(F32)
    v = np.concatenate([np.array(specials, F32), body])
    n = len(v)
    if keyed:
        lab = (rng.permutation(10 * n)[:n] + 5).astype(np.uint32)
        ops = [("put", lab, v), ("get", lab), ("bytes", lab), ("info",)]
    else:
        ops = [("add", 0, v[:9]), ("add", 9, v[9:]), ("get", all_keys(0, n)), ("bytes", all_keys(0, n)), ("info",)]
    return script(dim, "sq8", ops, keyed=keyed, vmin=vmin, step=step)


def range_scripts():
    """range: a column of only NaN and inf, n = 0, one row, -0 against +0, a range that overflows (and the refusal of its store)"""
    rng = np.random.default_rng(5)
    out = []
    for dim in (1, 65, 4096):
        v = rng.normal(size=(1000, dim)).astype(F32)
        v[rng.integers(0, 1000, 40), rng.integers(0, dim, 40)] = np.nan
        v[rng.integers(0, 1000, 40), rng.integers(0, dim, 40)] = np.inf
        v[:, dim // 2] = np.where(np.arange(1000) % 2, np.nan, -np.inf)                 # nothing finite: 0, 0
        out.append(script(dim, "f32", [("range", v), ("range", v[:0]), ("range", v[:1]), ("range", v[:67])]))
    z = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, -0.0], [0.0, 0.0, 0.0]], F32)
    big = np.array([[3e38, 1.0], [-3e38, 2.0]], F32)
    out.append(script(3, "f32", [("range", z)]))
    out.append(script(2, "f32", [("range", big)]))
    return out


def refusal_scripts():
    """parameters no store takes: the overflowed range's step = +inf, a NaN vmin, a negative step"""
    vmin, step = np_range(np.array([[3e38, 1.0], [-3e38, 2.0]], F32), 2)
    assert np.isinf(step[0])
    bad = [(vmin, step), (np.array([np.nan, 0], F32), np.ones(2, F32)), (np.zeros(2, F32), np.array([1.0, -1e-3], F32)),
           (np.array([np.inf, 0], F32), np.ones(2, F32))]
    return [script(2, "sq8", [], keyed=k, vmin=a, step=b) for a, b in bad for k in (False, True)]


def data_params(rng, rows, dim, scale=1.0):
    """random rows and the range of most of them, so that a few components are clamped"""
    v = (rng.normal(size=(rows, dim)) * scale).astype(F32)
    vmin, step = np_range(v[: max(1, rows * 3 // 4)], dim)
    return v, vmin, step


def rerank_script(dim, keyed, r_in, rows=300, nq=4):
    """dense or keyed: missing and duplicate keys, FLT_MAX values, counts, R below and above the survivors, a NaN query and an inf
    query component against finite rows"""
    rng = np.random.default_rng(1000 * r_in + dim + keyed)
    v, vmin, step = data_params(rng, rows, dim)
    q = rng.normal(size=(nq, dim)).astype(F32)
    q[1, 0] = np.nan
    q[2, dim - 1] = np.inf
    if keyed:
        lab = (rng.permutation(8 * rows)[:rows] + 3).astype(np.uint32)
        fill = [("put", lab[:200], v[:200]), ("put", lab[150:], v[150:]), ("remove", lab[10:20])]
    else:
        lab = all_keys(40, rows)
        fill = [("add", 40, v[:120]), ("add", 160, v[120:])]
    keys = lab[rng.integers(0, rows, (nq, r_in))]
    keys[0, :4] = (1, NO_KEY, keys[0, 5], lab[10])                                    # missing (the filler key too), a duplicate
    values = rng.random((nq, r_in)).astype(F32)
    values[3, ::3] = rc.FLT_MAX
    counts = np.array([r_in, r_in, r_in // 2, r_in], np.int32)[:nq]
    ops = fill + [("rerank", q, keys, 5, None, None), ("rerank", q, keys, r_in + 9, counts, values), ("info",)]
    return script(dim, "sq8", ops, keyed=keyed, vmin=vmin, step=step)


def knn_script(dim, keyed, nq, rows=300):
    """every row of the store: no filter, ALLOW and EXCLUDE, R below and above the rows held; a keyed store with free rows"""
    rng = np.random.default_rng(77 * dim + nq + keyed)
    v, vmin, step = data_params(rng, rows, dim)
    q = rng.normal(size=(nq, dim)).astype(F32)
    if keyed:
        lab = (rng.permutation(8 * rows)[:rows] + 3).astype(np.uint32)
        fill = [("put", lab, v), ("remove", lab[::7])]
    else:
        lab = all_keys(11, rows)
        fill = [("add", 11, v)]
    listed = np.concatenate([lab[rng.integers(0, rows, 90)], [2, 5000000]])
    ops = fill + [("knn", q, 10, None, []), ("knn", q, 10, 1, listed), ("knn", q, 33, 0, listed), ("knn", q, rows + 20, None, [])]
    return script(dim, "sq8", ops, keyed=keyed, vmin=vmin, step=step)


def keyed_script(dim):
    """repeated keys within one put (only the winner counts as clamped), overwrite, remove then get"""
    rng = np.random.default_rng(9 + dim)
    v, vmin, step = data_params(rng, 60, dim, scale=2.0)
    v[:, 0] = np.where(np.arange(60) % 2, np.nan, v[:, 0])                            # odd inputs: a clamped component each
    lab = np.array([5, 9, 5, 5, 12, 9, 7, 5] + list(range(100, 152)), np.uint32)      # key 5 four times, key 9 twice
    ops = [("put", lab, v), ("info",), ("get", [5, 9, 12, 7, 6, NO_KEY]), ("bytes", [5, 9, 12, 7]),
           ("put", [9, 100], v[:2]), ("info",), ("remove", [5, 5, 101, 4000]), ("get", [5, 9, 100, 101, 102]), ("info",),
           ("put", [5], v[3:4]), ("get", [5]), ("info",)]
    return script(dim, "sq8", ops, keyed=True, vmin=vmin, step=step)


def plain_get_scripts():
    """get on stores of floats and halves: keys below, inside and above a dense store, the filler key, a keyed store after a remove"""
    rng = np.random.default_rng(3)
    out = []
    for dtype in ("f32", "f16"):
        for dim in (1, 65, 260):
            v = (rng.normal(size=(20, dim)) * 100).astype(F32)
            v[3, 0] = np.nan
            v[4, dim - 1] = 1e6                                                       # +inf as a half
            out.append(script(dim, dtype, [("add", 10, v), ("get", [9, 10, 29, 30, 0, NO_KEY, 13, 14, 13])]))
            out.append(script(dim, dtype, [("put", all_keys(50, 20)[::-1].copy(), v), ("remove", [55]), ("get", [50, 55, 69, 70, NO_KEY, 53])],
                              keyed=True))
    return out


if __name__ == "__main__":                                                            # isolated(): IN OUT, pickled
    with open(sys.argv[1], "rb") as f:
        name, args = pickle.load(f)
    assert np.array([1], np.uint32).view(F32)[0] * F32(2.0) != 0, "subnormals are flushed in a fresh interpreter"
    result = globals()[name](*args)
    with open(sys.argv[2], "wb") as f:
        pickle.dump(result, f)
