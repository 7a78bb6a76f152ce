"""Shared by the tests of the exact range search over a refine store (qadc_refine_range, qadc_refine_rerank_range; DESIGN.md section
11.21).  A CASE is a dict keyed (bool), dim, dtype ("f32" | "f16" | "sq8"), vmin, step (sq8) and ops — the life of one store:

    ("add", first_key, vectors [n][dim])                 a dense store
    ("put", labels uint32 [n], vectors [n][dim])         a keyed store
    ("remove", labels uint32 [n])                        a keyed store
    ("range", queries [nq][dim], radius [nq], filter)    filter: None or (mode "exclude" | "allow", keys uint32 [n])
    ("rerank_range", queries [nq][dim], in_lims uint64 [nq + 1], keys uint32 [in_lims[nq]], radius [nq])

and three things run cases and return one result per range / rerank_range operation, to be compared for equality:
  run_twin   refine::range / refine::rerank_range of quick-adc_amd/host/refine.hpp through tests/cpp/refine_range_host.cpp, with the
             driver's cross-checks beside them (xr_*: rerank_range of every held key; knn_* / rr_*: the twin's knn and rerank)
  run_numpy  an independent restatement: refine_cases.np_distance over the held rows, the filter in numpy, a float compare with the
             radius, a sort of the words
  run_store  pyqadc.Refine on the GPU, through the host form or through torch tensors
A result is a dict lims uint64 [nq + 1], keys uint32, dist float32, missing."""
import os
import subprocess

import numpy as np

import refine_cases as rc
import refine_sq_cases as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_range_host")
DTYPES = sq.DTYPES
MODES = {"exclude": 0, "allow": 1}
NO_KEY = rc.NO_KEY
F32 = np.float32
INF = F32(np.inf)
FLT_MAX = rc.FLT_MAX
SUBNORMAL = np.array([1], np.uint32).view(F32)[0]
REGION = 4096                # the plan's default region (host/refine_range_plan.hpp: kRangeDefaultRegion)
SORT_LDS = 4096              # kRangeSortLds: longer segments take the radix passes
CHUNK = 7168                 # kRangeDefaultChunk
GROUPS = 8                   # kKnnMaxGroups: a launch walks GROUPS * CHUNK rows


def build_driver():
    from test_scanner_hip_cpp import _compile
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def _vec(v, dim=None):
    v = np.ascontiguousarray(v, F32)
    return v.reshape(len(v), -1) if dim is None else v.reshape(-1, dim)


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, np.uint64).astype(np.uint32)).reshape(-1)


def add(first_key, vectors):
    return ("add", int(first_key), _vec(vectors))


def put(labels, vectors):
    return ("put", _u32(labels), _vec(vectors))


def remove(labels):
    return ("remove", _u32(labels))


def _radius(radius, nq):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(radius, F32), (nq,)), F32)


def range_(queries, radius, filter=None):
    q = np.ascontiguousarray(queries, F32)
    q = q.reshape(1, -1) if q.ndim == 1 else q
    if filter is not None:
        filter = (filter[0], _u32(filter[1]))
    return ("range", q, _radius(radius, len(q)), filter)


def rerank_range(queries, segments, radius):
    """segments: one key list per query"""
    q = np.ascontiguousarray(queries, F32)
    q = q.reshape(1, -1) if q.ndim == 1 else q
    assert len(segments) == len(q)
    lims = np.zeros(len(q) + 1, np.uint64)
    lims[1:] = np.cumsum([len(s) for s in segments])
    keys = np.concatenate([_u32(s) for s in segments]) if len(segments) else np.zeros(0, np.uint32)
    return ("rerank_range", q, lims, keys, _radius(radius, len(q)))


def case(keyed, dim, dtype, ops, vmin=None, step=None):
    c = dict(keyed=bool(keyed), dim=int(dim), dtype=dtype, ops=list(ops), vmin=None, step=None)
    if dtype == "sq8":
        c["vmin"], c["step"] = np.ascontiguousarray(vmin, F32).reshape(dim), np.ascontiguousarray(step, F32).reshape(dim)
    return c


def sq_params(vectors):
    """a range for SQ8 rows whose steps are normal numbers: the restatement then needs no subnormal arithmetic"""
    v = _vec(vectors)
    fin = np.where(np.isfinite(v), v, F32(0))
    vmin = fin.min(axis=0).astype(F32)
    step = np.maximum((fin.max(axis=0) - vmin) / F32(255), F32(1e-3)).astype(F32)
    return vmin, step


def dense_case(dim, dtype, lo, vectors, ops):
    vmin, step = sq_params(vectors) if dtype == "sq8" else (None, None)
    return case(False, dim, dtype, [add(lo, vectors)] + list(ops), vmin, step)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------

def run_twin(exe, tmp_path, cases):
    fin, fout = str(tmp_path / "range.in"), str(tmp_path / "range.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            np.array([c["keyed"], c["dim"], DTYPES[c["dtype"]], len(c["ops"])], np.int32).tofile(f)
            if c["dtype"] == "sq8":
                c["vmin"].tofile(f)
                c["step"].tofile(f)
            for op in c["ops"]:
                if op[0] == "add":
                    np.array([0], np.int32).tofile(f)
                    np.array([op[1], len(op[2])], np.uint32).tofile(f)
                    op[2].tofile(f)
                elif op[0] == "put":
                    np.array([1], np.int32).tofile(f)
                    np.array([len(op[1])], np.uint64).tofile(f)
                    op[1].tofile(f)
                    op[2].tofile(f)
                elif op[0] == "remove":
                    np.array([2], np.int32).tofile(f)
                    np.array([len(op[1])], np.uint64).tofile(f)
                    op[1].tofile(f)
                elif op[0] == "range":
                    _, q, radius, flt = op
                    np.array([3, q.shape[0], -1 if flt is None else MODES[flt[0]]], np.int32).tofile(f)
                    np.array([0 if flt is None else len(flt[1])], np.uint64).tofile(f)
                    q.tofile(f)
                    radius.tofile(f)
                    if flt is not None:
                        flt[1].tofile(f)
                else:
                    _, q, lims, keys, radius = op
                    np.array([4, q.shape[0]], np.int32).tofile(f)
                    lims.tofile(f)
                    q.tofile(f)
                    radius.tofile(f)
                    keys.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        def csr(nq):
            lims = np.fromfile(f, np.uint64, nq + 1)
            n = int(lims[-1])
            return lims, np.fromfile(f, np.uint32, n), np.fromfile(f, F32, n)

        def rect(nq):
            R = int(np.fromfile(f, np.int32, 1)[0])
            return (np.fromfile(f, np.uint32, nq * R).reshape(nq, R), np.fromfile(f, F32, nq * R).reshape(nq, R), np.fromfile(f, np.int32, nq))
        for c in cases:
            res = []
            for op in c["ops"]:
                if op[0] not in ("range", "rerank_range"):
                    continue
                nq = op[1].shape[0]
                lims, keys, dist = csr(nq)
                r = dict(lims=lims, keys=keys, dist=dist, missing=0)
                if op[0] == "range":
                    xl, xk, xd = csr(nq)
                    r.update(xr=dict(lims=xl, keys=xk, dist=xd, missing=int(np.fromfile(f, np.uint64, 1)[0])))
                    r["knn_keys"], r["knn_dist"], r["knn_sizes"] = rect(nq)
                else:
                    r["missing"] = int(np.fromfile(f, np.uint64, 1)[0])
                    r["rr_keys"], r["rr_dist"], r["rr_sizes"] = rect(nq)
                    r["rr_missing"] = int(np.fromfile(f, np.uint64, 1)[0])
                res.append(r)
            got.append(res)
        assert f.read() == b""
    return got


# ---- the numpy restatement --------------------------------------------------------------------------------------------------------

def held_rows(c, upto=None):
    """(keys uint32 ascending, rows float32 as the store reads them) after the first `upto` operations"""
    held = {}
    for op in c["ops"][:upto]:
        if op[0] in ("add", "put"):
            rows = sq._convert(c, op[2])[0]
            labels = op[1] if op[0] == "put" else np.arange(op[1], op[1] + len(rows))
            for lab, row in zip(np.asarray(labels).tolist(), rows):
                held[lab] = row
        elif op[0] == "remove":
            for lab in op[1].tolist():
                held.pop(lab, None)
    keys = np.array(sorted(held), np.uint32)
    rows = np.stack([held[int(k)] for k in keys]) if len(keys) else np.zeros((0, c["dim"]), F32)
    return keys, rows


def np_words(q, radius, keys, rows):
    """the sorted words of the rows (keys unique) whose distance to q is < radius"""
    if len(keys) == 0:
        return np.zeros(0, np.uint64)
    d = rc.np_distance(q, rows)
    with np.errstate(invalid="ignore"):
        keep = d < radius                                  # a float32 compare: NaN on either side is False
    assert d.dtype == F32 and np.asarray(radius).dtype == F32
    return np.sort((d[keep].view(np.uint32).astype(np.uint64) << np.uint64(32)) | keys[keep].astype(np.uint64))


def _result(words_per_query, missing=0):
    lims = np.zeros(len(words_per_query) + 1, np.uint64)
    lims[1:] = np.cumsum([len(w) for w in words_per_query])
    w = np.concatenate(words_per_query) if len(words_per_query) else np.zeros(0, np.uint64)
    return dict(lims=lims, keys=(w & np.uint64(0xFFFFFFFF)).astype(np.uint32), dist=(w >> np.uint64(32)).astype(np.uint32).view(F32),
                missing=missing)


def np_range(keys, rows, queries, radius, flt):
    if flt is not None:
        keep = np.isin(keys, flt[1]) == (flt[0] == "allow")
        keys, rows = keys[keep], rows[keep]
    return _result([np_words(queries[q], radius[q], keys, rows) for q in range(len(queries))])


def np_rerank_range(keys, rows, queries, lims, cand, radius):
    out, missing = [], 0
    for q in range(len(queries)):
        k = cand[int(lims[q]):int(lims[q + 1])]
        held = np.isin(k, keys)
        missing += int((~held).sum())
        k = np.unique(k[held])
        out.append(np_words(queries[q], radius[q], k, rows[np.searchsorted(keys, k)]))
    return _result(out, missing)


def run_numpy(c):
    got = []
    for i, op in enumerate(c["ops"]):
        if op[0] == "range":
            keys, rows = held_rows(c, i)
            got.append(np_range(keys, rows, op[1], op[2], op[3]))
        elif op[0] == "rerank_range":
            keys, rows = held_rows(c, i)
            got.append(np_rerank_range(keys, rows, op[1], op[2], op[3], op[4]))
    return got


# ---- the GPU ----------------------------------------------------------------------------------------------------------------------

def make_store(pyqadc, c):
    if c["dtype"] == "sq8":
        return pyqadc.Refine(c["dim"], "sq8", keyed=c["keyed"], vmin=c["vmin"], step=c["step"])
    return pyqadc.Refine(c["dim"], c["dtype"], keyed=c["keyed"])


def run_store(pyqadc, c, device=False, plan=None, st=None, reruns=None):
    """the case on a pyqadc.Refine (a new one, closed at the end, unless `st` is given); device: the _device forms on torch tensors;
    plan: (region_rows, chunk_rows, pass_nq) for set_range_plan; reruns: a list that gets range_reruns() after every operation"""
    own = st is None
    if own:
        st = make_store(pyqadc, c)
    if plan is not None:
        st.set_range_plan(*plan)
    if device:
        import torch

        def dev(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:%d" % st.device)
    got = []
    for op in c["ops"]:
        if op[0] == "add":
            st.add(op[2], op[1])
        elif op[0] == "put":
            st.put(op[2], op[1])
        elif op[0] == "remove":
            st.remove(op[1])
        elif op[0] == "range":
            _, q, radius, flt = op
            f = None if flt is None else pyqadc.AdcFilter(flt[1], flt[0], device=st.device)
            if device:
                lims, k, d = st.range_device(dev(q), radius, filter=f)
                k, d = k.cpu().numpy().view(np.uint32), d.cpu().numpy()
            else:
                lims, k, d = st.range(q, radius, filter=f)
            if f is not None:
                f.close()
            got.append(dict(lims=lims.astype(np.uint64), keys=k, dist=d, missing=0))
        else:
            _, q, lims, keys, radius = op
            if device:
                ol, k, d, missing = st.rerank_range_device(dev(q), lims, dev(keys), radius)
                k, d = k.cpu().numpy().view(np.uint32), d.cpu().numpy()
            else:
                ol, k, d, missing = st.rerank_range(q, lims, keys, radius)
            got.append(dict(lims=ol.astype(np.uint64), keys=k, dist=d, missing=missing))
        if reruns is not None and op[0] in ("range", "rerank_range"):
            reruns.append(st.range_reruns())
    if own:
        st.close()
    return got


def same(a, b):
    """None where two results agree bit for bit, else what differs"""
    for name in ("lims", "keys"):
        if not np.array_equal(np.asarray(a[name]).astype(np.uint64), np.asarray(b[name]).astype(np.uint64)):
            return name
    if not np.array_equal(np.ascontiguousarray(a["dist"], F32).view(np.uint32), np.ascontiguousarray(b["dist"], F32).view(np.uint32)):
        return "dist"
    if a["missing"] != b["missing"]:
        return "missing %d != %d" % (a["missing"], b["missing"])
    return None


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        diff = same(g, w)
        assert diff is None, "%s operation %d: %s differs" % (what, i, diff)


def kept(result):
    return np.diff(result["lims"].astype(np.int64))


def radius_keeping(result_inf, q, count, strict=True):
    """a radius under which query q keeps exactly `count` rows, from a radius +inf result with distinct finite distances there: the
    distance of its row number `count` (not kept itself), or +inf to keep all.  strict=False: ties are allowed (fewer rows are kept)"""
    lo, hi = int(result_inf["lims"][q]), int(result_inf["lims"][q + 1])
    d = result_inf["dist"][lo:hi]
    if count >= len(d):
        return INF
    assert not strict or count == 0 or d[count - 1] < d[count]
    return d[count]
