"""Shared by the tests of the exhaustive search over a refine store (qadc_refine_knn).  A CASE is a dict
keyed (bool), dim, dtype ("f32" | "f16"), ops — the life of one store as a list of operations

    ("add", first_key, vectors [n][dim])                 a dense store
    ("put", labels uint32 [n], vectors [n][dim])         a keyed store
    ("remove", labels uint32 [n])                        a keyed store
    ("knn", queries [nq][dim], R, filter)                filter: None or (mode "exclude" | "allow", keys uint32 [n])

and three things run cases and return one result per knn operation, to be compared for equality:
  run_twin   refine::knn of quick-adc_amd/host/refine.hpp through tests/cpp/refine_knn_host.cpp; beside it (rr_keys, rr_dist,
             rr_sizes) the twin's rerank fed every held key that passes
  run_numpy  an independent restatement: refine_cases.np_distance over all held rows, the filter applied in numpy
  run_store  pyqadc.Refine on the GPU, through the host form or through torch tensors
A result is a dict keys [nq][R], dist [nq][R], sizes [nq]."""
import os
import subprocess

import numpy as np

import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_knn_host")
NO_KEY = rc.NO_KEY
MODES = {"exclude": 0, "allow": 1}
MAX_R = 1024                 # QADC_REFINE_KNN_MAX_R
CHUNK = 7168                 # the plan's default chunk_rows (host/refine_knn_plan.hpp: kKnnDefaultChunk)
QT, QT_SMALL = 32, 4         # the plan's tiles at dim <= 128: kKnnMaxQt, and kKnnSmallQt for calls of at most 4 queries


def build_driver():
    from test_scanner_hip_cpp import _compile
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def add(first_key, vectors):
    vectors = np.ascontiguousarray(vectors, np.float32)
    return ("add", int(first_key), vectors.reshape(len(vectors), -1))


def put(labels, vectors):
    vectors = np.ascontiguousarray(vectors, np.float32)
    return ("put", np.ascontiguousarray(labels, np.uint32).reshape(-1), vectors.reshape(len(vectors), -1))


def remove(labels):
    return ("remove", np.ascontiguousarray(labels, np.uint32).reshape(-1))


def knn(queries, R, filter=None):
    queries = np.ascontiguousarray(queries, np.float32)
    queries = queries.reshape(1, -1) if queries.ndim == 1 else queries
    if filter is not None:
        filter = (filter[0], np.ascontiguousarray(filter[1], np.uint32).reshape(-1))
    return ("knn", queries, int(R), filter)


def case(keyed, dim, dtype, ops):
    return dict(keyed=bool(keyed), dim=int(dim), dtype=dtype, ops=list(ops))


def from_rerank_case(c, Rs):
    """a case of refine_cases (a dense store and queries) as a knn case: one knn per R of Rs"""
    return case(False, c["dim"], c["dtype"], [add(k, v) for k, v in c["adds"]] + [knn(c["queries"], R) for R in Rs])


def run_twin(exe, tmp_path, cases):
    fin, fout = str(tmp_path / "knn.in"), str(tmp_path / "knn.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            np.array([c["keyed"], c["dim"], rc.DTYPES[c["dtype"]], len(c["ops"])], np.int32).tofile(f)
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
                else:
                    _, q, R, flt = op
                    np.array([3, q.shape[0], R, -1 if flt is None else MODES[flt[0]]], np.int32).tofile(f)
                    np.array([0 if flt is None else len(flt[1])], np.uint64).tofile(f)
                    q.tofile(f)
                    if flt is not None:
                        flt[1].tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        def triple(nq, R):
            return (np.fromfile(f, np.uint32, nq * R).reshape(nq, R), np.fromfile(f, np.float32, nq * R).reshape(nq, R),
                    np.fromfile(f, np.int32, nq))
        for c in cases:
            res = []
            for op in c["ops"]:
                if op[0] == "knn":
                    nq, R = op[1].shape[0], op[2]
                    k, d, s = triple(nq, R)
                    rk, rd, rs = triple(nq, R)
                    res.append(dict(keys=k, dist=d, sizes=s, rr_keys=rk, rr_dist=rd, rr_sizes=rs))
            got.append(res)
        assert f.read() == b""
    return got


def held_rows(c, upto=None):
    """(keys uint32 ascending, rows float32 as the store holds them) after the first `upto` operations"""
    held = {}
    for op in c["ops"][:upto]:
        if op[0] in ("add", "put"):
            rows = op[2]
            if c["dtype"] == "f16":
                with np.errstate(over="ignore"):
                    rows = rows.astype(np.float16).astype(np.float32)
            labels = op[1] if op[0] == "put" else np.arange(op[1], op[1] + len(rows))
            for lab, row in zip(np.asarray(labels).tolist(), rows):
                held[lab] = row
        elif op[0] == "remove":
            for lab in op[1].tolist():
                held.pop(lab, None)
    keys = np.array(sorted(held), np.uint32)
    rows = np.stack([held[int(k)] for k in keys]) if len(keys) else np.zeros((0, c["dim"]), np.float32)
    return keys, rows


def np_knn(keys, rows, queries, R, flt):
    if flt is not None:
        keep = np.isin(keys, flt[1]) == (flt[0] == "allow")
        keys, rows = keys[keep], rows[keep]
    nq = queries.shape[0]
    out = dict(keys=np.full((nq, R), NO_KEY, np.uint32), dist=np.full((nq, R), np.inf, np.float32), sizes=np.zeros(nq, np.int32))
    if len(keys) == 0:
        return out
    for q in range(nq):
        d = rc.np_distance(queries[q], rows)
        img = d.view(np.uint32).astype(np.uint64)
        img[np.isnan(d)] = rc.NAN_IMAGE
        words = np.sort((img << np.uint64(32)) | keys.astype(np.uint64))[:R]
        n = len(words)
        out["keys"][q, :n] = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out["dist"][q, :n] = (words >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out["sizes"][q] = n
    return out


def run_numpy(c):
    got = []
    for i, op in enumerate(c["ops"]):
        if op[0] == "knn":
            keys, rows = held_rows(c, i)
            got.append(np_knn(keys, rows, op[1], op[2], op[3]))
    return got


def make_store(pyqadc, c):
    return pyqadc.Refine(c["dim"], c["dtype"], keyed=c["keyed"])


def run_store(pyqadc, c, device=False, plan=None, device_filter=False, st=None):
    """the case on a pyqadc.Refine (a new one, closed at the end, unless `st` is given); device: knn_device on torch tensors;
    plan: (chunk_rows, pass_nq) for set_knn_plan; device_filter: the filters through AdcFilter.from_device"""
    own = st is None
    if own:
        st = make_store(pyqadc, c)
    if plan is not None:
        st.set_knn_plan(*plan)
    if device or device_filter:
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
        else:
            _, q, R, flt = op
            f = None
            if flt is not None:
                f = pyqadc.AdcFilter.from_device(dev(flt[1]), flt[0]) if device_filter else pyqadc.AdcFilter(flt[1], flt[0], device=st.device)
            if device:
                k, d, s = st.knn_device(dev(q), R, filter=f)
                k, d, s = k.cpu().numpy().view(np.uint32), d.cpu().numpy(), s.cpu().numpy()
            else:
                k, d, s = st.knn(q, R, filter=f)
            if f is not None:
                f.close()
            got.append(dict(keys=k, dist=d, sizes=s))
    if own:
        st.close()
    return got


def same(a, b):
    """None where two results agree bit for bit, else what differs"""
    for name in ("sizes", "keys"):
        if not np.array_equal(a[name], b[name]):
            return name
    if not np.array_equal(a["dist"].view(np.uint32), b["dist"].view(np.uint32)):
        return "dist"
    return None


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        diff = same(g, w)
        assert diff is None, "%s knn %d: %s differs" % (what, i, diff)


def tie_case(rng, dim, dtype, R, lo=50, rows=40):
    """ten identical rows under the keys lo + 10 .. lo + 19, all at distance 0 from query 0: its first ten results, by key, so R = 5
    cuts the tie, R = 10 ends with it and R = 11 goes one past it"""
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[10:20] = vec[10]
    q = rng.normal(size=(3, dim)).astype(np.float32)
    q[0] = vec[10]
    return case(False, dim, dtype, [add(lo, vec), knn(q, R), knn(q, 5), knn(q, 10), knn(q, 11)])
