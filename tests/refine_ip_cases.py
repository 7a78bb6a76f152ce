"""Shared by the tests of the inner-product metric on a refine store (qadc_refine_set_metric).  A CASE is
the contents of one store and what is asked of it: a dict keyed (bool), dim, dtype ("f32" | "f16" | "sq8"), vmin, step (sq8), lo,
labels uint32 [n] (dense: lo + arange(n); keyed: any, the last of equal labels wins), vectors [n][dim], ops — a list of

    ("rerank", metric, queries [nq][dim], keys uint32 [nq][r_in], R, counts int32 [nq] | None, values [nq][r_in] | None)
    ("knn",    metric, queries [nq][dim], R, filter)                            filter: None or ("exclude" | "allow", keys uint32 [n])
    ("probed", metric, parts [uint32 labels], assign int32 [nq][ma], queries [nq][dim], R, filter)

with metric "l2" or "ip" per operation, so that one store answers under both.  Three things run a case and return one result per
operation — a dict keys [nq][R], dist [nq][R], sizes [nq], missing — to be compared for equality, bit for bit:
  run_twin   refine::rerank, ::knn and ::knn_probed of quick-adc_amd/host/refine.hpp through tests/cpp/refine_ip_host.cpp
  run_numpy  an independent restatement of the definition: strips of 64, the tree, the image, a sort of words
  run_store  pyqadc.Refine on the GPU, through the host forms or through torch tensors"""
import os
import subprocess

import numpy as np

import refine_cases as rc
import refine_sq_cases as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_ip_host")
F32 = np.float32
NO_KEY = rc.NO_KEY
FLT_MAX = rc.FLT_MAX
DTYPES = sq.DTYPES
METRICS = {"l2": 0, "ip": 1}
MODES = {"exclude": 0, "allow": 1}
KINDS = {"rerank": 0, "knn": 1, "probed": 2}
NAN_IMAGE_IP = 0xFFC00000            # every NaN score, behind -inf's image
NEG_INF_BITS = 0xFF800000            # the score behind out_sizes[q] under "ip"
NAN_BITS = 0x7FC00000                # how a NaN score comes out
DIMS = (1, 63, 64, 65, 128, 4096)
MAX_R = 1024                         # QADC_REFINE_KNN_MAX_R


def build_driver():
    """the driver, compiled where it is missing or older than its sources (seven test modules ask for it)"""
    from test_scanner_hip_cpp import _compile
    sources = (EXE + ".cpp", os.path.join(ROOT, "quick-adc_amd", "host", "refine.hpp"))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in sources):
        _compile(EXE + ".cpp", EXE, link=False)
    return EXE


# ---- cases ----------------------------------------------------------------------------------------------------------------------

def _filter(f):
    return None if f is None else (f[0], np.ascontiguousarray(np.asarray(f[1], np.uint64).astype(np.uint32)).reshape(-1))


def rerank(metric, queries, keys, R, counts=None, values=None):
    queries = np.ascontiguousarray(queries, F32)
    queries = queries.reshape(1, -1) if queries.ndim == 1 else queries
    keys = np.ascontiguousarray(np.asarray(keys, np.uint64).astype(np.uint32)).reshape(queries.shape[0], -1)
    return ("rerank", metric, queries, keys, int(R), None if counts is None else np.ascontiguousarray(counts, np.int32),
            None if values is None else np.ascontiguousarray(values, F32).reshape(keys.shape))


def knn(metric, queries, R, filter=None):
    queries = np.ascontiguousarray(queries, F32)
    return ("knn", metric, queries.reshape(1, -1) if queries.ndim == 1 else queries, int(R), _filter(filter))


def probed(metric, parts, assign, queries, R, filter=None):
    queries = np.ascontiguousarray(queries, F32)
    queries = queries.reshape(1, -1) if queries.ndim == 1 else queries
    parts = [np.ascontiguousarray(np.asarray(p, np.uint64).astype(np.uint32)).reshape(-1) for p in parts]
    return ("probed", metric, parts, np.ascontiguousarray(assign, np.int32).reshape(queries.shape[0], -1), queries, int(R), _filter(filter))


def case(dim, dtype, vectors, ops, lo=0, labels=None, vmin=None, step=None):
    """labels None: a dense store over lo ..; else a keyed store"""
    vectors = np.ascontiguousarray(vectors, F32).reshape(-1, dim)
    keyed = labels is not None
    labels = (np.arange(len(vectors), dtype=np.uint64) + np.uint64(lo)).astype(np.uint32) if labels is None else \
        np.ascontiguousarray(np.asarray(labels, np.uint64).astype(np.uint32)).reshape(-1)
    assert len(labels) == len(vectors)
    c = dict(keyed=keyed, dim=int(dim), dtype=dtype, lo=int(lo), labels=labels, vectors=vectors, ops=list(ops), vmin=None, step=None)
    if dtype == "sq8":
        if vmin is None:
            vmin, step = sq_params(vectors)
        c["vmin"], c["step"] = np.ascontiguousarray(vmin, F32).reshape(dim), np.ascontiguousarray(step, F32).reshape(dim)
    return c


def sq_params(vec):
    """a range that holds every finite component of vec"""
    fin = np.where(np.isfinite(vec), vec, F32(0.0)) if len(vec) else np.zeros((1, vec.shape[1]), F32)
    lo, hi = fin.min(axis=0).astype(F32), fin.max(axis=0).astype(F32)
    return lo, ((hi - lo) / F32(255.0)).astype(F32)


def op_shape(op):
    """(nq, R) of an operation"""
    return (op[2].shape[0], op[4]) if op[0] == "rerank" else (op[2].shape[0], op[3]) if op[0] == "knn" else (op[4].shape[0], op[5])


# ---- the twin -------------------------------------------------------------------------------------------------------------------

def _write_filter_keys(f, flt):
    if flt is not None:
        flt[1].tofile(f)


def run_twin(exe, tmp_path, cases):
    fin, fout = str(tmp_path / "ip.in"), str(tmp_path / "ip.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            np.array([c["keyed"], c["dim"], DTYPES[c["dtype"]], len(c["ops"])], np.int32).tofile(f)
            np.array([c["lo"]], np.uint32).tofile(f)
            np.array([len(c["vectors"])], np.uint64).tofile(f)
            if c["dtype"] == "sq8":
                c["vmin"].tofile(f)
                c["step"].tofile(f)
            if c["keyed"]:
                c["labels"].tofile(f)
            c["vectors"].tofile(f)
            for op in c["ops"]:
                np.array([KINDS[op[0]], METRICS[op[1]]], np.int32).tofile(f)
                if op[0] == "rerank":
                    _, _, q, keys, R, counts, values = op
                    np.array([q.shape[0], keys.shape[1], R, counts is not None, values is not None], np.int32).tofile(f)
                    q.tofile(f)
                    keys.tofile(f)
                    if counts is not None:
                        counts.tofile(f)
                    if values is not None:
                        values.tofile(f)
                elif op[0] == "knn":
                    _, _, q, R, flt = op
                    np.array([q.shape[0], R, -1 if flt is None else MODES[flt[0]]], np.int32).tofile(f)
                    np.array([0 if flt is None else len(flt[1])], np.uint64).tofile(f)
                    q.tofile(f)
                    _write_filter_keys(f, flt)
                else:
                    _, _, parts, assign, q, R, flt = op
                    np.array([q.shape[0], R, -1 if flt is None else MODES[flt[0]], assign.shape[1], len(parts)], np.int32).tofile(f)
                    np.array([0 if flt is None else len(flt[1])], np.uint64).tofile(f)
                    for p in parts:
                        np.array([len(p)], np.uint64).tofile(f)
                        p.tofile(f)
                    assign.tofile(f)
                    q.tofile(f)
                    _write_filter_keys(f, flt)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        for c in cases:
            res = []
            for op in c["ops"]:
                nq, R = op_shape(op)
                missing = int(np.fromfile(f, np.uint64, 1)[0])
                res.append(dict(missing=missing, keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R),
                                dist=np.fromfile(f, F32, nq * R).reshape(nq, R), sizes=np.fromfile(f, np.int32, nq)))
            got.append(res)
        assert f.read() == b""
    return got


def twin_images(exe, tmp_path, bits):
    """(img_ip, bits of img_ip_inverse(img_ip)) of the bit patterns, by the twin"""
    fin, fout = str(tmp_path / "img.in"), str(tmp_path / "img.out")
    np.ascontiguousarray(bits, np.uint32).tofile(fin)
    out = subprocess.run([exe, "--images", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    both = np.fromfile(fout, np.uint32)
    return both[:len(bits)], both[len(bits):]


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------

def held_rows(c):
    """(keys uint32 ascending, rows float32 [n][dim] as the store's arithmetic reads them)"""
    v = c["vectors"]
    if c["dtype"] == "sq8":
        v = sq.np_decode(sq.np_encode(v, c["vmin"], c["step"])[0], c["vmin"], c["step"])
    elif c["dtype"] == "f16":
        with np.errstate(over="ignore"):
            v = v.astype(np.float16).astype(F32)
    last = {int(k): i for i, k in enumerate(c["labels"].tolist())}              # (the last of equal labels wins)
    keys = np.array(sorted(last), np.uint32)
    rows = v[[last[int(k)] for k in keys]] if len(keys) else np.zeros((0, c["dim"]), F32)
    return keys, rows


def np_fold(terms):
    """terms [n][dim] float32 -> the definition's sum of every row: 64 strided partial sums from +0, then the six halvings"""
    n, dim = terms.shape
    with np.errstate(all="ignore"):
        strips = np.concatenate([terms, np.zeros((n, -dim % 64), F32)], axis=1).reshape(n, -1, 64)   # (a p is never -0: p + (+0) is p)
        p = np.zeros((n, 64), F32)
        for j in range(strips.shape[1]):
            p = p + strips[:, j, :]
        for s in (32, 16, 8, 4, 2, 1):
            p = p[:, :s] + p[:, s:2 * s]
    assert p.dtype == F32
    return p[:, 0]


def np_score(q, X):
    with np.errstate(all="ignore"):
        m = q[None, :].astype(F32) * X.astype(F32)
    assert m.dtype == F32
    return np_fold(m)


def np_img_ip(s):
    b = np.ascontiguousarray(s, F32).view(np.uint32)
    img = np.where((b & np.uint32(0x80000000)) != 0, b, ~b & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    img[np.isnan(s)] = NAN_IMAGE_IP
    return img


def np_img_ip_inverse(img):
    img = np.ascontiguousarray(img, np.uint32)
    b = np.where((img & np.uint32(0x80000000)) != 0, img, ~img & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    b[img > np.uint32(NEG_INF_BITS)] = NAN_BITS
    return b


def np_select(metric, query, keys, rows, entries, R):
    """entries: int64 keys, held or not, repeated or not -> (keys [R], dist bits [R], size, missing)"""
    ok = np.full(R, NO_KEY, np.uint32)
    od = np.full(R, NEG_INF_BITS if metric == "ip" else 0x7F800000, np.uint32)
    held = np.isin(entries, keys)
    at = np.searchsorted(keys, entries[held])
    missing = int((~held).sum())
    at = np.unique(at)
    if len(at) == 0:
        return ok, od, 0, missing
    if metric == "ip":
        img = np_img_ip(np_score(query, rows[at])).astype(np.uint64)
    else:
        d = rc.np_distance(query, rows[at])
        img = d.view(np.uint32).astype(np.uint64)
        img[np.isnan(d)] = rc.NAN_IMAGE
    words = np.sort((img << np.uint64(32)) | keys[at].astype(np.uint64))[:R]
    n = len(words)
    ok[:n] = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    high = (words >> np.uint64(32)).astype(np.uint32)
    od[:n] = np_img_ip_inverse(high) if metric == "ip" else high
    return ok, od, n, missing


def _passes(keys, flt):
    return np.ones(len(keys), bool) if flt is None else (np.isin(keys, flt[1]) == (flt[0] == "allow"))


def run_numpy(c):
    keys, rows = held_rows(c)
    got = []
    for op in c["ops"]:
        nq, R = op_shape(op)
        res = dict(keys=np.zeros((nq, R), np.uint32), dist=np.zeros((nq, R), F32), sizes=np.zeros(nq, np.int32), missing=0)
        for q in range(nq):
            if op[0] == "rerank":
                _, metric, queries, cand, _, counts, values = op
                count = cand.shape[1] if counts is None else int(counts[q])
                e = cand[q, :count].astype(np.int64)
                if values is not None:
                    e = e[values[q, :count] != FLT_MAX]
            elif op[0] == "knn":
                _, metric, queries, _, flt = op
                e = keys[_passes(keys, flt)].astype(np.int64)
            else:
                _, metric, parts, assign, queries, _, flt = op
                probes = []
                for p in assign[q].tolist():
                    if 0 <= p < len(parts) and p not in probes:
                        probes.append(p)
                e = np.concatenate([parts[p] for p in probes] + [np.zeros(0, np.uint32)])
                e = e[_passes(e, flt)].astype(np.int64)
            k, d, n, m = np_select(metric, queries[q], keys.astype(np.int64), rows, e, R)
            res["keys"][q], res["sizes"][q] = k, n
            res["dist"][q] = d.view(F32)
            res["missing"] += m
        got.append(res)
    return got


same = rc.same


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        diff = same(g, w)
        assert diff is None, "%s operation %d: %s differs" % (what, i, diff)


# ---- the GPU --------------------------------------------------------------------------------------------------------------------

def make_store(pyqadc, c, metric="l2"):
    st = pyqadc.Refine(c["dim"], c["dtype"], keyed=c["keyed"], vmin=c["vmin"], step=c["step"], metric=metric)
    if len(c["vectors"]):
        if c["keyed"]:
            st.put(c["vectors"], c["labels"])
        else:
            st.add(c["vectors"], c["lo"])
    return st


def make_index(pyqadc, parts, seed=0):
    """an owned 8-bit AdcIndex whose partitions hold random codes and the labels of `parts`"""
    rng = np.random.default_rng(seed)
    idx = pyqadc.AdcIndex(8, 8)
    idx.add_partitions([rng.integers(0, 256, (len(p), 8), dtype=np.uint8) for p in parts], list(parts))
    return idx


def run_store(pyqadc, c, device=False, plan=None, st=None, index_of=make_index):
    """the case on a pyqadc.Refine (a new one, closed at the end, unless `st` is given); device: the _device forms on torch tensors;
    plan: (chunk_rows, pass_nq) for set_knn_plan; index_of(pyqadc, parts) -> the index of a probed operation (closed after it)"""
    own = st is None
    if own:
        st = make_store(pyqadc, c)
    if plan is not None:
        st.set_knn_plan(*plan)
    if device:
        import torch

        def dev(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:%d" % st.device)

        def host(k, d, s):
            return k.cpu().numpy().view(np.uint32), d.cpu().numpy(), s.cpu().numpy()
    got = []
    try:
        for op in c["ops"]:
            st.set_metric(op[1])
            assert st.metric == op[1]
            flt = op[-1] if op[0] != "rerank" else None
            f = None if flt is None else pyqadc.AdcFilter(flt[1], flt[0], device=st.device)
            m = 0
            try:
                if op[0] == "rerank":
                    _, _, q, keys, R, counts, values = op
                    if device:
                        k, d, s, m = st.rerank_device(dev(q), dev(keys), R, counts=dev(counts), values=dev(values))
                        k, d, s = host(k, d, s)
                    else:
                        k, d, s, m = st.rerank(q, keys, R, counts=counts, values=values)
                elif op[0] == "knn":
                    _, _, q, R, _ = op
                    if device:
                        k, d, s = host(*st.knn_device(dev(q), R, filter=f))
                    else:
                        k, d, s = st.knn(q, R, filter=f)
                else:
                    _, _, parts, assign, q, R, _ = op
                    idx = index_of(pyqadc, parts)
                    try:
                        if device:
                            k, d, s, m = st.knn_probed_device(idx, dev(q), dev(assign), R, filter=f)
                            k, d, s = host(k, d, s)
                        else:
                            k, d, s, m = st.knn_probed(idx, q, assign, R, filter=f)
                    finally:
                        idx.close()
            finally:
                if f is not None:
                    f.close()
            got.append(dict(keys=k, dist=d, sizes=s, missing=m))
    finally:
        if own:
            st.close()
    return got


# ---- case builders --------------------------------------------------------------------------------------------------------------

def bits(*patterns):
    return np.array(patterns, np.uint32).view(F32)


def every_key(c_keys, nq):
    return np.tile(np.asarray(c_keys, np.uint32), (nq, 1))


def split(labels, sizes):
    cuts = np.cumsum((0,) + tuple(sizes))
    assert cuts[-1] == len(labels)
    return [labels[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def three_ops(metric, q, keys, R, parts=None, flt=None):
    """rerank fed every key, knn, and knn_probed at ma = K with the keys as labels: the same selection three ways"""
    nq = q.shape[0]
    parts = split(np.asarray(keys, np.uint32), (len(keys) // 3, 0, len(keys) - len(keys) // 3)) if parts is None else parts
    assign = np.tile(np.arange(len(parts), dtype=np.int32), (nq, 1))
    return [rerank(metric, q, every_key(keys, nq), R), knn(metric, q, R, flt), probed(metric, parts, assign, q, R, flt)]


def random_case(rng, dim, dtype, keyed, rows=120, nq=3, lo=40, scale=1.0):
    """rows and queries of both signs; rerank with repeated, missing and skipped entries; knn; knn_probed; each under both metrics"""
    vec = (rng.normal(size=(rows, dim)) * scale).astype(F32)
    q = (rng.normal(size=(nq, dim)) * scale).astype(F32)
    labels = (rng.permutation(4 * rows)[:rows] + lo).astype(np.uint32) if keyed else None
    keys = np.sort(labels) if keyed else np.arange(lo, lo + rows, dtype=np.uint32)
    r_in = 48
    cand = keys[rng.integers(0, rows, (nq, r_in))].copy()
    cand[0, 3] = cand[0, 4]                                                    # a key twice
    cand[1, 5:8] = (0xFFFFFFFF, lo - 1, int(keys.max()) + 1)                   # missing
    values = rng.random((nq, r_in)).astype(F32)
    values[2, 10:14] = FLT_MAX                                                 # skipped
    counts = np.full(nq, r_in, np.int32)
    counts[nq - 1] = r_in // 2
    ops = []
    for metric in ("ip", "l2"):
        ops += [rerank(metric, q, cand, 10, counts, values), rerank(metric, q, cand, r_in + 3)]
        for R in (1, rows - 1, rows + 5):
            ops += three_ops(metric, q, keys, R)
        some = rng.choice(keys, rows // 2, replace=False)
        ops += [knn(metric, q, 20, ("allow", some)), knn(metric, q, 20, ("exclude", some))]
    return case(dim, dtype, vec, ops, lo=lo, labels=labels)


def sign_case(dtype, keyed=False, dim=3):
    """scores 3, 2, 1, +0, +0, -1, -2, -3 (and their halves) in one query: R cuts at a positive, a zero and a negative score"""
    vec = np.zeros((8, dim), F32)
    vec[:, 0] = (3, -1, 0, 2, -3, 1, 0, -2)
    q = np.zeros((2, dim), F32)
    q[0, 0], q[1, 0] = 1.0, -0.5
    keys = np.arange(10, 18, dtype=np.uint32)
    ops = [op for R in (1, 2, 3, 4, 5, 6, 8, 9) for op in three_ops("ip", q, keys, R)]
    return case(dim, dtype, vec, ops, lo=10, labels=keys if keyed else None, vmin=np.full(dim, -128, F32), step=np.ones(dim, F32))   # (bytes x + 128: exact)


def zero_case(dim=70):
    """what could give -0 if anything could: every product -0 (+0 * -1, -0 * +0), a row of -0, and +x + -x within a lane and across
    lanes; a score is never -0, so these tie at +0 (image 0x7FFFFFFF) and come out by key"""
    vec = np.zeros((6, dim), F32)
    vec[1, :] = -1.0                                                           # q = +0 everywhere: every product -0
    vec[2, 0] = -0.0
    vec[3, :2] = (1.0, -1.0)                                                   # q = (1, 1, 0 ..): 1 + -1 = +0 (one lane each: the tree adds them)
    vec[4, 0], vec[4, 64] = 1.0, -1.0                                          # the same within lane 0
    vec[5, :] = -0.0
    q = np.zeros((3, dim), F32)
    q[1, :] = -0.0                                                             # (-0) * (-1) = +0, (-0) * (+0) = -0
    q[2, :2], q[2, 64] = 1.0, 1.0
    keys = np.arange(6, dtype=np.uint32)
    return case(dim, "f32", vec, three_ops("ip", q, keys, 6) + three_ops("ip", q, keys, 3))


def nonfinite_case(rng, dim, dtype):
    """+-inf scores, inf - inf = NaN, inf * 0 = NaN, NaN rows and NaN queries: NaN behind -inf, as 0x7FC00000"""
    rows = 30
    vec = rng.normal(size=(rows, dim)).astype(F32)
    vec[3, 0] = np.nan
    vec[4, dim - 1] = np.inf
    vec[5, dim // 2] = -np.inf
    vec[6, 0] = np.inf
    vec[7, 0] = -np.nan
    vec[8, :] = 0.0
    if dim >= 2:
        vec[9, 0], vec[9, dim - 1] = np.inf, -np.inf                           # inf - inf for a query of one sign
    q = rng.normal(size=(5, dim)).astype(F32)
    q[0] = np.abs(q[0]) + F32(0.5)
    q[1, 0] = np.nan                                                           # every score NaN
    q[2, dim - 1] = np.inf
    q[3, dim // 2] = -np.inf
    q[4, 0] = 0.0                                                              # 0 * inf = NaN on rows 6 (and 9)
    keys = np.arange(rows, dtype=np.uint32)
    vmin, step = sq_params(vec)
    return case(dim, dtype, vec, three_ops("ip", q, keys, rows + 2) + three_ops("ip", q, keys, 7), vmin=vmin, step=step)


def overflow_case():
    """finite rows whose partial sums overflow: +inf and -inf scores, and inf - inf in the tree"""
    big = F32(3e38)
    vec = np.zeros((5, 128), F32)
    vec[0, :2] = big                                                           # lane 0 and lane 1: 3e38 + 3e38 = +inf in the tree
    vec[1, :2] = -big
    vec[2, 0], vec[2, 64] = big, big                                           # ... within lane 0
    vec[3, :4] = (big, big, -big, -big)                                        # lanes 0 + 2 and 1 + 3 cancel at stride 2: +0, finite
    vec[4, 0], vec[4, 64], vec[4, 1], vec[4, 65] = big, big, -big, -big        # lane 0 +inf, lane 1 -inf: NaN at stride 1
    q = np.ones((1, 128), F32)
    keys = np.arange(5, dtype=np.uint32)
    return case(128, "f32", vec, three_ops("ip", q, keys, 5))


def tie_case(rng, dim, dtype, keyed=False, lo=50, rows=40):
    """ten identical rows under the keys lo + 10 .. lo + 19, the largest score of query 0: R = 5 cuts the tie by key, 10 ends with
    it, 11 goes one past it"""
    vec = (rng.normal(size=(rows, dim)) * 0.1).astype(F32)
    vec[10:20] = np.sign(vec[10]) * F32(2.0) + (vec[10] == 0)
    q = rng.normal(size=(2, dim)).astype(F32)
    q[0] = vec[10]
    keys = np.arange(lo, lo + rows, dtype=np.uint32)
    ops = [op for R in (15, 5, 10, 11) for op in three_ops("ip", q, keys, R)]
    return case(dim, dtype, vec, ops, lo=lo, labels=keys if keyed else None)


def norm_case(rng, dim=8, rows=200, nq=6):
    """Rows: signed permutations of one multiset of small integers, so all of one squared norm; queries: small integers.  Every
    product, sum and square is then an exact integer below 2^24, D = |q|^2 + |x|^2 - 2 S exactly, and the order by larger S, ties
    by key, is the order by smaller D, ties by key: the key lists under the two metrics are equal.  Rows repeat, so ties happen."""
    base = np.array([0, 1, 1, 2, 3, 5, 8, 13][:dim] + [0] * max(0, dim - 8))
    vec = np.stack([rng.permutation(base) * rng.choice([-1, 1], dim) for _ in range(rows)]).astype(F32)
    vec[50:60] = vec[7]
    q = rng.integers(-9, 10, (nq, dim)).astype(F32)
    keys = np.arange(rows, dtype=np.uint32)
    ops = []
    for metric in ("ip", "l2"):
        for R in (1, 17, rows):
            ops += three_ops(metric, q, keys, R)
    return case(dim, "f32", vec, ops)


def image_sweep():
    """bit patterns: both zeros, both infinities, the edges of the subnormals and of the finite range, NaNs of either sign, quiet and
    signalling, and a stride through everything"""
    edge = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F800000, 0xBF800000,
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF,
            0x7FBFFFFF, 0xFFBFFFFF]
    return np.concatenate([np.array(edge, np.uint32), np.arange(0, 2 ** 32, 65521, dtype=np.uint64).astype(np.uint32)])
