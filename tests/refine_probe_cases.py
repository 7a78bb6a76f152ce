"""Shared by the tests of the probed exact search over a refine store (qadc_refine_knn_probed).  A CASE is a
dict keyed (bool), dim, dtype ("f32" | "f16" | "sq8"), vmin, step (sq8), ops — the life of the store, refine_knn_cases' add / put /
remove —, parts — the partitions of the index as [(labels uint32 [n] | None, key_base, rows)] —, index_filter — None or (mode, keys),
the filter set on the index — and calls, a list of

    (queries [nq][dim], assign int32 [nq][ma], R, filter)     filter: None or (mode "exclude" | "allow", keys uint32 [n])

and three things run cases and return one result per call, to be compared for equality:
  run_twin   refine::knn_probed of quick-adc_amd/host/refine.hpp through tests/cpp/refine_probe_host.cpp; beside it, where every
             query has at most 8192 entries, "rr": the twin's rerank fed the entries the driver lists itself
  run_numpy  an independent restatement: the entries gathered in numpy, refine_cases.np_distance over their rows
  run_gpu    pyqadc.Refine.knn_probed on an AdcIndex built from the partitions, through the host form or through torch tensors
A result is a dict keys [nq][R], dist [nq][R], sizes [nq], missing."""
import os
import subprocess

import numpy as np

import refine_cases as rc
import refine_knn_cases as kc
import refine_sq_cases as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_probe_host")
PLAN_EXE = os.path.join(ROOT, "tests", "cpp", "refine_probe_plan_host")
NO_KEY = rc.NO_KEY
MODES = kc.MODES
DTYPES = sq.DTYPES
SIZES = (0, 1, 63, 300, 700)     # the partitions of most GPU tests
add, put, remove = kc.add, kc.put, kc.remove


def build_driver():
    from test_scanner_hip_cpp import _compile
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def build_plan_driver():
    from test_scanner_hip_cpp import _compile
    _compile(PLAN_EXE + ".cpp", PLAN_EXE, link=False)
    return PLAN_EXE


def _filter(f):
    return None if f is None else (f[0], np.ascontiguousarray(np.asarray(f[1], np.uint64).astype(np.uint32)).reshape(-1))


def call(queries, assign, R, filter=None):
    queries = np.ascontiguousarray(queries, np.float32)
    queries = queries.reshape(1, -1) if queries.ndim == 1 else queries
    assign = np.ascontiguousarray(assign, np.int32).reshape(queries.shape[0], -1)
    return (queries, assign, int(R), _filter(filter))


def part(labels=None, key_base=0, rows=None):
    if labels is not None:
        labels = np.ascontiguousarray(np.asarray(labels, np.uint64).astype(np.uint32)).reshape(-1)
        return (labels, 0, len(labels))
    return (None, int(key_base), int(rows))


def case(keyed, dim, dtype, ops, parts, calls, index_filter=None, vmin=None, step=None):
    c = dict(keyed=bool(keyed), dim=int(dim), dtype=dtype, ops=list(ops), parts=list(parts), calls=list(calls), index_filter=_filter(index_filter),
             vmin=None, step=None)
    if dtype == "sq8":
        c["vmin"] = np.ascontiguousarray(vmin, np.float32).reshape(dim)
        c["step"] = np.ascontiguousarray(step, np.float32).reshape(dim)
    return c


def part_keys(p):
    labels, base, rows = p
    return labels if labels is not None else (np.arange(rows, dtype=np.uint64) + np.uint64(base)).astype(np.uint32)


def split_labels(labels, sizes=SIZES):
    """labels cut into labelled partitions of the given sizes"""
    assert len(labels) == sum(sizes)
    cuts = np.cumsum((0,) + tuple(sizes))
    return [part(labels[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def _write_filter(f, flt):
    np.array([-1 if flt is None else MODES[flt[0]]], np.int32).tofile(f)
    np.array([0 if flt is None else len(flt[1])], np.uint64).tofile(f)
    if flt is not None:
        flt[1].tofile(f)


def run_twin(exe, tmp_path, cases):
    fin, fout = str(tmp_path / "probe.in"), str(tmp_path / "probe.out")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for c in cases:
            np.array([c["keyed"], c["dim"], DTYPES[c["dtype"]], len(c["ops"]), len(c["parts"]), len(c["calls"])], np.int32).tofile(f)
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
                else:
                    np.array([2], np.int32).tofile(f)
                    np.array([len(op[1])], np.uint64).tofile(f)
                    op[1].tofile(f)
            for labels, base, rows in c["parts"]:
                np.array([labels is not None], np.int32).tofile(f)
                np.array([base], np.uint32).tofile(f)
                np.array([rows], np.uint64).tofile(f)
                if labels is not None:
                    labels.tofile(f)
            _write_filter(f, c["index_filter"])
            for q, a, R, flt in c["calls"]:
                np.array([q.shape[0], a.shape[1], R, -1 if flt is None else MODES[flt[0]]], np.int32).tofile(f)
                np.array([0 if flt is None else len(flt[1])], np.uint64).tofile(f)
                q.tofile(f)
                a.tofile(f)
                if flt is not None:
                    flt[1].tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        def result(nq, R):
            return dict(keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R), dist=np.fromfile(f, np.float32, nq * R).reshape(nq, R),
                        sizes=np.fromfile(f, np.int32, nq), missing=int(np.fromfile(f, np.uint64, 1)[0]))
        for c in cases:
            res = []
            for q, a, R, flt in c["calls"]:
                r = result(q.shape[0], R)
                r["rr"] = result(q.shape[0], R) if int(np.fromfile(f, np.int32, 1)[0]) else None
                res.append(r)
            got.append(res)
        assert f.read() == b""
    return got


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------

def held_rows(c):
    """{key: row float32 [dim] as the distance reads it} after the store's operations"""
    held = {}
    for op in c["ops"]:
        if op[0] in ("add", "put"):
            rows = op[2]
            if c["dtype"] == "f16":
                with np.errstate(over="ignore"):
                    rows = rows.astype(np.float16).astype(np.float32)
            elif c["dtype"] == "sq8":
                rows = sq.np_decode(sq.np_encode(rows, c["vmin"], c["step"])[0], c["vmin"], c["step"])
            labels = op[1] if op[0] == "put" else np.arange(op[1], op[1] + len(rows))
            for lab, row in zip(np.asarray(labels).tolist(), rows):
                held[lab] = row
        else:
            for lab in op[1].tolist():
                held.pop(lab, None)
    return held


def _passes(keys, flt):
    return np.ones(len(keys), bool) if flt is None else (np.isin(keys, flt[1]) == (flt[0] == "allow"))


def run_numpy(c):
    held = held_rows(c)
    held_keys = np.array(sorted(held), np.uint32)
    got = []
    for queries, assign, R, flt in c["calls"]:
        nq = queries.shape[0]
        out = dict(keys=np.full((nq, R), NO_KEY, np.uint32), dist=np.full((nq, R), np.inf, np.float32), sizes=np.zeros(nq, np.int32), missing=0)
        for q in range(nq):
            probed = sorted(set(int(p) for p in assign[q] if 0 <= p < len(c["parts"])))
            keys = np.concatenate([part_keys(c["parts"][p]) for p in probed] + [np.zeros(0, np.uint32)]).astype(np.uint32)
            keys = keys[_passes(keys, c["index_filter"]) & _passes(keys, flt)]
            is_held = np.isin(keys, held_keys)
            out["missing"] += int((~is_held).sum())
            keys = np.unique(keys[is_held])
            if len(keys) == 0:
                continue
            d = rc.np_distance(queries[q], np.stack([held[int(k)] for k in keys]))
            img = d.view(np.uint32).astype(np.uint64)
            img[np.isnan(d)] = rc.NAN_IMAGE
            words = np.sort((img << np.uint64(32)) | keys.astype(np.uint64))[:R]
            n = len(words)
            out["keys"][q, :n] = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            out["dist"][q, :n] = (words >> np.uint64(32)).astype(np.uint32).view(np.float32)
            out["sizes"][q] = n
        got.append(out)
    return got


same = rc.same


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        diff = same(g, w)
        assert diff is None, "%s call %d: %s differs" % (what, i, diff)


# ---- the GPU ------------------------------------------------------------------------------------------------------------------

def make_store(pyqadc, c):
    st = pyqadc.Refine(c["dim"], c["dtype"], keyed=c["keyed"], vmin=c["vmin"], step=c["step"])
    for op in c["ops"]:
        if op[0] == "add":
            st.add(op[2], op[1])
        elif op[0] == "put":
            st.put(op[2], op[1])
        else:
            st.remove(op[1])
    return st


def make_index(pyqadc, parts, sq_count=8, seed=0):
    """an owned 8-bit AdcIndex whose partitions hold random codes and the parts' labels (all labelled, or none with key_base 0)"""
    rng = np.random.default_rng(seed)
    labelled = [p[0] is not None for p in parts]
    assert all(labelled) or not any(labelled)
    assert all(labelled) or all(p[1] == 0 for p in parts)
    idx = pyqadc.AdcIndex(sq_count, 8)
    codes = [rng.integers(0, 256, (p[2], sq_count), dtype=np.uint8) for p in parts]
    idx.add_partitions(codes, [p[0] for p in parts] if all(labelled) and parts else None)
    return idx


def parts_of(index):
    """the partitions of an AdcIndex as a case takes them, read back from the index (unlabelled: key_base 0, an owned index's rule)"""
    out = []
    for p in range(index.partition_count()):
        _, labels = index.read_partition(p)
        out.append(part(labels) if labels is not None else part(None, 0, index.partition_size(p)))
    return out


def run_calls(pyqadc, st, idx, calls, device=False):
    if device:
        import torch

        def dev(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:%d" % st.device)
    got = []
    for q, a, R, flt in calls:
        f = None if flt is None else pyqadc.AdcFilter(flt[1], flt[0], device=st.device)
        if device:
            k, d, s, m = st.knn_probed_device(idx, dev(q), dev(a), R, filter=f)
            k, d, s = k.cpu().numpy().view(np.uint32), d.cpu().numpy(), s.cpu().numpy()
        else:
            k, d, s, m = st.knn_probed(idx, q, a, R, filter=f)
        if f is not None:
            f.close()
        got.append(dict(keys=k, dist=d, sizes=s, missing=m))
    return got


def run_gpu(pyqadc, c, device=False, plan=None):
    """the case on a new pyqadc.Refine and a new owned AdcIndex; plan: (chunk_rows, pass_nq) for set_knn_plan"""
    st = make_store(pyqadc, c)
    idx = make_index(pyqadc, c["parts"])
    flt = None
    try:
        if plan is not None:
            st.set_knn_plan(*plan)
        if c["index_filter"] is not None:
            flt = pyqadc.AdcFilter(c["index_filter"][1], c["index_filter"][0], device=st.device)
            idx.set_filter(flt)
        return run_calls(pyqadc, st, idx, c["calls"], device)
    finally:
        idx.set_filter(None)
        idx.close()
        st.close()
        if flt is not None:
            flt.close()


# ---- case builders ------------------------------------------------------------------------------------------------------------

def sq_params(vec):
    lo, hi = vec.min(axis=0).astype(np.float32), vec.max(axis=0).astype(np.float32)
    return lo, ((hi - lo) / np.float32(255.0)).astype(np.float32)


def dense_case(rng, dim, dtype, calls_of, sizes=SIZES, lo=0, shuffle=True, keyed=False):
    """a store of sum(sizes) random rows under the keys lo .. and labelled partitions that hold each key once (shuffled);
    calls_of(vec, labels) -> the calls"""
    n = sum(sizes)
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    labels = np.arange(lo, lo + n, dtype=np.uint32)
    if shuffle:
        labels = rng.permutation(labels)
    kw = {}
    if dtype == "sq8":
        kw["vmin"], kw["step"] = sq_params(vec)
    ops = [put(np.arange(lo, lo + n, dtype=np.uint32), vec)] if keyed else [add(lo, vec)]
    return case(keyed, dim, dtype, ops, split_labels(labels, sizes), calls_of(vec, labels), **kw)


def probes(rng, nq, ma, K):
    """assign [nq][ma]: ma distinct partitions per query"""
    return np.stack([rng.permutation(K)[:ma] for _ in range(nq)]).astype(np.int32)
