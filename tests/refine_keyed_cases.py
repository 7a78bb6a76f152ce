"""Shared by the tests of the keyed refine store: a life of a store is a SCRIPT, a list of operations

    ("put", labels uint32 [n], vectors float32 [n][dim])
    ("remove", labels uint32 [n])
    ("rerank", queries [nq][dim], keys uint32 [nq][r_in], R, counts int32 [nq] or None, values float32 [nq][r_in] or None)

and three things run a script and return one result per operation, to be compared for equality:
  run_twin   the host twin refine::keyed_store (quick-adc_amd/host/refine.hpp) through tests/cpp/refine_keyed_host.cpp
  run_numpy  an independent restatement: a dict from key to row, refine_cases.np_distance and a sort of (distance image, key) words
  run_store  a pyqadc.Refine(keyed=True) on the GPU, through the host forms or through torch tensors
A result is a dict: put -> ok (0: refused), live; remove -> removed, live; rerank -> missing, keys, dist, sizes."""
import os
import subprocess

import numpy as np

import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_keyed_host")
NO_KEY = rc.NO_KEY


def build_driver():
    from test_scanner_hip_cpp import _compile
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def put(labels, vectors):
    vectors = np.ascontiguousarray(vectors, np.float32)
    return ("put", np.ascontiguousarray(labels, np.uint32).reshape(-1), vectors.reshape(len(vectors), -1))


def remove(labels):
    return ("remove", np.ascontiguousarray(labels, np.uint32).reshape(-1))


def rerank(queries, keys, R, counts=None, values=None):
    queries = np.ascontiguousarray(queries, np.float32)
    queries = queries.reshape(1, -1) if queries.ndim == 1 else queries
    keys = np.ascontiguousarray(keys, np.uint32).reshape(queries.shape[0], -1)
    return ("rerank", queries, keys, int(R), None if counts is None else np.ascontiguousarray(counts, np.int32),
            None if values is None else np.ascontiguousarray(values, np.float32).reshape(keys.shape))


def run_twin(exe, tmp_path, dim, dtype, script):
    fin, fout = str(tmp_path / "keyed.in"), str(tmp_path / "keyed.out")
    with open(fin, "wb") as f:
        np.array([dim, rc.DTYPES[dtype], len(script)], np.int32).tofile(f)
        for op in script:
            if op[0] == "put":
                np.array([0], np.int32).tofile(f)
                np.array([len(op[1])], np.uint64).tofile(f)
                op[1].tofile(f)
                op[2].tofile(f)
            elif op[0] == "remove":
                np.array([1], np.int32).tofile(f)
                np.array([len(op[1])], np.uint64).tofile(f)
                op[1].tofile(f)
            else:
                _, q, k, R, counts, values = op
                np.array([2, q.shape[0], k.shape[1], R, counts is not None, values is not None], np.int32).tofile(f)
                q.tofile(f)
                k.tofile(f)
                if counts is not None:
                    counts.tofile(f)
                if values is not None:
                    values.tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    got = []
    with open(fout, "rb") as f:
        for op in script:
            if op[0] == "put":
                got.append(dict(ok=int(np.fromfile(f, np.int32, 1)[0]), live=int(np.fromfile(f, np.uint64, 1)[0])))
            elif op[0] == "remove":
                got.append(dict(removed=int(np.fromfile(f, np.uint64, 1)[0]), live=int(np.fromfile(f, np.uint64, 1)[0])))
            else:
                nq, R = op[1].shape[0], op[3]
                missing = int(np.fromfile(f, np.uint64, 1)[0])
                got.append(dict(missing=missing, keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R),
                                dist=np.fromfile(f, np.float32, nq * R).reshape(nq, R), sizes=np.fromfile(f, np.int32, nq)))
        assert f.read() == b""
    return got


def run_numpy(dim, dtype, script):
    held, got = {}, []
    for op in script:
        if op[0] == "put":
            _, labels, vectors = op
            if (labels == NO_KEY).any():
                got.append(dict(ok=0, live=len(held)))
                continue
            rows = vectors
            if dtype == "f16":
                with np.errstate(over="ignore"):
                    rows = vectors.astype(np.float16).astype(np.float32)
            for lab, row in zip(labels.tolist(), rows):
                held[lab] = row
            got.append(dict(ok=1, live=len(held)))
        elif op[0] == "remove":
            gone = [lab for lab in set(op[1].tolist()) if lab in held]
            for lab in gone:
                del held[lab]
            got.append(dict(removed=len(gone), live=len(held)))
        else:
            _, queries, keys, R, counts, values = op
            nq, r_in = keys.shape
            out = dict(missing=0, keys=np.full((nq, R), NO_KEY, np.uint32), dist=np.full((nq, R), np.inf, np.float32), sizes=np.zeros(nq, np.int32))
            for q in range(nq):
                count = r_in if counts is None else int(counts[q])
                k = keys[q, :count]
                if values is not None:
                    k = k[values[q, :count] != rc.FLT_MAX]
                here = np.array([int(x) in held for x in k], bool)
                out["missing"] += int((~here).sum())
                k = np.unique(k[here])
                if len(k) == 0:
                    continue
                d = rc.np_distance(queries[q], np.stack([held[int(x)] for x in k]))
                img = d.view(np.uint32).astype(np.uint64)
                img[np.isnan(d)] = rc.NAN_IMAGE
                words = np.sort((img << np.uint64(32)) | k.astype(np.uint64))[:R]
                n = len(words)
                out["keys"][q, :n] = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                out["dist"][q, :n] = (words >> np.uint64(32)).astype(np.uint32).view(np.float32)
                out["sizes"][q] = n
            got.append(out)
    return got


def run_store(pyqadc, st, script, device=False):
    """the script on the pyqadc.Refine `st`; device: through put_device / remove_device / rerank_device and torch tensors"""
    got = []
    if device:
        import torch

        def dev(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:%d" % st.device)
    for op in script:
        if op[0] == "put":
            try:
                st.put_device(dev(op[2]), dev(op[1])) if device else st.put(op[2], op[1])
                ok = 1
            except pyqadc.QadcError as e:
                assert "qadc error -1:" in str(e), e                             # QADC_E_ARG: the filler key
                ok = 0
            got.append(dict(ok=ok, live=st.keyed_info()["live"]))
        elif op[0] == "remove":
            removed = st.remove_device(dev(op[1])) if device else st.remove(op[1])
            got.append(dict(removed=removed, live=st.keyed_info()["live"]))
        else:
            _, q, k, R, counts, values = op
            if device:
                ok, od, osz, missing = st.rerank_device(dev(q), dev(k), R, counts=None if counts is None else dev(counts),
                                                        values=None if values is None else dev(values))
                ok, od, osz = ok.cpu().numpy().view(np.uint32), od.cpu().numpy(), osz.cpu().numpy()
            else:
                ok, od, osz, missing = st.rerank(q, k, R, counts=counts, values=values)
            got.append(dict(missing=missing, keys=ok, dist=od, sizes=osz))
    return got


def differs(a, b):
    """None where two results of one operation agree bit for bit, else what differs"""
    if "keys" in a:
        return rc.same(a, b)
    for name in a:
        if a[name] != b[name]:
            return "%s %r != %r" % (name, a[name], b[name])
    return None


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        diff = differs(g, w)
        assert diff is None, "%s operation %d: %s" % (what, i, diff)


def all_keys_rerank(rng, dim, keys, extra=(), R=None, nq=2):
    """a rerank whose lists hold every key of `keys` and `extra` (absent ones) once, in a random order per query, in chunks of at
    most 8192 candidates -> a list of operations"""
    keys = np.unique(np.concatenate([np.asarray(keys, np.uint32), np.asarray(extra, np.uint32)]))
    ops = []
    for first in range(0, len(keys), 8192):
        chunk = keys[first:first + 8192]
        q = rng.normal(size=(nq, dim)).astype(np.float32)
        ops.append(rerank(q, np.stack([rng.permutation(chunk) for _ in range(nq)]), len(chunk) if R is None else R))
    return ops
