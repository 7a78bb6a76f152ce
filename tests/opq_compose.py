"""What OPQ learning (qadc_opq_cross_host, qadc_procrustes_host, qadc_opq_train_host) must compute, and the
plumbing its tests share: the CPU twins through their driver (tests/cpp/opq_host.cpp), the learning set of the issue's sketch, the
loop composed from the public calls, and float64 helpers."""
import os
import subprocess

import numpy as np

import adc_compose as ac
import pq_train_compose as ptc
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "opq_host")
BLOCK = 2048                                                     # include/qadc.h QADC_OPQ_BLOCK


def build_driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "opq_host.cpp"), EXE, link=False)
    return EXE


def _run(exe, mode, tmp_path, header, arrays):
    fin, fout = str(tmp_path / ("opq_%s.in" % mode)), str(tmp_path / ("opq_%s.out" % mode))
    with open(fin, "wb") as f:
        np.array(header, np.int32).tofile(f)
        for a in arrays:
            a.tofile(f)
    out = subprocess.run([exe, mode, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    return fout


def _shape(codebooks):
    nsq, K, ds = codebooks.shape
    return nsq, {16: 4, 256: 8}[K], nsq * ds


def twin_cross(exe, tmp_path, v, codes, codebooks, coarse=None):
    """host/db_build.hpp opq_cross -> float64 [dim][dim]"""
    nsq, bits, dim = _shape(codebooks)
    v = np.ascontiguousarray(v, np.float32)
    co = np.zeros((0, dim), np.float32) if coarse is None else np.ascontiguousarray(coarse, np.float32)
    fout = _run(exe, "cross", tmp_path, [v.shape[0], dim, nsq, bits, len(co)],
                [v, np.ascontiguousarray(codebooks, np.float32), co, np.ascontiguousarray(codes, np.uint8)])
    return np.fromfile(fout, np.float64).reshape(dim, dim)


def chain(exe, tmp_path, x, y, descending=False):
    """the plain restatement: per block of 2048 rows one std::fmaf chain per (a, b), the blocks added in float64"""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    fout = _run(exe, "chain", tmp_path, [x.shape[0], x.shape[1], int(descending)], [x, y])
    return np.fromfile(fout, np.float64).reshape(x.shape[1], x.shape[1])


def twin_train(exe, tmp_path, v, seed, outer, inner, rotation, coarse=None, div_mode=1):
    """host/db_build.hpp opq_train_iterations -> (rotation, codebooks, codes, empty, rounds_done)"""
    nsq, bits, dim = _shape(seed)
    v = np.ascontiguousarray(v, np.float32)
    n = v.shape[0]
    co = np.zeros((0, dim), np.float32) if coarse is None else np.ascontiguousarray(coarse, np.float32)
    fout = _run(exe, "train", tmp_path, [n, dim, nsq, bits, len(co), outer, inner, div_mode],
                [v, np.ascontiguousarray(seed, np.float32), co, np.ascontiguousarray(rotation, np.float32)])
    with open(fout, "rb") as f:
        rot = np.fromfile(f, np.float32, dim * dim).reshape(dim, dim)
        cb = np.fromfile(f, np.float32, seed.size).reshape(seed.shape)
        codes = np.fromfile(f, np.uint8, n * (nsq // 2 if bits == 4 else nsq)).reshape(n, -1)
        empty = int(np.fromfile(f, np.uint64, 1)[0])
        done = int(np.fromfile(f, np.int32, 1)[0])
        assert f.read() == b""
    return rot, cb, codes, empty, done


def reconstruction(codebooks, codes):
    """Y [n][dim] float32: the centroids the codes select, side by side"""
    nsq, bits, _ = _shape(codebooks)
    a = ptc.unpack(codes, bits)
    return np.ascontiguousarray(np.concatenate([codebooks[m][a[:, m]] for m in range(nsq)], axis=1), np.float32)


def x0_of(po, v, coarse):
    """the learning set as the quantizer sees it before rotation"""
    v = np.ascontiguousarray(v, np.float32)
    return v if coarse is None else ac.residuals(v, coarse, ac.assign(po, v, coarse, 1))[:, 0, :]


def same_doubles(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN entries differ" % what
    ok = (got.view(np.uint64) == want.view(np.uint64)) | gn
    assert ok.all(), "%s: %d of %d entries differ, first at %s" % (what, int((~ok).sum()), ok.size, np.argwhere(~ok)[0])


def orthogonality(rotation):
    """max |R R^T - I| in float64"""
    r = np.asarray(rotation, np.float64)
    return float(np.abs(r @ r.T - np.eye(r.shape[0])).max())


def sketch_set():
    """the issue's learning set: n = 3000, dim 32, a decaying spectrum hidden behind a random orthogonal matrix; a 16 x 4 quantizer
    seeded from 16 distinct rows -> (vectors, seed)"""
    rng = np.random.default_rng(20)
    n, dim = 3000, 32
    z = rng.normal(size=(n, dim)) * 0.85 ** np.arange(dim)
    q, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
    v = np.ascontiguousarray(z @ q, np.float32)
    return v, ptc.seed_rows(v, 16, 4, rng.choice(n, 16, replace=False))


def rotated(v, rotation):
    """rotated[r] = sum_c x[c] R[r][c], in float64 (for error figures only)"""
    return np.asarray(v, np.float64) @ np.asarray(rotation, np.float64).T


def composed(pyqadc, v, seed, outer, inner, rotation, coarse=None, div_mode=1):
    """the loop of qadc_opq_train_host written with the public calls -> (rotation, codebooks, codes, empty, rounds_done)"""
    rot, cb, done = np.array(rotation, np.float32, copy=True), np.array(seed, np.float32, copy=True), 0
    for _ in range(outer):
        cb, codes, _ = pyqadc.train_pq(v, cb, inner, coarse=coarse, rotation=rot, div_mode=div_mode)
        M = pyqadc.opq_cross(v, codes, cb, coarse=coarse)
        if not np.isfinite(M).all():
            break
        rot = pyqadc.procrustes(M)[0]
        done += 1
    cb, codes, empty = pyqadc.train_pq(v, cb, inner, coarse=coarse, rotation=rot, div_mode=div_mode)
    return rot, cb, codes, empty, done
