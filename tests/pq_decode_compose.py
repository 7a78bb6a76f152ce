"""What the PQ decoder (qadc_pq_decode_host / _device, qadc_adc_index_reconstruct*; include/qadc.h "Reconstruction", DESIGN.md
section 11.19) must compute: the definition in numpy, the CPU twin through its driver (tests/cpp/pq_decode_host.cpp), and the
fixtures the CPU and GPU tests share.

The definition: gather (a copy), un-rotate (ONE chain acc = fmaf(y[r], rotation[r][c], acc) over ascending r), add the coarse
centroid (one float add), error (ONE chain acc = fmaf(d, d, acc), d = v[c] - x[c]).  fma() restates the fused step exactly: a * b is
exact in float64 (48 bits), the float64 sum acc + a * b is corrected to round-to-odd with the error term of a two-sum, and a
round-to-odd value of 53 bits rounds to float32 as the infinitely precise sum does (53 >= 2 * 24 + 2) — pq_repair_compose's
argument, for a product of two different factors."""
import os
import subprocess

import numpy as np

import pq_train_compose as ptc
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "pq_decode_host")
PLAN_EXE = os.path.join(ROOT, "tests", "cpp", "pq_decode_plan_host")
PAIRS = [(16, 4), (32, 4), (4, 8), (8, 8), (16, 8), (2, 16), (4, 16), (8, 16)]     # the encoders' (sq_count, sq_bits)
NAN_BITS = 0x7FC00000
MISSING = np.uint64(0xFFFFFFFFFFFFFFFF)
CHUNK = 262144                                                                     # QADC_DECODE_CHUNK


def pair_id(p):
    return "%dx%d" % p


def build_driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "pq_decode_host.cpp"), EXE, link=False)
    return EXE


def build_plan_driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "pq_decode_plan_host.cpp"), PLAN_EXE, link=False)
    return PLAN_EXE


def fma(a, b, acc):
    """float32 fmaf(a, b, acc) elementwise (broadcasting)"""
    with np.errstate(all="ignore"):
        p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)     # exact
        c = np.broadcast_to(np.asarray(acc, np.float32).astype(np.float64), p.shape)
        s = c + p
        bb = s - c
        err = (c - (s - bb)) + (p - bb)                                     # two-sum: c + p = s + err exactly
        odd = (s.view(np.uint64) & np.uint64(1)) == 1
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def bits_of(cb):
    return {16: 4, 256: 8, 65536: 16}[cb.shape[1]]


def code_cols(nsq, bits):
    return nsq // 2 if bits == 4 else nsq


def unpack(codes, bits):
    """codes in the encoder's layout -> int64 [n][nsq]"""
    return np.asarray(codes).astype(np.int64) if bits == 16 else ptc.unpack(codes, bits).astype(np.int64)


def pack(assign, bits):
    return np.ascontiguousarray(assign, np.uint16) if bits == 16 else ptc.pack(assign, bits)


def missing_rows(assign, n, K):
    if assign is None:
        return np.zeros(n, bool)
    a = np.asarray(assign, np.int64)
    return (a < 0) | ((a >= K) if K > 0 else False)


def restate(cb, codes, assign=None, coarse=None, rotation=None, vectors=None):
    """the definition -> out float32 [n][dim] (and err float32 [n] with vectors)"""
    cb = np.ascontiguousarray(cb, np.float32)
    nsq, _, ds = cb.shape
    bits, dim = bits_of(cb), nsq * ds
    a = unpack(codes, bits)
    n = a.shape[0]
    K = 0 if coarse is None else len(coarse)
    y = np.concatenate([cb[m][a[:, m]] for m in range(nsq)], axis=1).reshape(n, dim) if n else np.zeros((0, dim), np.float32)
    z = y
    if rotation is not None:
        rot = np.ascontiguousarray(rotation, np.float32)
        z = np.zeros((n, dim), np.float32)
        for r in range(dim):
            z = fma(y[:, r:r + 1], rot[r][None, :], z)
    miss = missing_rows(assign if (K > 0 or assign is not None) else None, n, K)
    x = z
    if K > 0:
        safe = np.where(miss, 0, np.asarray(assign, np.int64))
        with np.errstate(all="ignore"):
            x = (z + np.asarray(coarse, np.float32)[safe]).astype(np.float32)
    x = np.ascontiguousarray(x, np.float32).copy()
    if rotation is not None or K > 0:
        x.view(np.uint32)[np.isnan(x)] = NAN_BITS                           # a NaN arithmetic made or passed on: the canonical one
    x.view(np.uint32)[miss] = NAN_BITS
    if vectors is None:
        return x
    v = np.ascontiguousarray(vectors, np.float32)
    err = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for c in range(dim):
            d = (v[:, c] - x[:, c]).astype(np.float32)
            err = fma(d, d, err)
    err.view(np.uint32)[np.isnan(err)] = NAN_BITS
    return x, err


def twin(exe, tmp_path, cb, codes, assign=None, coarse=None, rotation=None, vectors=None):
    """host/pq_decode.hpp pq_decode -> out (and err with vectors)"""
    cb = np.ascontiguousarray(cb, np.float32)
    nsq, _, ds = cb.shape
    bits, dim = bits_of(cb), nsq * ds
    c = np.ascontiguousarray(codes, "<u2" if bits == 16 else np.uint8)
    n = c.shape[0]
    K = 0 if coarse is None else len(coarse)
    fin, fout = str(tmp_path / "decode.in"), str(tmp_path / "decode.out")
    with open(fin, "wb") as f:
        np.array([n, dim, nsq, bits, K, rotation is not None, assign is not None, vectors is not None], np.int64).tofile(f)
        cb.tofile(f)
        for arr, dt in ((rotation, np.float32), (coarse, np.float32), (assign, np.int32)):
            if arr is not None:
                np.ascontiguousarray(arr, dt).tofile(f)
        c.tofile(f)
        if vectors is not None:
            np.ascontiguousarray(vectors, np.float32).tofile(f)
    out = subprocess.run([exe, "decode", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    with open(fout, "rb") as f:
        x = np.fromfile(f, np.float32, n * dim).reshape(n, dim)
        err = np.fromfile(f, np.float32, n) if vectors is not None else None
        assert f.read() == b""
    return x if vectors is None else (x, err)


def where_numpy(sizes, labels, key_base, keys):
    """the lookup's definition: the smallest (partition, row) whose key is keys[i] -> uint64 [count]"""
    first = {}
    for p, n in enumerate(sizes):
        ks = np.asarray(labels[p], np.uint32) if labels is not None else (np.uint32(key_base[p]) + np.arange(n, dtype=np.uint32))
        for r in range(int(n)):
            first.setdefault(int(ks[r]), (p << 32) | r)
    return np.array([first.get(int(k), int(MISSING)) for k in np.asarray(keys, np.uint32).reshape(-1)], np.uint64)


def twin_where(exe, tmp_path, sizes, labels, key_base, keys):
    """host/pq_decode.hpp reconstruct_where"""
    sizes = np.ascontiguousarray(sizes, np.uint32)
    keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
    fin, fout = str(tmp_path / "where.in"), str(tmp_path / "where.out")
    with open(fin, "wb") as f:
        np.array([len(sizes), labels is not None, keys.size], np.int64).tofile(f)
        sizes.tofile(f)
        np.ascontiguousarray(key_base if key_base is not None else np.zeros(len(sizes)), np.uint32).tofile(f)
        if labels is not None:
            for l in labels:
                np.ascontiguousarray(l, np.uint32).tofile(f)
        keys.tofile(f)
    out = subprocess.run([exe, "where", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    return np.fromfile(fout, np.uint64)


def same_floats(got, want, what=""):
    """bit for bit, NaN payloads included"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d floats differ, first at %s: %r against %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


# ---- inputs ----

def random_case(rng, nsq, bits, dim, n, K=0, rotated=False, scale=1.0):
    """-> dict(cb, codes, assign, coarse, rotation, vectors): floats of every sign and size, every code value possible"""
    ds = dim // nsq
    cb = (rng.normal(size=(nsq, 1 << bits, ds)) * scale).astype(np.float32)
    codes = pack(rng.integers(0, 1 << bits, (n, nsq)), bits)
    coarse = rng.normal(size=(K, dim)).astype(np.float32) if K else None
    assign = rng.integers(0, K, n).astype(np.int32) if K else None
    rotation = None
    if rotated:
        q, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
        rotation = np.ascontiguousarray(q, np.float32)
    vectors = rng.normal(size=(n, dim)).astype(np.float32)
    return dict(cb=cb, codes=codes, assign=assign, coarse=coarse, rotation=rotation, vectors=vectors)


def exact_fixture(nsq, bits, dim, K=0, rotated=False, seed=0):
    """The exactness fixture: everything a small integer, so that every product and sum of the decoder AND of the encoders is exact
    in float32 (an integer below 2^24), with no zero entry, pairwise distinct centroids per sub-quantizer, pairwise distinct coarse
    centroids and a signed permutation for rotation.

    Codebook entries are non-zero integers in [-A, A]; centroid k of a sub-quantizer carries the digits of k in base 2 A in its first
    components (so the rows are pairwise distinct), in an order shuffled per sub-quantizer.  Coarse entries are S j with j in
    {-2, -1, 1, 2} and S = 2 A + 64.  Then for x = coarse[p] + (signed permutation of a centroid row y):
      * the coarse assignment of x is p: against any other centroid p' the squared distance grows by the sum over the differing
        components of S t (S t + 2 y_c) with t a non-zero integer, and S > 2 A >= 2 |y_c| makes every term positive;
      * the residual x - coarse[p] is the permuted y exactly, the encoders' rotation (a signed permutation) returns y exactly, and the
        distance of y's sub-vectors to their own centroids is 0 while every other centroid differs in a component, so it is >= 1;
      * every intermediate of the expansion distances (||v||^2 + ||c||^2) - 2 v.c is an integer of magnitude at most
        4 dim (2 S + A)^2, asserted below to stay under 2^24, hence exact whatever the grouping of the sums."""
    rng = np.random.default_rng(1000 * bits + 10 * nsq + dim + seed)
    ds, cent = dim // nsq, 1 << bits
    A = next(a for a in (2, 8, 128) if (2 * a) ** ds >= cent)
    S = 2 * A + 64
    assert 4 * dim * (2 * S + A) ** 2 < 1 << 24, "the fixture would leave the exact range of float32"
    vals = np.concatenate([np.arange(-A, 0), np.arange(1, A + 1)]).astype(np.float32)
    base = len(vals)
    cb = vals[rng.integers(0, base, (nsq, cent, ds))]
    k = np.arange(cent)
    for m in range(nsq):
        order = rng.permutation(cent)
        for d in range(ds):
            if base ** d < cent:
                cb[m, order, d] = vals[(k // base ** d) % base]
        assert len(np.unique(cb[m], axis=0)) == cent
    coarse = None
    if K:
        js = np.array([-2, -1, 1, 2])
        rows = set()
        while len(rows) < K:
            rows.add(tuple(js[rng.integers(0, 4, dim)]))
        coarse = np.array(sorted(rows), np.float32)[rng.permutation(K)] * np.float32(S)
    rotation = None
    if rotated:
        rotation = np.zeros((dim, dim), np.float32)
        rotation[np.arange(dim), rng.permutation(dim)] = rng.choice([-1.0, 1.0], dim)
    return dict(cb=np.ascontiguousarray(cb, np.float32), coarse=coarse, rotation=rotation, A=A, S=S)


def exact_rows(fx, n, seed=0):
    """n rows of the fixture: (codes in the encoder's layout, assign or None)"""
    rng = np.random.default_rng(seed + 77)
    nsq, cent, _ = fx["cb"].shape
    bits = bits_of(fx["cb"])
    codes = pack(rng.integers(0, cent, (n, nsq)), bits)
    assign = None if fx["coarse"] is None else rng.integers(0, len(fx["coarse"]), n).astype(np.int32)
    return codes, assign


def encode_twin(po, fx, vectors):
    """the CPU statement of the encoders on the fixture's quantizers -> (assign or None, codes in the encoder's layout)"""
    import adc16_encode_compose as a16e
    import adc_compose as ac
    cb, coarse, rotation = fx["cb"], fx["coarse"], fx["rotation"]
    bits = bits_of(cb)
    if bits == 8:
        return ac.encode(po, cb, vectors, coarse, rotation)
    if bits == 16:
        return a16e.encode16(po, cb, vectors, coarse, rotation)
    v = np.ascontiguousarray(vectors, np.float32)
    a = None
    if coarse is not None:
        a = ac.assign(po, v, coarse, 1)[:, 0].copy()
        v = np.ascontiguousarray(v - coarse[a], np.float32)
    return a, po.pq_encode(cb, v, rotation=rotation)


def plan(exe, lines):
    """host/pq_decode_plan.hpp for "sq_count sq_bits dim n aligned" lines -> list of None (refused) or dict"""
    names = ("dim dsub centroids code_bytes vec lanes_per_row rows_per_wg cb_in_lds cb_bytes gather_lds row_blocks gather_grid reg tile "
             "col_tiles row_tiles rot_grid rot_lds err_grid cover").split()
    out = subprocess.run([exe], input="\n".join("%d %d %d %d %d" % l for l in lines).encode(), stdout=subprocess.PIPE, timeout=600)
    assert out.returncode == 0
    res = []
    for line in out.stdout.decode().splitlines():
        res.append(None if line == "refused" else dict(zip(names, (int(t) for t in line.split()))))
    assert len(res) == len(lines)
    return res
