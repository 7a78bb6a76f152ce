"""What the float-ADC feeders (qadc_adc_search*, qadc_adc_encode_host, the host twin pq_bytes) must compute, composed from the
oracle's functions: assign, residual, OPQ rotation, the two table forms and the codes for 256 centroids per sub-quantizer.
Every float is compared bit for bit: device, host twin and oracle evaluate the same sums in the same order."""
import numpy as np


def rotate(x, rotation):
    """opq::rotate_multiple_vectors restated: rotated[r] = sum_c x[c] * rotation[r][c], one float32 sum in ascending c
    (numpy rounds every multiply and every add: no fused multiply-add)."""
    x = np.ascontiguousarray(x, np.float32)
    rot = np.ascontiguousarray(rotation, np.float32)
    acc = np.zeros(x.shape, np.float32)
    with np.errstate(all="ignore"):
        for c in range(x.shape[-1]):
            acc = acc + x[..., c:c + 1] * rot[:, c]
    return acc


def assign(po, queries, coarse, ma, sum_mode=1):
    """find_k_neighbors(k = ma) -> int32 [nq][ma], nearest first; a flat database (coarse None) probes partition 0"""
    q = np.ascontiguousarray(queries, np.float32)
    if coarse is None:
        return np.zeros((q.shape[0], ma), np.int32)
    return po.select_k_neighbors(po.cross_dists(coarse, q, sum_mode), ma)[0]


def residuals(queries, coarse, a, rotation=None):
    """-> float32 [nq][ma][dim]: q - coarse[assign] (the query itself for a flat database), rotated for OPQ"""
    q = np.ascontiguousarray(queries, np.float32)
    with np.errstate(all="ignore"):
        res = np.repeat(q[:, None, :], a.shape[1], axis=1) if coarse is None else q[:, None, :] - np.asarray(coarse, np.float32)[a]
    res = np.ascontiguousarray(res, np.float32)
    return res if rotation is None else rotate(res, rotation)


def tables_expansion(po, codebooks, x, sum_mode=1):
    """x [n][dim] -> [n][nsq*256]: per sub-quantizer the oracle's compute_cross_dists_blas restatement"""
    nsq, _, ds = codebooks.shape
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], nsq, 256), np.float32)
    for m in range(nsq):
        out[:, m, :] = po.cross_dists(codebooks[m], x[:, m * ds:(m + 1) * ds], sum_mode)
    return out.reshape(x.shape[0], nsq * 256)


def tables_direct(po, codebooks, x, sum_mode=1):
    """x [n][dim] -> [n][nsq*256]: the oracle's compute_dists_single_simd_cg restatement, which is written for 16 centroids: the
    codebooks [nsq][256][ds] go in as [nsq*16][16][ds] and every sub-vector is repeated 16 times"""
    nsq, _, ds = codebooks.shape
    cb = np.ascontiguousarray(codebooks, np.float32).reshape(nsq * 16, 16, ds)
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], nsq * 256), np.float32)
    for i in range(x.shape[0]):
        out[i] = po.tables_direct(cb, np.repeat(x[i].reshape(nsq, ds), 16, axis=0).reshape(-1), sum_mode)
    return out


def expansion_used(table_form, ma):
    """table_form 2 = nns_engine's rule: the direct form for ma == 1 only"""
    return bool(table_form) if table_form != 2 else ma > 1


def tables(po, codebooks, res, table_form, sum_mode=1):
    """res [nq][ma][dim] -> [nq][ma][nsq*256]"""
    nq, ma, dim = res.shape
    f = tables_expansion if expansion_used(table_form, ma) else tables_direct
    return f(po, codebooks, res.reshape(nq * ma, dim), sum_mode).reshape(nq, ma, -1)


def pin_to_reference(po, codebooks, x, sum_mode=1):
    """Where the reference's own build is there: its norm half (compute_cross_dists_blas up to the sgemm call) and its direct
    form agree with the restatements used above, for the sub-vector sizes its dispatch has.  x [n][dim], a few rows."""
    if sum_mode != 1 or not po.have_ref_float():
        return
    nsq, _, ds = codebooks.shape
    x = np.ascontiguousarray(x, np.float32)
    for m in range(nsq):
        sub = x[:, m * ds:(m + 1) * ds]
        want = po.reff_cross_norms(codebooks[m], sub)
        if want is not None:
            got = po.cross_dists(codebooks[m], sub, 1, with_product=False)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "norm half, sq_dim %d" % ds
    if ds in (8, 16, 32):
        cb = np.ascontiguousarray(codebooks, np.float32).reshape(nsq * 16, 16, ds)
        for i in range(x.shape[0]):
            v = np.repeat(x[i].reshape(nsq, ds), 16, axis=0).reshape(-1)
            assert np.array_equal(po.tables_direct(cb, v, 1).view(np.uint32), po.reff_tables_direct(cb, v).view(np.uint32)), \
                "direct form, sq_dim %d" % ds


def codes(po, codebooks, x, sum_mode=1):
    """encode_multiple_vectors for 8-bit sub-quantizers on vectors already made residuals and rotated -> uint8 [n][nsq]"""
    nsq, _, ds = codebooks.shape
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], nsq), np.uint8)
    for m in range(nsq):
        d = po.cross_dists(codebooks[m], x[:, m * ds:(m + 1) * ds], sum_mode)
        out[:, m] = po.select_k_neighbors(d, 1)[0][:, 0].astype(np.uint8)
    return out


def encode(po, codebooks, vectors, coarse=None, rotation=None, sum_mode=1):
    """index_db::add_vectors' compute -> (assign [n] or None, codes [n][nsq])"""
    v = np.ascontiguousarray(vectors, np.float32)
    a = None
    x = v
    if coarse is not None:
        a = assign(po, v, coarse, 1, sum_mode)
        with np.errstate(all="ignore"):
            x = np.ascontiguousarray(v - np.asarray(coarse, np.float32)[a[:, 0]], np.float32)
    if rotation is not None:
        x = rotate(x, rotation)
    return (None if a is None else a[:, 0].copy()), codes(po, codebooks, x, sum_mode)


def random_rotation(rng, dim):
    """an orthonormal [dim][dim] float32 matrix"""
    q, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
    return np.ascontiguousarray(q, np.float32)


def assert_same_floats(got, want, what=""):
    """bit for bit, except that a NaN matches any NaN"""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN entries differ" % what
    ok = (got.view(np.uint32) == want.view(np.uint32)) | gn
    assert ok.all(), "%s: %d of %d entries differ, first at %s" % (what, int((~ok).sum()), ok.size, np.argwhere(~ok)[0])
