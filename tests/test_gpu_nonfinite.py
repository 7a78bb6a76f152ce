"""GPU: coarse selection, the encoder and the k-means iterations on NaN, +inf and FLT_MAX distances.

The reference is compiled with -ffast-math, and its kv_binheap's replace test compiles to !(v >= top): a NaN replaces the heap
top, and the next value replaces a NaN top (oracle/qadc_oracle.c orc_select_k_neighbors, pinned to the reference build by
tests/test_oracle_float_ref.py::test_coarse_selection_on_non_finite_distances_is_the_reference_binary).  Every expected value
here is that selection on the oracle's coarse distances (and, where oracle/_ref is built, the reference's own selection too) —
never numpy's argmin / argsort, which order NaN differently.  Every assign[] entry must also lie in [0, K).

NaN and infinite float tables through the pre-scan, qmin and QuantizerMAX (query_scan, qadc_search with a NaN query vector) are
tests/test_gpu_nonfinite_tables.py's.  Out of scope: qadc_search refusing a NaN coarse row with ma > 256."""
import numpy as np
import pytest

import pyoracle as po
from helpers import coarse_dists, path_independent

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
NAN_POS = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
NAN_NEG = np.array([0xffc00000], np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def reference_select(d, k):
    """find_k_neighbors' selection with k on the distances d [n][K]: the oracle's, and the reference's own where it is built."""
    a = po.select_k_neighbors(d, k)[0]
    if po.have_ref_float():
        assert np.array_equal(a, po.reff_select_k_neighbors(d, k)[0])
    return a


def nonfinite_problem(rng, nq, K, dim, tail_nan=True):
    """Queries [nq][dim] and coarse centroids [K][dim] whose distances hold NaN of both signs, +inf and FLT_MAX-sized values:
    NaN centroid rows at 0, in the middle, at K-1 and in the last partial 256-block; NaN query rows (a whole row of NaN
    distances), queries scaled by 1e20 (||q||^2 overflows: a whole row of +inf), finite rows in between.  tail_nan=False leaves
    the rows at K-1 and in the last block finite (with a NaN at K-1, k = 1 picks K-1 in every row)."""
    c = rng.normal(size=(K, dim)).astype(np.float32)
    spots = ((0, NAN_POS), (K // 2, NAN_NEG)) + (((K - 1, NAN_NEG), (K - 1 - (K % 256) // 2, NAN_POS)) if tail_nan else ())
    for at, v in spots:
        c[at] = v
    c[K // 3, 0] = NAN_NEG                                          # one NaN component
    c[K // 5] = np.float32(1.5e19)                                  # ||c||^2 = +inf: a column of +inf
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    q[1::9] = NAN_POS
    q[2::9, dim - 1] = NAN_NEG
    q[4::9] *= np.float32(1e20)
    q[6::9] = c[(np.arange(6, nq, 9) * 7) % K]                      # distance ~0 to one centroid, exact ties of +0.0 possible
    return q, c


SHAPES = [  # (dim, K, ma, nq): the rounds form (ma < 8), the radix form (8 <= ma <= 256), both on the tiled distances
            # (dim % 4 == 0, K <= 16384); the fused form (dim % 4 != 0, or K > 16384) with 1 and 4 queries per workgroup
    (32, 300, 1, 40), (32, 300, 2, 40), (32, 1000, 7, 300), (32, 300, 8, 40), (32, 1000, 16, 300),
    (30, 300, 1, 40), (30, 300, 2, 600), (30, 700, 7, 40), (30, 300, 8, 600), (30, 700, 16, 40),
    (8, 16500, 1, 40), (8, 16500, 8, 600),
]


@path_independent
@pytest.mark.parametrize("tail_nan", [True, False])
@pytest.mark.parametrize("dim,K,ma,nq", SHAPES)
def test_coarse_assign_on_nonfinite_distances_is_find_k_neighbors(pyqadc, dim, K, ma, nq, tail_nan):
    rng = np.random.default_rng(dim * 100000 + K * 10 + ma)
    q, c = nonfinite_problem(rng, nq, K, dim, tail_nan)
    got = pyqadc.coarse_assign(q, c, ma)
    assert ((got >= 0) & (got < K)).all(), "assign[] entry outside [0, K)"
    d = coarse_dists(q, c)
    assert np.isnan(d).any() and np.isinf(d).any()
    want = reference_select(d, ma)
    bad = np.nonzero((got != want).any(1))[0]
    assert not len(bad), (bad[:5], got[bad[:2]], want[bad[:2]])


@path_independent
def test_coarse_assign_all_inf_rows_and_wide_nan_refusal(pyqadc):
    """All-+inf rows take the reference's order ([0, 1, 2] for ma = 3); a NaN row with ma > 256 is refused, not answered
    differently; the same ma on finite rows still works."""
    rng = np.random.default_rng(3)
    K, dim = 600, 16
    c = rng.normal(size=(K, dim)).astype(np.float32)
    q = rng.normal(size=(5, dim)).astype(np.float32) * np.float32(1e20)
    for ma in (3, 12):
        assert pyqadc.coarse_assign(q, c, ma).tolist() == [list(range(ma))] * 5
    q2 = rng.normal(size=(3, dim)).astype(np.float32)
    want = reference_select(coarse_dists(q2, c), 300)
    assert np.array_equal(pyqadc.coarse_assign(q2, c, 300), want)
    q2[1, 0] = np.nan
    with pytest.raises(pyqadc.QadcError, match="NaN"):
        pyqadc.coarse_assign(q2, c, 300)


@path_independent
@pytest.mark.parametrize("dim,opq", [(32, False), (32, True), (48, True)])
def test_ivf_encode_on_nan_centroids_codebooks_and_vectors(pyqadc, dim, opq):
    """qadc_ivf_encode_host with NaN coarse rows, NaN codebook entries (centroid 0, a middle one, 15) and vectors with a NaN
    component: assign = the reference's k = 1 selection, codes = the oracle's encoder (its compiled replace test) on the residuals."""
    rng = np.random.default_rng(dim + 7 * opq)
    M, K, n = 16, 70, 1500
    ds = dim // M
    cb = rng.normal(size=(M, 16, ds)).astype(np.float32)
    cb[0, 0, 0] = NAN_POS
    cb[1, 8, :] = NAN_NEG
    cb[2, 15, ds - 1] = NAN_POS
    cb[5, 0] = np.nan
    cb[5, 15] = np.nan
    coarse = rng.normal(size=(K, dim)).astype(np.float32)
    coarse[0] = NAN_POS
    coarse[K // 2, 3] = NAN_NEG
    coarse[K - 1] = NAN_NEG
    v = rng.normal(size=(n, dim)).astype(np.float32)
    v[::17, 5] = np.nan
    v[3::23] *= np.float32(1e20)
    rot = (rng.normal(size=(dim, dim)) * 0.3).astype(np.float32) if opq else None
    assign, codes = pyqadc.ivf_encode(cb, v, coarse=coarse, rotation=rot)
    assert ((assign >= 0) & (assign < K)).all()
    want_assign = reference_select(coarse_dists(v, coarse), 1)[:, 0]
    assert np.array_equal(assign, want_assign)
    with np.errstate(invalid="ignore", over="ignore"):
        res = (v - coarse[want_assign]).astype(np.float32)
    assert np.array_equal(codes, po.pq_encode(cb, res, rot))
    _, flat = pyqadc.ivf_encode(cb, v)
    assert np.array_equal(flat, po.pq_encode(cb, v))


@path_independent
@pytest.mark.parametrize("dim", [32, 30])
def test_kmeans_iterations_through_an_empty_cluster(pyqadc, dim):
    """Three k-means rounds from seeds with a duplicated centroid: cluster 1 is empty in round 1 (an exact tie keeps centroid
    0), its centroid is NaN from round 2 on, and the assignment then follows the reference's NaN rule.  Compared with a CPU loop
    of the reference's selection and its compiled centroid update (sum * (1 / count))."""
    rng = np.random.default_rng(dim)
    n, K = 2000, 20
    v = rng.normal(size=(n, dim)).astype(np.float32)
    seed = v[:K].copy()
    seed[1] = seed[0]
    cen, asg = pyqadc.kmeans_iterations(v, seed, 3)
    c = seed.copy()
    for it in range(3):
        a = reference_select(coarse_dists(v, c), 1)[:, 0]
        if it == 0:
            assert not (a == 1).any()
        s = np.zeros_like(c)
        cnt = np.zeros(K, np.int64)
        for i in range(n):
            s[a[i]] = (s[a[i]] + v[i]).astype(np.float32)
            cnt[a[i]] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            nxt = (s * (np.float32(1.0) / cnt[:, None].astype(np.float32)).astype(np.float32)).astype(np.float32)
        if po.have_ref_float():
            assert np.array_equal(po.reff_kmeans_update(v, a, K), nxt, equal_nan=True)
        c = nxt
    assert np.isnan(c[1]).all()
    assert ((asg >= 0) & (asg < K)).all()
    assert np.array_equal(asg, a) and np.array_equal(cen, c, equal_nan=True)


@path_independent
@pytest.mark.parametrize("M,dim", [(32, 1024), (16, 2048)])
@pytest.mark.parametrize("form", [0, 1])
def test_pq_encode_above_64k_of_lds(pyqadc, M, dim, form):
    """The encoder keeps the codebooks in LDS: 128 KiB (+ 2 KiB of norms for form 1) at these shapes, above the default 64 KiB
    dynamic-LDS limit."""
    rng = np.random.default_rng(M + dim + form)
    cb = rng.normal(size=(M, 16, dim // M)).astype(np.float32)
    v = rng.normal(size=(200, dim)).astype(np.float32)
    v[7, 3] = np.nan
    assert np.array_equal(pyqadc.pq_encode(cb, v, encode_form=form), po.pq_encode(cb, v, form=form))
    with pytest.raises(pyqadc.QadcError):
        pyqadc.pq_encode(rng.normal(size=(16, 16, 129)).astype(np.float32), rng.normal(size=(2, 16 * 129)).astype(np.float32))
