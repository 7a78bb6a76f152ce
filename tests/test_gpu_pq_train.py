"""GPU: learning the product quantizer (qadc_pq_train_host / _device; pyqadc.train_pq, train_pq_device).

Every float is compared bit for bit (adc_compose.assert_same_floats: a NaN matches any NaN).  Primary expectation: the numpy /
oracle loop of tests/pq_train_compose.py.  Second expectation: the route without this call — pyqadc.kmeans_iterations on every host
slice.  The returned codes are the encoder's under the codebooks of before the last update."""
import numpy as np
import pytest

import adc_compose as ac
import pq_train_compose as ptc
import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

STEP = 256                                                       # vectors the update kernel stages per step at the shapes below
SHAPES = {                                                       # (sq_count, bits, dim, n)
    "16x4-d32": (16, 4, 32, 3000), "16x4-d64": (16, 4, 64, 2500), "32x4-d96": (32, 4, 96, 2000),   # dsub 3: the any-size norm path
    "4x8-d32": (4, 8, 32, 12000), "8x8-d32": (8, 8, 32, 11000), "16x8-d48": (16, 8, 48, 10500),
}
SMALL = dict(("%s-n%d" % (name, n), (nsq, bits, dim, n)) for name, (nsq, bits, dim) in (("16x4-d32", (16, 4, 32)), ("4x8-d32", (4, 8, 32)))
             for n in (1, STEP - 1, STEP, STEP + 1))
# sub-vectors wide enough that a workgroup stages fewer vectors per step (host/pq_train_plan.hpp): n sits one past a step
WIDE = {"4x8-d96-step128": (4, 8, 96, 2 * 128 + 1), "4x8-d160-step64": (4, 8, 160, 4 * 64 + 1), "16x4-d2048-step32": (16, 4, 2048, 6 * 32 + 1),
        "4x8-d1200-step16-two-windows": (4, 8, 1200, 17 * 16 + 1)}


def make(nsq, bits, dim, n, seed=0, distinct=True):
    rng = np.random.default_rng([nsq, bits, dim, n, seed])
    v = rng.normal(size=(n, dim)).astype(np.float32)
    K = 1 << bits
    if distinct and n >= K:
        return v, ptc.seed_rows(v, nsq, bits, rng.choice(n, K, replace=False))
    return v, rng.normal(size=(nsq, K, dim // nsq)).astype(np.float32)


def slices_route(v, seed, iters, div_mode=1):
    """what the library offered before: one k-means per host slice"""
    nsq, K, ds = seed.shape
    cb = np.zeros_like(seed)
    assign = np.zeros((v.shape[0], nsq), np.int32)
    for m in range(nsq):
        cb[m], assign[:, m] = pyqadc.kmeans_iterations(np.ascontiguousarray(v[:, m * ds:(m + 1) * ds]), seed[m], iters, div_mode=div_mode)
    return cb, ptc.pack(assign, {16: 4, 256: 8}[K])


def encoder(codebooks, x):
    return pyqadc.pq_encode(codebooks, x) if codebooks.shape[1] == 16 else pyqadc.adc_encode(codebooks, x)[1]


def check_case(po, v, seed, iters, div_mode, no_nan=False):
    want_cb, want_codes, before = ptc.train(po, v, seed, iters, div_mode)
    if no_nan:
        assert not np.isnan(want_cb).any()                       # (on the CPU expectation: the seeds are distinct data rows)
    cb, codes, empty = pyqadc.train_pq(v, seed, iters, div_mode=div_mode)
    ac.assert_same_floats(cb, want_cb, "codebooks against the oracle loop")
    assert np.array_equal(codes, want_codes)
    assert empty == ptc.empty_count(want_cb)
    cb2, codes2 = slices_route(v, seed, iters, div_mode)
    ac.assert_same_floats(cb, cb2, "codebooks against k-means per slice")
    assert np.array_equal(codes, codes2)
    if not np.isnan(before).any():
        assert np.array_equal(codes, encoder(before, v))         # the codes of the codebooks of before the last update
    return cb, codes


@path_independent
@pytest.mark.parametrize("div_mode", [1, 0])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_training_matches_the_oracle_loop_and_the_slices(po, shape, iters, div_mode):
    v, seed = make(*SHAPES[shape])
    check_case(po, v, seed, iters, div_mode, no_nan=True)


@path_independent
@pytest.mark.parametrize("div_mode", [1, 0])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("shape", sorted(SMALL) + sorted(WIDE))
def test_training_around_a_step_of_the_update_kernel(po, shape, iters, div_mode):
    """n = 1, and one below, at and above the vectors staged per step; clusters empty out here and the NaN centroids take part"""
    v, seed = make(*dict(SMALL, **WIDE)[shape])
    check_case(po, v, seed, iters, div_mode)


@path_independent
@pytest.mark.parametrize("shape", ["16x4-d32", "8x8-d32"])
def test_the_comparison_sees_the_order_of_the_sums(po, shape):
    """a tenth of the rows scaled by 10^3: summing the members of a cluster in descending vector index changes the expectation, so an
    update that adds in another order (atomics, a tree, per-wave partial sums) cannot pass"""
    nsq, bits, dim, n = SHAPES[shape]
    rng = np.random.default_rng([3, nsq])
    v = rng.normal(size=(n, dim)).astype(np.float32)
    v[rng.choice(n, n // 10, replace=False)] *= np.float32(1e3)
    seed = ptc.seed_rows(v, nsq, bits, rng.choice(n, 1 << bits, replace=False))
    want_cb = ptc.train(po, v, seed, 1)[0]
    other = ptc.train(po, v, seed, 1, descending=True)[0]
    assert not np.isnan(want_cb).any()
    assert (want_cb.view(np.uint32) != other.view(np.uint32)).any()
    for iters in (1, 3):
        check_case(po, v, seed, iters, 1)


@path_independent
@pytest.mark.parametrize("shape", ["16x4-d32", "4x8-d32"])
def test_an_empty_cluster_becomes_nan_and_stays(po, shape):
    nsq, bits, dim, n = SHAPES[shape]
    v, seed = make(nsq, bits, dim, n, seed=1)
    seed[2, 1] = seed[2, 0]                                      # an equal distance does not replace: centroid 1 of sub-quantizer 2 gets nobody
    for iters in (1, 2, 3):
        want_cb = ptc.train(po, v, seed, iters)[0]
        assert np.isnan(want_cb[2, 1]).all()
        cb, codes = check_case(po, v, seed, iters, 1)
        assert np.isnan(cb[2, 1]).all()
        assert pyqadc.train_pq(v, seed, iters)[2] == ptc.empty_count(want_cb) >= 1
    # from round 2 on the assignment follows the compiled replace test on a NaN distance: the NaN centroid takes over from every
    # earlier one and loses to the next, so nobody is assigned to centroids 0 and 1 of that sub-quantizer
    a = ptc.unpack(pyqadc.train_pq(v, seed, 2)[1], bits)[:, 2]
    assert not np.isin(a, (0, 1)).any()


@path_independent
def test_a_learning_set_longer_than_one_pass_of_the_build_calls():
    """n = 262144 + 37 (the other build calls take passes of 262144 vectors), one round, against k-means per slice only: the Python
    loop would be too slow here"""
    n = pyqadc.QADC_INDEX_ADD_CHUNK + 37
    v, seed = make(16, 4, 16, n)
    cb, codes, empty = pyqadc.train_pq(v, seed, 1)
    cb2, codes2 = slices_route(v, seed, 1)
    ac.assert_same_floats(cb, cb2)
    assert np.array_equal(codes, codes2) and empty == ptc.empty_count(cb2)


@path_independent
@pytest.mark.parametrize("opq", [False, True], ids=["residual", "residual-opq"])
@pytest.mark.parametrize("shape", ["16x4-d32", "8x8-d32"])
def test_training_on_the_residual_and_the_rotated_residual(po, shape, opq):
    nsq, bits, dim, _ = SHAPES[shape]
    n, K = 3000, 20
    rng = np.random.default_rng([9, nsq, int(opq)])
    v = rng.normal(size=(n, dim)).astype(np.float32)
    coarse = v[rng.choice(n, K, replace=False)].copy()
    rot = ac.random_rotation(rng, dim) if opq else None
    x = ac.residuals(v, coarse, ac.assign(po, v, coarse, 1), rot)[:, 0, :]
    seed = ptc.seed_rows(x, nsq, bits, rng.choice(n, 1 << bits, replace=False))
    want_cb, want_codes, _ = ptc.train(po, x, seed, 2)
    cb, codes, empty = pyqadc.train_pq(v, seed, 2, coarse=coarse, rotation=rot)
    ac.assert_same_floats(cb, want_cb)
    assert np.array_equal(codes, want_codes) and empty == ptc.empty_count(want_cb)


@path_independent
@pytest.mark.parametrize("shape", ["16x4-d64", "16x8-d48"])
def test_the_device_form_equals_the_host_form(shape):
    import torch
    nsq, bits, dim, n = SHAPES[shape]
    v, seed = make(nsq, bits, dim, n, seed=2)
    coarse = v[:20].copy()
    want = pyqadc.train_pq(v, seed, 3, coarse=coarse)
    t = torch.from_numpy(v).to("cuda:0")
    got = pyqadc.train_pq_device(t, seed, 3, coarse=coarse)
    again = pyqadc.train_pq_device(t, seed, 3, coarse=coarse)
    assert np.array_equal(t.cpu().numpy(), v)                    # the learning set is read only
    for g in (got, again):
        ac.assert_same_floats(g[0], want[0])
        assert np.array_equal(g[1], want[1]) and g[2] == want[2]
    with pytest.raises(TypeError):
        pyqadc.train_pq_device(v, seed, 1)
    with pytest.raises(pyqadc.QadcError):
        pyqadc.train_pq_device(torch.from_numpy(v), seed, 1)     # a host tensor


def clustered(rng, n, dim):
    """tools/adc_bench.clustered at a small size: vectors around 50 centres"""
    centers = (rng.normal(size=(50, dim)) * 3).astype(np.float32)
    return centers[rng.integers(0, len(centers), n)] + rng.normal(size=(n, dim)).astype(np.float32)


@path_independent
@pytest.mark.parametrize("bits", [4, 8])
def test_trained_codebooks_reconstruct_better_and_serve_an_index(po, bits):
    rng = np.random.default_rng(bits)
    n, dim, K, nsq = 6000, 32, 8, 16 if bits == 4 else 8
    v = clustered(rng, n, dim)
    coarse = v[rng.choice(n, K, replace=False)].copy()
    x = ac.residuals(v, coarse, ac.assign(po, v, coarse, 1))[:, 0, :]
    seed = pyqadc.pq_seed(x, nsq, bits, rng)
    cb, codes, empty = pyqadc.train_pq(v, seed, 5, coarse=coarse)
    assert empty == 0
    before = ptc.reconstruction_error(x, seed, encoder(seed, x))
    after = ptc.reconstruction_error(x, cb, codes)
    assert after < before, (after, before)
    idx = pyqadc.Index(nsq) if bits == 4 else pyqadc.AdcIndex(nsq, 8)
    try:
        idx.set_pq(cb)
        idx.set_coarse(coarse)
        idx.add_vectors(v)
        if bits == 4:
            idx.finalize(0.5)
            r = idx.search(v[:4], 2, 10)
            assert (r["status"] == 0).all() and (r["sizes"] == 10).all() and (r["keys"] < n).all()
        else:
            keys, vals, sizes, _ = idx.search(v[:4], 2, 10)
            assert (sizes == 10).all() and (keys < n).all()
    finally:
        idx.close()
