"""GPU: learning a product quantizer of 16-bit sub-quantizers (qadc_pq_train16_host / _device, qadc_pq_update16_host;
pyqadc.train_pq16, train_pq16_device, pq_update16).

Every float is compared bit for bit (adc_compose.assert_same_floats: a NaN matches any NaN).  The expectation is
tests/pq_train16_compose.py: the oracle's assignment (adc16_encode_compose.codes16) and a sequential float32 sum per cluster in
ascending vector index.  Where a full CPU oracle would take minutes (65536 live clusters), a round is checked in two halves: its
codes against the existing 16-bit encoder on the codebooks of the round before (the encoder is pinned to the oracle by
test_gpu_adc16_encode.py), its codebooks against the compose update of those codes."""
import ctypes as C

import numpy as np
import pytest

import adc_compose as ac
import pq_train16_compose as p16
import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

K16 = 65536
UPDATE_SHAPES = {"2x16-d8": (2, 8), "2x16-d6": (2, 6), "2x16-d128": (2, 128), "2x16-d192": (2, 192), "8x16-d16": (8, 16)}   # dsub 4, 3, 64, 96, 2
EDGES = np.array([0, 1, 255, 256, 257, 65280, 65535], np.uint16)                     # both radix digits' edges


def crafted_codes(pattern, n, nsq, rng):
    if pattern.startswith("all-"):
        return np.full((n, nsq), int(pattern[4:]), np.uint16)
    if pattern == "mod":
        return np.ascontiguousarray(np.broadcast_to((np.arange(n) % K16).astype(np.uint16)[:, None], (n, nsq)))
    return rng.choice(EDGES, size=(n, nsq))


def assert_update(v, codes, nsq, div_mode, what=""):
    want_cb, want_counts = p16.update(v, codes, div_mode)
    cb, counts = pyqadc.pq_update16(v, codes, nsq, div_mode=div_mode)
    assert np.array_equal(counts, want_counts), "%s: cluster sizes differ" % what
    ac.assert_same_floats(cb, want_cb, "%s: codebooks against the compose update" % what)
    return cb


# ---- 1. the update alone, crafted codes --------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("pattern", ["all-0", "all-255", "all-256", "all-65535", "mod", "edges"])
@pytest.mark.parametrize("n", [1, 255, 1025, 70000])
@pytest.mark.parametrize("shape", sorted(UPDATE_SHAPES))
def test_update_alone_on_crafted_codes(shape, n, pattern):
    nsq, dim = UPDATE_SHAPES[shape]
    rng = np.random.default_rng([nsq, dim, n, len(pattern)])
    v = rng.normal(size=(n, dim)).astype(np.float32)
    codes = crafted_codes(pattern, n, nsq, rng)
    for div_mode in (1, 0):
        cb = assert_update(v, codes, nsq, div_mode, "%s n %d %s div_mode %d" % (shape, n, pattern, div_mode))
        live = np.zeros((nsq, K16), bool)
        for m in range(nsq):
            live[m, codes[:, m]] = True
        assert np.array_equal(np.isnan(cb).all(axis=2), ~live) and np.array_equal(np.isnan(cb).any(axis=2), ~live)


@path_independent
@pytest.mark.parametrize("div_mode", [1, 0])
def test_update_sums_in_ascending_vector_index(div_mode):
    """values of mixed magnitude: the sum taken in descending order differs, so a wrong order cannot pass"""
    rng = np.random.default_rng(17)
    n, nsq, dim = 5000, 2, 6
    v = rng.choice(np.array([-1, 1], np.float32), size=(n, dim)) * rng.random((n, dim)).astype(np.float32)
    big = rng.random((n, dim)) < 0.2
    v[big] = (rng.choice(np.array([-1e8, 1e8], np.float32), size=int(big.sum())) * rng.random(int(big.sum())).astype(np.float32))
    codes = rng.choice(EDGES, size=(n, nsq))
    ascending = p16.update(v, codes, div_mode)[0]
    descending = p16.update(v, codes, div_mode, descending=True)[0]
    assert not np.array_equal(ascending.view(np.uint32), descending.view(np.uint32))
    assert_update(v, codes, nsq, div_mode, "mixed magnitude")


# ---- 2. one round and two, full CPU oracle -----------------------------------------------------------------------------------

SMALL = {"2x16-d8": (2, 8), "8x16-d16": (8, 16)}


def small_case(shape, seed=0):
    nsq, dim = SMALL[shape]
    rng = np.random.default_rng([nsq, dim, seed])
    return rng, rng.normal(size=(700, dim)).astype(np.float32), rng.normal(size=(nsq, K16, dim // nsq)).astype(np.float32)


def assert_training(po, x, v, seed, iters, sum_mode=1, div_mode=1, **front):
    want_cb, want_codes, _ = p16.train(po, x, seed, iters, div_mode, sum_mode)
    cb, codes, empty = pyqadc.train_pq16(v, seed, iters, div_mode=div_mode, sum_mode=sum_mode, **front)
    assert codes.dtype == np.uint16 and np.array_equal(codes, want_codes), "codes after %d rounds" % iters
    ac.assert_same_floats(cb, want_cb, "codebooks after %d rounds" % iters)
    assert empty == p16.empty_count(want_cb)
    return cb, codes, empty


@path_independent
@pytest.mark.parametrize("sum_mode", [1, 0])
@pytest.mark.parametrize("shape", sorted(SMALL))
def test_rounds_match_the_full_oracle(po, shape, sum_mode):
    """the second round runs on codebooks that are mostly NaN: the heap takes the first smallest after the last NaN"""
    _, v, seed = small_case(shape)
    assert_training(po, v, v, seed, 1, sum_mode)
    cb, _, empty = assert_training(po, v, v, seed, 2, sum_mode)
    assert empty >= seed.shape[0] * (K16 - 700) and np.isnan(cb).any()


@path_independent
def test_division_as_the_source_reads(po):
    _, v, seed = small_case("2x16-d8", seed=3)
    assert_training(po, v, v, seed, 1, div_mode=0)


# ---- 3. several rounds, every cluster alive ----------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(2, 8, 70000), (4, 32, 98304)], ids=["2x16-d8-n70000", "4x16-d32-n98304"])
def test_rounds_with_every_cluster_alive(shape):
    nsq, dim, n = shape
    rng = np.random.default_rng([nsq, dim, n])
    v = rng.standard_normal((n, dim), dtype=np.float32)
    seed = p16.seed_rows(v, nsq, rng.choice(n, K16, replace=False))
    before = seed
    for r in (1, 2, 3):
        cb, codes, empty = pyqadc.train_pq16(v, seed, r)
        assert np.array_equal(codes, pyqadc.adc_encode16(before, v)[1]), "round %d: the codes are not the encoder's" % r
        ac.assert_same_floats(cb, p16.update(v, codes)[0], "round %d: the codebooks against the compose update of its codes" % r)
        assert empty == 0, "round %d emptied %d clusters" % (r, empty)
        before = cb


# ---- 4. the front ------------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("opq", [False, True], ids=["residual", "residual-opq"])
def test_training_on_the_rotated_residual(po, opq):
    rng, v, seed = small_case("2x16-d8", seed=5 + opq)
    coarse = v[rng.choice(len(v), 20, replace=False)].copy()
    rot = ac.random_rotation(rng, v.shape[1]) if opq else None
    x = ac.residuals(v, coarse, ac.assign(po, v, coarse, 1), rot)[:, 0, :]
    assert_training(po, x, v, seed, 1, coarse=coarse, rotation=rot)


# ---- 5. the device form ------------------------------------------------------------------------------------------------------

@path_independent
def test_device_form_returns_the_host_forms_bits():
    import torch
    rng, v, seed = small_case("8x16-d16", seed=7)
    coarse = v[:20].copy()
    want = pyqadc.train_pq16(v, seed, 2, coarse=coarse)
    t = torch.from_numpy(v).to("cuda:0")
    keep = t.clone()
    got = pyqadc.train_pq16_device(t, seed, 2, coarse=coarse)
    ac.assert_same_floats(got[0], want[0])
    assert np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert torch.equal(t, keep)
    with pytest.raises(TypeError):
        pyqadc.train_pq16_device(v, seed, 1)
    with pytest.raises(pyqadc.QadcError):
        pyqadc.train_pq16_device(t.t(), seed, 1)


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------

@path_independent
def test_the_same_call_twice_and_a_good_call_after_a_refused_one():
    rng = np.random.default_rng(9)
    n, nsq, dim = 70000, 2, 8
    v = rng.standard_normal((n, dim), dtype=np.float32)
    seed = p16.seed_rows(v, nsq, rng.choice(n, K16, replace=False))
    first = pyqadc.train_pq16(v, seed, 2)
    with pytest.raises(pyqadc.QadcError, match="iters"):
        pyqadc.train_pq16(v, seed, -1)
    lib = pyqadc.lib()
    assert lib.qadc_pq_update16_host(v.ctypes.data_as(C.POINTER(C.c_float)), n, dim, nsq, None, seed.ctypes.data_as(C.POINTER(C.c_float)),
                                     None, 1, 0) == pyqadc.QADC_E_ARG
    again = pyqadc.train_pq16(v, seed, 2)
    assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32)) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    a, b = pyqadc.pq_update16(v, first[1], nsq), pyqadc.pq_update16(v, first[1], nsq)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), first[0].view(np.uint32))       # the update of the last round's codes is the result


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------

@path_independent
def test_trained_codebooks_build_and_search_an_index():
    rng = np.random.default_rng(11)
    n, nsq, dim, R, nq = 70000, 2, 8, 50, 4
    v = rng.standard_normal((n, dim), dtype=np.float32)
    seed = p16.seed_rows(v, nsq, rng.choice(n, K16, replace=False))
    errs = []
    for r in (1, 3):
        cb, _, empty = pyqadc.train_pq16(v, seed, r)
        assert empty == 0
        errs.append(p16.reconstruction_error(v, cb, pyqadc.adc_encode16(cb, v)[1]))
    assert errs[1] <= errs[0], "the reconstruction error rose from round 1 (%r) to round 3 (%r)" % tuple(errs)
    queries = v[rng.choice(n, nq, replace=False)] + np.float32(0.01)
    got, ref = pyqadc.AdcIndex.create16(nsq), pyqadc.AdcIndex.create16(nsq)
    try:
        for idx in (got, ref):
            idx.set_pq(cb)
            idx.set_coarse(None)
        got.add_vectors(v)
        ref.add_partitions([pyqadc.adc_encode16(cb, v)[1]])
        res, want = got.search(queries, 1, R), ref.search(queries, 1, R)
        for x, y in zip(res, want):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
        assert (res[2] == R).all()
    finally:
        got.close()
        ref.close()
