"""GPU: the cross matrix of OPQ learning (qadc_opq_cross_host / _device; pyqadc.opq_cross, opq_cross_device).

M is compared bit for bit (float64) with the host twin (quick-adc_amd/host/db_build.hpp opq_cross, through tests/cpp/opq_host.cpp):
per block of 2048 vectors one float fmaf chain per (a, b) in ascending vector index, the blocks added in float64."""
import numpy as np
import pytest

import opq_compose as oc
import pq_train_compose as ptc
import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

SHAPES = {"16x4-d32": (16, 4, 32), "32x4-d96": (32, 4, 96),          # dsub 3
          "4x8-d32": (4, 8, 32), "16x8-d48": (16, 8, 48),
          "4x8-d200": (4, 8, 200)}                                   # dim is no multiple of any tile: four tiles per edge, the last 8 wide
SIZES = [1, oc.BLOCK - 1, oc.BLOCK, oc.BLOCK + 1, 2 * oc.BLOCK + 1]


@pytest.fixture(scope="module")
def driver():
    return oc.build_driver()


def make(nsq, bits, dim, n, seed=0, coarse=False, spread=False):
    rng = np.random.default_rng([nsq, bits, dim, n, seed])
    v = rng.normal(size=(n, dim)).astype(np.float32)
    if spread:
        v[rng.choice(n, n // 10, replace=False)] *= np.float32(1e3)
    cb = rng.normal(size=(nsq, 1 << bits, dim // nsq)).astype(np.float32)
    a = rng.integers(0, 1 << bits, (n, nsq))
    a[0], a[-1] = 0, (1 << bits) - 1                                 # centroid 0 and the last centroid, in every sub-quantizer
    co = rng.normal(size=(7, dim)).astype(np.float32) if coarse else None
    return v, ptc.pack(a, bits), cb, co


@path_independent
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_cross_matches_the_twin(driver, tmp_path, shape, n):
    v, codes, cb, _ = make(*SHAPES[shape], n)
    M = pyqadc.opq_cross(v, codes, cb)
    assert M.dtype == np.float64 and M.shape == (v.shape[1], v.shape[1])
    oc.same_doubles(M, oc.twin_cross(driver, tmp_path, v, codes, cb), "M against the twin")


@path_independent
@pytest.mark.parametrize("shape,n", [("16x4-d32", oc.BLOCK + 1), ("4x8-d200", 300), ("16x8-d48", 2 * oc.BLOCK + 1)])
def test_cross_on_the_residual_to_a_coarse_quantizer(driver, tmp_path, shape, n):
    v, codes, cb, co = make(*SHAPES[shape], n, seed=1, coarse=True)
    M = pyqadc.opq_cross(v, codes, cb, coarse=co)
    oc.same_doubles(M, oc.twin_cross(driver, tmp_path, v, codes, cb, co), "M on the residual")
    assert (M != pyqadc.opq_cross(v, codes, cb)).any()               # the coarse quantizer takes part


@path_independent
@pytest.mark.parametrize("shape", ["32x4-d96", "4x8-d32"])
def test_the_device_form_equals_the_host_form(shape):
    import torch
    v, codes, cb, co = make(*SHAPES[shape], oc.BLOCK + 77, seed=2, coarse=True)
    t = torch.from_numpy(v).to("cuda:0")
    for coarse in (None, co):
        want = pyqadc.opq_cross(v, codes, cb, coarse=coarse)
        oc.same_doubles(pyqadc.opq_cross_device(t, codes, cb, coarse=coarse), want)
        oc.same_doubles(pyqadc.opq_cross_device(t, codes, cb, coarse=coarse), want)
    assert np.array_equal(t.cpu().numpy(), v)                        # the learning set is read only
    with pytest.raises(pyqadc.QadcError):
        pyqadc.opq_cross_device(torch.from_numpy(v), codes, cb)      # a host tensor


@path_independent
@pytest.mark.parametrize("shape", ["16x4-d32", "4x8-d200"])
def test_the_comparison_sees_the_order_of_the_sums(driver, tmp_path, shape):
    """a tenth of the rows scaled by 10^3: the chains taken in descending vector index give another matrix, so a kernel that adds in
    another order (atomics, a tree, chains split between lanes or workgroups) cannot pass"""
    n = 2 * oc.BLOCK + 1
    v, codes, cb, _ = make(*SHAPES[shape], n, seed=3, spread=True)
    y = oc.reconstruction(cb, codes)
    want = oc.chain(driver, tmp_path, v, y)
    assert (want != oc.chain(driver, tmp_path, v, y, descending=True)).any()
    oc.same_doubles(oc.twin_cross(driver, tmp_path, v, codes, cb), want, "the twin against the plain chains")
    oc.same_doubles(pyqadc.opq_cross(v, codes, cb), want, "M against the plain chains")
