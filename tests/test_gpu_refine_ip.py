"""GPU: re-ranking by inner product (pyqadc.Refine(metric="ip").rerank and .rerank_device over qadc_refine_rerank*; DESIGN.md section
11.23) against the host twin (refine::rerank of quick-adc_amd/host/refine.hpp with metric kIP through tests/cpp/refine_ip_host.cpp):
keys, the scores' bit patterns, sizes and the missing count, for equality — there is no tolerance anywhere.  Dense and keyed stores
of float, half and SQ8 rows, the strips of 64 components a lane walks, counts, skipped, missing and repeated entries, r_in 1 and
8192, and the scores the order has to cope with: both signs, +0, the non-finite ones and ties."""
import numpy as np
import pytest

import refine_ip_cases as ic
from helpers import path_independent

pytestmark = pytest.mark.gpu
GPU_DIMS = (1, 63, 64, 65, 128, 257, 4096)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return ic.build_driver()


def reranks(c):
    """the case with its rerank operations alone"""
    return dict(c, ops=[op for op in c["ops"] if op[0] == "rerank"])


def check(pyqadc, twin, tmp_path, cases, names=None):
    wants = ic.run_twin(twin, tmp_path, cases)
    for i, (c, want) in enumerate(zip(cases, wants)):
        what = names[i] if names else "case %d" % i
        ic.assert_same(ic.run_store(pyqadc, c), want, what + ", host form")
        ic.assert_same(ic.run_store(pyqadc, c, device=True), want, what + ", device form")
    return wants


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_dims_counts_skips_missing_and_repeated_keys(pyqadc, twin, tmp_path, dtype, keyed):
    rng = np.random.default_rng(3 + ic.DTYPES[dtype] + 5 * keyed)
    cases = [reranks(ic.random_case(rng, dim, dtype, keyed, rows=120 if dim < 4096 else 40)) for dim in GPU_DIMS]
    wants = check(pyqadc, twin, tmp_path, cases, ["dim %d" % d for d in GPU_DIMS])
    for w in wants:
        assert w[0]["missing"] == 3 and w[0]["sizes"].min() >= 8
        full = w[1]                                                            # R above the survivors: fillers -inf under key 0xFFFFFFFF
        n = full["sizes"][0]
        assert n < full["keys"].shape[1] and (full["keys"][0, n:] == ic.NO_KEY).all()
        assert (full["dist"][0, n:].view(np.uint32) == ic.NEG_INF_BITS).all() and (np.diff(full["dist"][0, :n]) <= 0).all()


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_r_in_1_and_8192(pyqadc, twin, tmp_path, dtype):
    rng = np.random.default_rng(17)
    dim, rows = 4, 1500
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    q = rng.normal(size=(3, dim)).astype(np.float32)
    wide = rng.integers(0, rows + 20, (3, 8192)).astype(np.uint32)            # most keys several times, some missing
    ops = [ic.rerank("ip", q, wide, 100), ic.rerank("ip", q, wide, 8192), ic.rerank("ip", q, [[5], [rows + 3], [7]], 1),
           ic.rerank("ip", q, [[5], [rows + 3], [7]], 4)]
    (want,) = check(pyqadc, twin, tmp_path, [ic.case(dim, dtype, vec, ops)])
    assert want[1]["sizes"].max() <= rows and want[1]["sizes"].min() > 1400 and want[0]["missing"] > 0
    assert want[2]["sizes"].tolist() == [1, 0, 1] and want[2]["missing"] == 1 and want[2]["keys"][1, 0] == ic.NO_KEY


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_signs_zeros_non_finite_scores_and_ties(pyqadc, twin, tmp_path, dtype, keyed):
    rng = np.random.default_rng(19)
    cases = [reranks(ic.sign_case(dtype, keyed)), reranks(ic.zero_case()), reranks(ic.overflow_case())]
    names = ["signs", "zeros", "overflow"]
    for dim in GPU_DIMS:
        cases += [reranks(ic.nonfinite_case(rng, dim, dtype)), reranks(ic.tie_case(rng, dim, dtype, keyed))]
        names += ["non-finite dim %d" % dim, "ties dim %d" % dim]
    wants = check(pyqadc, twin, tmp_path, cases, names)
    signs = wants[0][-1]                                                       # R = 9 over the scores 3, 2, 1, +0, +0, -1, -2, -3
    assert signs["keys"][0].tolist() == [10, 13, 15, 12, 16, 11, 17, 14, ic.NO_KEY]
    for res in wants[1]:
        assert not (res["dist"].view(np.uint32) == 0x80000000).any()           # no score is -0
    assert wants[2][0]["dist"][0].view(np.uint32).tolist() == [0x7F800000, 0x7F800000, 0, 0xFF800000, ic.NAN_BITS]
    assert (wants[3][0]["dist"][1].view(np.uint32)[:30] == ic.NAN_BITS).all()  # a NaN query: every score NaN, by key
    assert wants[4][1]["keys"][0].tolist() == [60, 61, 62, 63, 64]             # R = 5 cuts the tie, by key
