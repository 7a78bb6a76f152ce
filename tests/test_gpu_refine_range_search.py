"""GPU: an index's range search, then the exact radius (AdcIndex.range_search_refined and .range_search_refined_device; DESIGN.md
section 11.21) on the clustered 32-d set of tests/test_gpu_refine_search.py: an 8x8 IVF index, a float-ADC view of a 16x4 Index and
a 4x16 index.  The composition equals its parts: range_search, range_collect, then the host twin's rerank_range
(tests/cpp/refine_range_host.cpp) on what they returned — for equality."""
import numpy as np
import pytest

import refine_range_cases as rr
from helpers import path_independent
from test_gpu_refine_search import DIM, N, NQ, World

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = ["8x8", "16x4 view", "4x16"]


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return rr.build_driver()


@pytest.fixture(scope="module")
def world(pyqadc):
    w = World(pyqadc)
    yield w
    w.close()


def as_result(lims, keys, dist, missing):
    if not isinstance(keys, np.ndarray):
        keys, dist = keys.cpu().numpy().view(np.uint32), dist.cpu().numpy()
    return dict(lims=np.asarray(lims).astype(np.uint64), keys=keys, dist=dist, missing=missing)


def radii(idx, world, ma, rows):
    """per query an ADC radius that keeps about `rows` rows: the largest value of its own heap of that many"""
    _, vals, _, _ = idx.search(world.queries, ma, rows)
    return vals.max(axis=1).astype(F32)


def twin_of(world, twin, tmp_path, dtype, lims, keys, radius):
    segs = [keys[int(lims[q]):int(lims[q + 1])] for q in range(NQ)]
    c = rr.dense_case(DIM, dtype, 0, world.vectors, [rr.rerank_range(world.queries, segs, radius)])
    return rr.run_twin(twin, tmp_path, [c])[0][0]


@path_independent
@pytest.mark.parametrize("shape", SHAPES)
def test_the_composition_equals_its_parts(world, twin, tmp_path, shape):
    import torch
    idx = world.adc(shape)
    ma = 4
    adc_radius = radii(idx, world, ma, 600)
    lims, keys, vals = idx.range_search(world.queries, ma, adc_radius)
    k2, _ = idx.range_collect(lims)
    assert np.array_equal(k2, keys) and 300 * NQ < int(lims[-1])
    exact = np.sort(((world.vectors[None, :, :] - world.queries[:, None, :]) ** 2).sum(-1), axis=1)[:, 150].astype(F32)
    dq = torch.from_numpy(world.queries).cuda()
    for dtype in ("f32", "f16"):
        want = twin_of(world, twin, tmp_path, dtype, lims, keys, exact)
        got = as_result(*idx.range_search_refined(world.queries, ma, adc_radius, exact, world.stores[dtype]))
        dev = as_result(*idx.range_search_refined_device(dq, ma, adc_radius, exact, world.stores[dtype]))
        assert rr.same(got, want) is None and rr.same(dev, want) is None, (shape, dtype)
        kept = rr.kept(want)
        assert want["missing"] == 0 and (kept > 0).all() and (kept <= 155).all() and kept.sum() < int(lims[-1])


@path_independent
def test_per_query_filters_hold_for_the_refined_rows(world, twin, tmp_path, pyqadc):
    import torch
    idx = world.adc("8x8")
    rng = np.random.default_rng(41)
    ma = 4
    adc_radius = radii(idx, world, ma, 800)
    allowed = np.sort(rng.permutation(N)[:N // 2]).astype(np.uint32)
    f = pyqadc.AdcFilter(allowed, "allow")
    filters = [f if q % 2 else None for q in range(NQ)]
    try:
        lims, keys, _ = idx.range_search(world.queries, ma, adc_radius, filters=filters)
        got = as_result(*idx.range_search_refined(world.queries, ma, adc_radius, np.inf, world.stores["f32"], filters=filters))
        dev = as_result(*idx.range_search_refined_device(torch.from_numpy(world.queries).cuda(), ma, adc_radius, np.inf, world.stores["f32"],
                                                         filters=filters))
    finally:
        f.close()
    want = twin_of(world, twin, tmp_path, "f32", lims, keys, np.inf)
    assert rr.same(got, want) is None and rr.same(dev, want) is None
    for q in range(NQ):
        mine = got["keys"][int(got["lims"][q]):int(got["lims"][q + 1])]
        assert np.isin(mine, allowed).all() == bool(q % 2) or len(mine) == 0, q
    assert rr.kept(got).sum() == int(lims[-1]), "under radius +inf every ADC row with a finite distance stays (the keys differ)"


@path_independent
def test_a_label_in_two_partitions_comes_out_once(world, twin, tmp_path, pyqadc):
    """two partitions that hold the same vectors under the same labels: the ADC result lists a key twice, the refined result once"""
    n = 3000
    _, codes = pyqadc.adc_encode(world.cb8, world.vectors[:n])   # (flat codes under two coarse centroids: the ADC values mean little, and need not)
    labels = np.arange(n, dtype=np.uint32)
    idx = pyqadc.AdcIndex(8, 8)
    idx.set_pq(world.cb8)
    idx.set_coarse(np.stack([world.vectors[:n].mean(0), world.vectors[:n].mean(0) + F32(0.01)]).astype(F32))
    idx.add_partitions([codes, codes], labels=[labels, labels])
    st = pyqadc.Refine(DIM, "f32")
    st.add(world.vectors[:n], 0)
    try:
        adc_radius = np.full(NQ, 1e30, F32)
        lims, keys, _ = idx.range_search(world.queries, 2, adc_radius)
        assert int(lims[-1]) == 2 * n * NQ
        got = as_result(*idx.range_search_refined(world.queries, 2, adc_radius, np.inf, st))
    finally:
        idx.close()
        st.close()
    c = rr.dense_case(DIM, "f32", 0, world.vectors[:n], [rr.rerank_range(world.queries, [keys[int(lims[q]):int(lims[q + 1])] for q in range(NQ)], np.inf)])
    want = rr.run_twin(twin, tmp_path, [c])[0][0]
    assert rr.same(got, want) is None and rr.kept(got).tolist() == [n] * NQ
