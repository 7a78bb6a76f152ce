"""GPU: the exact range search on a keyed refine store (DESIGN.md sections 11.14 and 11.21) against the host twin
(refine::keyed_store under refine::range and refine::rerank_range): after puts, overwrites and removes, with freed rows reused, a
removed key is absent from range and missing in rerank_range, and no slot, row or order of earlier puts shows in a result."""
import numpy as np
import pytest

import refine_range_cases as rr
from helpers import path_independent

pytestmark = pytest.mark.gpu

INF, F32 = rr.INF, np.float32


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return rr.build_driver()


def life(rng, dim, dtype, nq=5):
    labels = rng.choice(2 ** 32 - 1, 600, replace=False).astype(np.uint32)
    labels[:3] = (0, 0xFFFFFFFE, 0xFFFFFFFD)
    vec = rng.normal(size=(600, dim)).astype(F32)
    q = rng.normal(size=(nq, dim)).astype(F32)
    d = ((vec[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(-1)
    part = np.quantile(d, 0.4, axis=1).astype(F32)
    segs = [labels[:40], labels[30:320][::-1], np.concatenate([labels[:5], labels[:5], [7, 0xFFFFFFFF]]), [], labels[590:]][:nq]
    segs += [labels[:9]] * (nq - len(segs))
    ops = [rr.range_(q, INF), rr.rerank_range(q, segs, INF),                              # an empty keyed store
           rr.put(labels[:400], vec[:400]), rr.range_(q, INF), rr.range_(q, part), rr.rerank_range(q, segs, INF),
           rr.remove(labels[10:300:2]), rr.range_(q, INF), rr.rerank_range(q, segs, INF), rr.rerank_range(q, segs, part),
           rr.put(labels[250:], vec[:350] + F32(1)),                                      # overwrites, and new keys into the freed rows
           rr.range_(q, part * F32(2)), rr.range_(q, INF, ("exclude", labels[:300])), rr.range_(q, INF, ("allow", labels[280:330])),
           rr.range_(q, INF, ("allow", [])), rr.rerank_range(q, segs, part * F32(2)),
           rr.remove(labels), rr.range_(q, INF), rr.rerank_range(q, segs, INF),           # allocated rows, none live
           rr.put(labels[:2], vec[:2]), rr.range_(q, INF)]
    vmin, step = rr.sq_params(np.concatenate([vec, vec + F32(1)])) if dtype == "sq8" else (None, None)
    return rr.case(True, dim, dtype, ops, vmin, step), labels


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
@pytest.mark.parametrize("dim", [1, 65, 257])
def test_the_life_of_a_keyed_store(pyqadc, twin, tmp_path, dim, dtype):
    rng = np.random.default_rng(dim + rr.DTYPES[dtype])
    c, labels = life(rng, dim, dtype)
    (want,) = rr.run_twin(twin, tmp_path, [c])
    rr.assert_same(rr.run_store(pyqadc, c), want, "host form")
    rr.assert_same(rr.run_store(pyqadc, c, device=True, plan=(16, 64, 2)), want, "device form, regions of 16, chunks of 64, passes of 2")
    kept = [int(w["lims"][-1]) for w in want]
    assert kept[0] == 0 and kept[1] == 0 and want[1]["missing"] == len(c["ops"][1][3]), "on an empty store every candidate is missing"
    removed = set(labels[10:300:2].tolist())
    assert kept[2] == 5 * 400 and kept[5] == 5 * (400 - len(removed))
    assert not (set(want[5]["keys"].tolist()) & removed), "a removed key is absent from range"
    assert want[6]["missing"] > want[4]["missing"], "a removed key is missing in rerank_range"
    assert kept[13] == 0 and kept[14] == 0 and kept[15] == 5 * 2


@path_independent
def test_one_put_or_many_in_any_order_give_the_same_result(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(3)
    dim, n = 32, 900
    labels = rng.choice(2 ** 32 - 1, n, replace=False).astype(np.uint32)
    vec = rng.normal(size=(n, dim)).astype(F32)
    q = rng.normal(size=(4, dim)).astype(F32)
    segs = [labels[:700], labels[::-1], [], labels[5:6]]
    tail = [rr.range_(q, 50.0), rr.rerank_range(q, segs, 55.0)]
    order = rng.permutation(n)
    a = rr.case(True, dim, "f32", [rr.put(labels, vec)] + tail)
    b = rr.case(True, dim, "f32", [rr.put(labels[order[:500]], vec[order[:500]] + F32(3)), rr.remove(labels[order[100:300]]),
                                   rr.put(labels[order[::-1]], vec[order[::-1]])] + tail)
    (want, _) = rr.run_twin(twin, tmp_path, [a, b])
    rr.assert_same(rr.run_store(pyqadc, a), want, "one put")
    rr.assert_same(rr.run_store(pyqadc, b), want, "puts, removes and overwrites")
    assert int(want[0]["lims"][-1]) > 100 and want[1]["missing"] == 0


@path_independent
@pytest.mark.parametrize("form", ["range", "rerank_range"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_put_overwrite_and_remove_leave_the_held_result_as_it_is(pyqadc, dtype, form):
    """a result is held; then a put that grows the store (the rows relocate, the table is rebuilt), an overwrite of kept keys, a
    remove of kept keys, and knn, rerank and get; the collects after them, into host and into device memory, equal the first bit
    for bit — and the next range call sees the store as it now is"""
    import torch
    rng = np.random.default_rng(50 + rr.DTYPES[dtype])
    dim, n0, n1 = 24, 300, 6000
    labels = rng.choice(2 ** 32 - 1, n0 + n1, replace=False).astype(np.uint32)
    vec = rng.normal(size=(n0 + n1, dim)).astype(F32)
    q = rng.normal(size=(4, dim)).astype(F32)
    c = rr.case(True, dim, dtype, [], *(rr.sq_params(np.concatenate([vec, vec + F32(2)])) if dtype == "sq8" else (None, None)))
    st = rr.make_store(pyqadc, c)
    st.put(vec[:n0], labels[:n0])
    radius = np.array([np.inf, 40.0, 48.0, 0.0], F32)
    if form == "range":
        lims, keys, dist = st.range(q, radius)
    else:
        segs = [labels[:n0], labels[100:250], np.concatenate([labels[:50], labels[:50], [9]]), labels[:5]]
        in_lims = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
        lims, keys, dist, missing = st.rerank_range(q, in_lims, np.concatenate(segs).astype(np.uint32), radius)
        assert missing >= 1
    n = int(lims[-1])
    assert n >= n0 and lims[4] == lims[3]
    before, slots = st.relocations(), st.keyed_info()["table_slots"]
    st.put(vec[n0:], labels[n0:])                                          # grows: the rows move and the table is rebuilt
    assert st.relocations() > before and st.keyed_info()["table_slots"] > slots
    st.put(vec[:100] + F32(2), labels[:100])                               # overwrites rows of kept keys
    assert st.remove(keys[:n0 // 2]) > 0                                    # removes kept keys
    st.put_device(torch.from_numpy(vec[n0:n0 + 7] - F32(1)).cuda(), torch.from_numpy(labels[n0:n0 + 7].view(np.int32)).cuda())
    st.remove_device(torch.from_numpy(labels[200:220].view(np.int32)).cuda())
    st.knn(q, 10)
    st.rerank(q, np.tile(labels[:20], (4, 1)), 5)
    st.get(labels[:4])
    for _ in range(2):
        k2, d2 = st.range_collect(lims)
        assert np.array_equal(k2, keys) and np.array_equal(d2.view(np.uint32), dist.view(np.uint32))
    dk, dd = st._range_collect_device(lims)
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), keys) and np.array_equal(dd.cpu().numpy().view(np.uint32), dist.view(np.uint32))
    assert st.range_collect_raw(n - 1)[0] == pyqadc.QADC_E_CAPACITY and st.range_collect_raw(n)[0] == 0
    l2, k2, d2 = st.range(q[:1], np.inf)                                    # the next call drops it and sees the store as it is
    assert int(l2[-1]) == st.info()["rows"] and not np.isin(keys[:n0 // 2], k2).any()
    st.close()
