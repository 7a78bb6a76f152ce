"""GPU: no plan shows in a result of the probed exact search (qadc_refine_knn_probed).  qadc_refine_set_knn_plan
cuts the rows a (query, group) buffer is offered between two selects down to 64 and to 1 and the queries of a pass down to 1 and 3;
every result equals the host twin's, which knows no chunk, group, launch or pass.  Ties spread over partitions, chunks, groups and
launches are cut by key, and rows ordered by distance inside a partition drive the bound both ways."""
import numpy as np
import pytest

import refine_probe_cases as pc
from helpers import path_independent

pytestmark = pytest.mark.gpu
K = len(pc.SIZES)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return pc.build_driver()


@path_independent
@pytest.mark.parametrize("plan", [(64, 0), (1, 0), (0, 1), (0, 3), (64, 3)], ids=["chunk64", "chunk1", "pass1", "pass3", "chunk64-pass3"])
def test_a_plan_gives_the_default_plans_bits(pyqadc, twin, tmp_path, plan):
    rng = np.random.default_rng(5)
    dim = 65
    q = rng.normal(size=(7, dim)).astype(np.float32)

    def calls(vec, labels):
        # (chunk_rows 1 takes a group per probe: ma <= 8 and R <= 1024 give it)
        return [pc.call(q, pc.probes(rng, 7, ma, K), R) for ma in (1, 2, K) for R in (1, 50, 1024)]
    c = pc.dense_case(rng, dim, "f32", calls)
    (want,) = pc.run_twin(twin, tmp_path, [c])
    pc.assert_same(pc.run_gpu(pyqadc, c), want, "the default plan")
    pc.assert_same(pc.run_gpu(pyqadc, c, plan=plan), want, "plan %s" % (plan,))
    pc.assert_same(pc.run_gpu(pyqadc, c, plan=plan, device=True), want, "plan %s, device form" % (plan,))


@path_independent
def test_a_chunk_below_the_probes_of_a_group_is_refused(pyqadc):
    rng = np.random.default_rng(1)
    sizes = (3,) * 9
    c = pc.dense_case(rng, 4, "f32", lambda vec, labels: [pc.call(vec[:1], [list(range(9))], 5)], sizes=sizes)
    with pytest.raises(pyqadc.QadcError):
        pc.run_gpu(pyqadc, c, plan=(1, 0))                                   # nine probes in eight groups
    pc.run_gpu(pyqadc, c, plan=(2, 0))


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ten_identical_rows_spread_over_the_walk_are_cut_by_key(pyqadc, twin, tmp_path, dtype):
    """ten copies of the query under ten keys: in partitions 2, 3 and 4, inside one chunk of 64, in different chunks (launches) of
    partition 4, and through probes that land in different groups; R = 5 cuts the tie, R = 10 ends with it, R = 11 goes one past"""
    rng = np.random.default_rng(8)
    dim, n = 96, sum(pc.SIZES)
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    labels = np.arange(1000, 1000 + n, dtype=np.uint32)
    at = np.array([1 + 5, 1 + 40, 64 + 3, 64 + 70, 64 + 299, 364 + 0, 364 + 10, 364 + 63, 364 + 64, 364 + 699])   # rows of the index
    vec[at] = vec[at[0]]
    q = rng.normal(size=(3, dim)).astype(np.float32)
    q[0] = vec[at[0]]
    if dtype == "f16":
        q[0] = vec[at[0]].astype(np.float16).astype(np.float32)
    calls = [pc.call(q, a, R) for a in ([[2, 3, 4]] * 3, [[4, 2, 3]] * 3, np.tile(np.arange(K, dtype=np.int32)[::-1], (3, 1))) for R in (5, 10, 11)]
    c = pc.case(False, dim, dtype, [pc.add(1000, vec)], pc.split_labels(labels), calls)
    (want,) = pc.run_twin(twin, tmp_path, [c])
    ties = np.sort(labels[at])
    assert want[0]["keys"][0].tolist() == ties[:5].tolist() and want[1]["keys"][0].tolist() == ties.tolist()
    assert (want[1]["dist"][0].view(np.uint32) == 0).all() and want[2]["dist"][0, 10] > 0
    for plan in (None, (64, 0), (7, 1)):
        pc.assert_same(pc.run_gpu(pyqadc, c, plan=plan), want, "plan %s" % (plan,))


@path_independent
@pytest.mark.parametrize("order", ["far-to-near", "near-to-far"])
def test_rows_ordered_by_distance_inside_a_partition(pyqadc, twin, tmp_path, order):
    """far to near every chunk beats the bound its buffer has so far; near to far none does after the first"""
    rng = np.random.default_rng(3)
    dim, sizes = 4, (0, 1, 63, 300, 9000)
    n = sum(sizes)
    radius = rng.random(n).astype(np.float32) * 100 + 1
    radius[364:] = np.sort(radius[364:])[::-1] if order == "far-to-near" else np.sort(radius[364:])
    unit = rng.normal(size=(n, dim))
    vec = (unit / np.linalg.norm(unit, axis=1, keepdims=True) * radius[:, None]).astype(np.float32)
    q = (rng.normal(size=(3, dim)) * 0.01).astype(np.float32)
    labels = np.arange(n, dtype=np.uint32)
    calls = [pc.call(q, [[4, 3]] * 3, 100), pc.call(q, [[4, 3]] * 3, 1), pc.call(q, np.tile(np.arange(K, dtype=np.int32), (3, 1)), 100)]
    c = pc.case(False, dim, "f32", [pc.add(0, vec)], pc.split_labels(labels, sizes), calls)
    (want,) = pc.run_twin(twin, tmp_path, [c])
    for plan in (None, (64, 0), (1000, 2)):
        pc.assert_same(pc.run_gpu(pyqadc, c, plan=plan), want, "plan %s" % (plan,))
