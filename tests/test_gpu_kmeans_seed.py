"""GPU: k-means++ seeding (qadc_kmeans_seed_host / _device) against its CPU twin (host/kmeans_seed.hpp
behind the trainers' front; tests/kmeans_seed_compose.py), bit for bit: centres, rows and fallbacks.

The shapes sit at the kernels' edges.  n runs across the tree's node sizes (64 rows a level-1 node and a wave's window, 4096 a
level-2 node and a workgroup, 64^3 + 1 the first set with a level-4 root); dsub runs from 1 (a sub-space closes at every column) over
5 (no multiple of the 32-column window, and windows that hold several sub-spaces) to 1024 (a chain that crosses 32 windows); dim 3
and 100 leave a partly filled last window.  The learning sets are clustered floats, so that the rounding of every distance and of every
tree sum takes part.  The k = 65536 case is launch-bound (2 x 65535 launches)."""
import json
import time

import numpy as np
import pytest

import kmeans_seed_compose as ks
from helpers import path_independent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def driver():
    return ks.build_driver()


def device(pyqadc, v, k, sq_count, seed, **kw):
    centres, rows, fallbacks = pyqadc.kmeans_seed(v, k, sq_count=sq_count, seed=seed, return_rows=True, **kw)
    if sq_count == 1:
        centres, rows = centres[None], rows[None]
    return centres, rows, fallbacks


def check(pyqadc, driver, tmp_path, v, k, sq_count, seed, **kw):
    got = device(pyqadc, v, k, sq_count, seed, **kw)
    want = ks.twin(driver, tmp_path, v, k, sq_count, seed, **kw)
    ks.same(got, want)
    return got


@path_independent
@pytest.mark.parametrize("sq_count", [1, 2])
@pytest.mark.parametrize("n", ks.EDGE_N)
def test_tree_edges(pyqadc, driver, tmp_path, n, sq_count):
    v = ks.real_set(n, 8)
    centres, rows, fallbacks = check(pyqadc, driver, tmp_path, v, min(n, 16), sq_count, seed=n)
    ks.check_centres(v, centres, rows, sq_count)
    assert fallbacks == 0


SHAPES = [(1, 3), (1, 100), (1, 128), (16, 16), (16, 128), (32, 128), (4, 20), (2, 128)]


@path_independent
@pytest.mark.parametrize("sq_count,dim", SHAPES, ids=["%dx%d" % (s, d // s) for s, d in SHAPES])
def test_shapes(pyqadc, driver, tmp_path, sq_count, dim):
    v = ks.real_set(4097 + 130, dim)                              # two workgroups, the second with three level-1 nodes
    centres, rows, fallbacks = check(pyqadc, driver, tmp_path, v, 9, sq_count, seed=dim)
    ks.check_centres(v, centres, rows, sq_count)
    assert fallbacks == 0


@path_independent
def test_dim_4096(pyqadc, driver, tmp_path):
    check(pyqadc, driver, tmp_path, ks.real_set(300, 4096), 6, 4, seed=1)


@path_independent
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5, 8])
def test_nonfinite_rows(pyqadc, driver, tmp_path, seed):
    v, bad = ks.nonfinite_set()
    _, rows, fallbacks = check(pyqadc, driver, tmp_path, v, 12, 1, seed=seed)
    assert not bad[rows[0][1:].astype(np.int64)].any() and fallbacks == int(bad[rows[0][0]])
    w, bad = ks.nonfinite_set(200, 8)                             # ... and with every bad value in its own sub-space of two columns
    check(pyqadc, driver, tmp_path, w, 12, 4, seed=seed)


@path_independent
def test_duplicates_identical_rows_and_k_equal_n(pyqadc, driver, tmp_path):
    distinct = ks.real_set(3, 4)
    v = distinct[np.random.default_rng(0).integers(0, 3, 130)]
    _, rows, fallbacks = check(pyqadc, driver, tmp_path, v, 9, 1, seed=2)
    assert fallbacks == 6 and rows[0][3:].tolist() == sorted(set(range(130)) - set(rows[0][:3].tolist()))[:6]
    same = np.tile(ks.real_set(1, 6), (4100, 1))                  # the fallback cursor crosses bitmap words; two workgroups
    _, rows, fallbacks = check(pyqadc, driver, tmp_path, same, 70, 2, seed=4)
    assert fallbacks == 2 * 69
    for n in (1, 2, 65, 300):
        _, rows, fallbacks = check(pyqadc, driver, tmp_path, ks.real_set(n, 4), n, 2, seed=n)
        assert fallbacks == 0 and all(sorted(r) == list(range(n)) for r in rows.tolist())


@path_independent
def test_the_seed_decides(pyqadc, driver, tmp_path):
    v = ks.real_set(5000, 16)
    a = check(pyqadc, driver, tmp_path, v, 8, 4, seed=2 ** 64 - 1)
    b = check(pyqadc, driver, tmp_path, v, 8, 4, seed=2 ** 63)
    assert not np.array_equal(a[1], b[1])
    ks.same(device(pyqadc, v, 8, 4, 2 ** 64 - 1), a)              # and nothing else: a second run


@path_independent
@pytest.mark.parametrize("front", ["coarse", "rotation", "both"])
def test_with_coarse_and_rotation(pyqadc, driver, tmp_path, front):
    rng = np.random.default_rng(3)
    v = ks.real_set(4200, 16)
    coarse = v[rng.choice(len(v), 5, replace=False)] + np.float32(0.25) if front != "rotation" else None
    rot = np.linalg.qr(rng.normal(size=(16, 16)))[0].astype(np.float32) if front != "coarse" else None
    got = check(pyqadc, driver, tmp_path, v, 10, 4, seed=6, coarse=coarse, rotation=rot)
    assert not np.array_equal(got[1], device(pyqadc, v, 10, 4, 6)[1])


@path_independent
def test_device_form_leaves_the_tensor_alone(pyqadc, driver, tmp_path):
    torch = pytest.importorskip("torch")
    v = ks.real_set(4500, 20)
    t = torch.from_numpy(v).cuda()
    centres, rows, fallbacks = pyqadc.kmeans_seed_device(t, 7, sq_count=4, seed=9, return_rows=True)
    ks.same((centres, rows, fallbacks), ks.twin(driver, tmp_path, v, 7, 4, seed=9))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), v.view(np.uint32))
    one = pyqadc.kmeans_seed_device(t, 7, seed=9)                 # sq_count 1: [k][dim], a seed for kmeans_iterations
    assert one.shape == (7, 20) and np.array_equal(one, pyqadc.kmeans_seed(v, 7, seed=9))
    with pytest.raises(pyqadc.QadcError, match="device memory"):
        pyqadc.kmeans_seed_device(t.cpu(), 7)
    with pytest.raises(TypeError):
        pyqadc.kmeans_seed_device(v, 7)


@path_independent
def test_k_65536(pyqadc):
    """S = 2, dim = 4, n = 65600: the twin's rows are recorded as a digest (kmeans_seed_compose.record_big: a minute of CPU)."""
    with open(ks.BIG_GOLDEN) as f:
        golden = json.load(f)
    assert {key: golden[key] for key in ks.BIG} == ks.BIG
    v = ks.big_set()
    start = time.perf_counter()
    centres, rows, fallbacks = device(pyqadc, v, ks.BIG["k"], ks.BIG["sq_count"], ks.BIG["seed"])
    print("kmeans_seed k = 65536, S = 2, n = 65600: %.2f s" % (time.perf_counter() - start))
    assert rows[:, :8].tolist() == golden["first_rows"] and rows[:, -8:].tolist() == golden["last_rows"]
    assert ks.rows_digest(rows) == golden["rows_sha256"] and fallbacks == golden["fallbacks"]
    ks.check_centres(v, centres, rows, 2)
    assert all(len(set(r)) == ks.BIG["k"] for r in rows.tolist())
