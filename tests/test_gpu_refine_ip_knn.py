"""GPU: maximum-inner-product search over a whole refine store (pyqadc.Refine(metric="ip").knn and .knn_device over qadc_refine_knn*;
DESIGN.md section 11.23) against the host twin (refine::knn of quick-adc_amd/host/refine.hpp with metric kIP through
tests/cpp/refine_ip_host.cpp): keys, the scores' bit patterns and sizes, for equality.  The shapes sit on the edges of the plan
(host/refine_knn_plan.hpp) — the register tiles of 32 and of 4 queries, the LDS tile at dim 4096, chunks, groups and launches under
plan=(64, 0) — and on the edges of the order: a bound that moves every chunk or never, a bound that crosses the sign change of the
image between two selects, and a tie spread over chunks, groups and launches."""
import numpy as np
import pytest

import refine_ip_cases as ic
from helpers import path_independent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return ic.build_driver()


def check(pyqadc, twin, tmp_path, c, what="", **how):
    (want,) = ic.run_twin(twin, tmp_path, [c])
    ic.assert_same(ic.run_store(pyqadc, c, **how), want, what + " host form")
    ic.assert_same(ic.run_store(pyqadc, c, device=True, **how), want, what + " device form")
    return want


TILES = [(dim, dtype, False) for dim in (1, 63, 64, 65, 128, 4096) for dtype in ("f32", "f16", "sq8")] + \
    [(65, dtype, True) for dtype in ("f32", "f16", "sq8")]          # (a keyed store walks its rows through row_key: one dim is enough)


@path_independent
@pytest.mark.parametrize("dim,dtype,keyed", TILES, ids=["%d-%s-%s" % (d, t, "keyed" if k else "dense") for d, t, k in TILES])
def test_dims_tiles_and_R(pyqadc, twin, tmp_path, dim, dtype, keyed):
    """nq at the edges of the plan's tile — 32 queries in registers up to dim 128 (4 for calls of at most 4 queries), an LDS tile at
    dim 4096 — and R against the rows held"""
    rng = np.random.default_rng(dim + ic.DTYPES[dtype] + 9 * keyed)
    rows = 300
    nqs = (1, 3, 4, 5, 31, 32, 33, 65) if dim < 4096 else (1, 3, 4, 5, 33)
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    q = rng.normal(size=(max(nqs), dim)).astype(np.float32)
    labels = (rng.permutation(4 * rows)[:rows] + 7).astype(np.uint32) if keyed else None
    ops = [ic.knn("ip", q[:n], R) for n in nqs for R in ((1, rows - 1, rows, rows + 5) if n in (1, 5, 33) else (rows - 1,))]
    ops.append(ic.knn("ip", q[:5], ic.MAX_R))
    want = check(pyqadc, twin, tmp_path, ic.case(dim, dtype, vec, ops, lo=7, labels=labels))
    assert want[2]["sizes"].tolist() == [rows] and want[3]["sizes"].tolist() == [rows]
    assert (want[3]["keys"][0, rows:] == ic.NO_KEY).all() and (want[3]["dist"][0, rows:].view(np.uint32) == ic.NEG_INF_BITS).all()
    assert (np.diff(want[2]["dist"][0]) <= 0).all() and want[2]["dist"][0, 0] > 0 > want[2]["dist"][0, -1]


@path_independent
@pytest.mark.parametrize("order", ["best-to-worst", "worst-to-best"])
def test_rows_ordered_by_score(pyqadc, twin, tmp_path, order):
    """worst to best every chunk beats the bound its group has so far; best to worst none does after the first.  The scores run
    from -100 to 20, so under chunks of 64 rows the bound crosses the sign change of the image between two selects."""
    rng = np.random.default_rng(3)
    dim, rows = 4, 3000
    q = rng.normal(size=(3, dim)).astype(np.float32)
    q[1:] = q[0] * np.array([[0.5], [2.0]], np.float32)                        # the same order for every query
    unit = q[0].astype(np.float64) / np.dot(q[0].astype(np.float64), q[0].astype(np.float64))
    score = np.sort(rng.random(rows) * 120 - 100)
    if order == "best-to-worst":
        score = score[::-1]
    noise = rng.normal(size=(rows, dim)) * 0.01
    noise -= np.outer(noise @ q[0].astype(np.float64), unit)                    # orthogonal to the query
    vec = (np.outer(score, unit) + noise).astype(np.float32)
    c = ic.case(dim, "f32", vec, [ic.knn("ip", q, 100), ic.knn("ip", q, 1), ic.knn("ip", q, ic.MAX_R)])
    want = check(pyqadc, twin, tmp_path, c, "the default plan")
    ic.assert_same(ic.run_store(pyqadc, c, plan=(64, 0)), want, "chunks of 64 rows")
    best = want[0]["keys"][0]
    assert (best >= rows - 150).all() if order == "worst-to-best" else (best < 150).all()
    assert want[2]["dist"][0, 0] > 10 and want[2]["dist"][0, -1] < -10       # R = 1024 reaches across zero


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_scores_that_straddle_zero_with_zeros_among_them(pyqadc, twin, tmp_path, dtype):
    """integer scores -40 .. 40 in a shuffled store, many rows at exactly +0: with chunks of 64 rows the bound of a group moves from a
    negative score's image over 0x7FFFFFFF (+0) to a positive score's, and R cuts inside the run of zeros"""
    rng = np.random.default_rng(5)
    dim, rows = 2, 1200
    vec = np.zeros((rows, dim), np.float32)
    vec[:, 0] = rng.integers(-40, 41, rows)
    vec[rng.random(rows) < 0.2, 0] = 0
    vec[:, 1] = rng.integers(-3, 4, rows)                                     # (the query's second component is 0: products of +-0)
    q = np.array([[1, 0], [-1, 0], [0.5, -0.0]], np.float32)
    pos, zero = int((vec[:, 0] > 0).sum()), int((vec[:, 0] == 0).sum())
    ops = [ic.knn("ip", q, R) for R in (pos - 1, pos, pos + 1, pos + zero // 2, pos + zero, pos + zero + 1, 1024)]
    c = ic.case(dim, dtype, vec, ops, vmin=np.full(dim, -128, np.float32), step=np.ones(dim, np.float32))
    want = check(pyqadc, twin, tmp_path, c, "chunks of 64 rows", plan=(64, 0))
    ic.assert_same(ic.run_store(pyqadc, c), want, "the default plan")
    cut = want[3]                                                              # R ends inside the zeros: +0 bits, keys ascending
    assert (cut["dist"][0, pos:].view(np.uint32) == 0).all() and (np.diff(cut["keys"][0, pos:].astype(np.int64)) > 0).all()
    assert want[5]["dist"][0, -1] == -1 and want[1]["dist"][0, -1] == 1
    for res in want:
        assert not (res["dist"].view(np.uint32) == 0x80000000).any()


@path_independent
def test_a_tie_across_chunks_groups_and_launches(pyqadc, twin, tmp_path):
    """ten identical rows, the best of query 0, spread over the store so that, in chunks of 64 rows, they lie in different chunks,
    groups and launches"""
    rng = np.random.default_rng(22)
    dim, rows = 96, 1500
    vec = (rng.normal(size=(rows, dim)) * 0.1).astype(np.float32)
    same = np.array([0, 63, 64, 65, 127, 511, 512, 1023, 1024, 1499])
    vec[same] = np.float32(2.0)
    q = np.stack([vec[0], -vec[0]])                                            # the tie is first for query 0 and last for query 1
    c = ic.case(dim, "f32", vec, [ic.knn("ip", q, R) for R in (1, 5, 9, 10, 11)] + [ic.knn("ip", q[1:], 1024)], lo=100)
    want = check(pyqadc, twin, tmp_path, c, "chunks of 64 rows", plan=(64, 0))
    assert want[3]["keys"][0].tolist() == (same + 100).tolist() and len(set(want[3]["dist"][0].view(np.uint32).tolist())) == 1
    assert want[1]["keys"][0].tolist() == (same[:5] + 100).tolist()
    assert not np.isin(want[5]["keys"][0], same + 100).any()
    ic.assert_same(ic.run_store(pyqadc, c), want, "the default plan")


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_allow_and_exclude_filters(pyqadc, twin, tmp_path, keyed):
    rng = np.random.default_rng(23)
    dim, rows, lo = 65, 700, 30
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    q = rng.normal(size=(5, dim)).astype(np.float32)
    labels = (rng.permutation(3 * rows)[:rows] + lo).astype(np.uint32) if keyed else None
    keys = labels if keyed else np.arange(lo, lo + rows, dtype=np.uint32)
    some = rng.choice(keys, rows // 3, replace=False)
    across = np.concatenate([np.arange(0, lo + 9), some[:50], [int(keys.max()) + 5]])
    ops = []
    for mode in ("exclude", "allow"):
        ops += [ic.knn("ip", q, R, (mode, s)) for R in (10, rows) for s in (some, across, np.zeros(0, np.uint32), keys)]
    c = ic.case(dim, "f16", vec, ops, lo=lo, labels=labels)
    want = check(pyqadc, twin, tmp_path, c, "the default plan")
    ic.assert_same(ic.run_store(pyqadc, c, plan=(64, 0)), want, "chunks of 64 rows")
    assert want[3]["sizes"].max() == 0 and (want[3]["dist"].view(np.uint32) == ic.NEG_INF_BITS).all()      # everything excluded
    assert not np.isin(want[4]["keys"], some).any() and want[4]["sizes"].tolist() == [rows - len(some)] * 5
    assert np.isin(want[8]["keys"], some).all() and want[10]["sizes"].max() == 0                           # an empty ALLOW set


@path_independent
def test_knn_is_rerank_of_every_key_on_the_gpu(pyqadc):
    rng = np.random.default_rng(24)
    dim, rows, lo, nq = 128, 4000, 1000, 5
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[100:110] = vec[5]
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    for dtype in ("f32", "f16", "sq8"):
        st = pyqadc.Refine.from_vectors(vec, dtype, first_key=lo, metric="ip")
        assert st.metric == "ip"
        keys = np.tile(np.arange(lo, lo + rows, dtype=np.uint32), (nq, 1))
        for R in (1, 100, 1024):
            k, d, s, missing = st.rerank(q, keys, R)
            gk, gd, gs = st.knn(q, R)
            assert missing == 0 and ic.same(dict(keys=gk, dist=gd, sizes=gs, missing=0), dict(keys=k, dist=d, sizes=s, missing=0)) is None, (dtype, R)
        st.close()
