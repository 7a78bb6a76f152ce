"""CPU: the host twin of k-means++ seeding (quick-adc_amd/host/kmeans_seed.hpp behind host/db_build.hpp's front; driver
tests/cpp/kmeans_seed_host.cpp) against the definition in include/qadc.h: the centres are the named rows, the picks are distinct, the
seed alone decides, a numpy restatement of the whole definition agrees on integer-valued data at the tree's edges, the fallback
picks, the rows that may never be drawn, and the D^2 law itself on eight points with hand-computed weights."""
import numpy as np
import pytest

import kmeans_seed_compose as ks


@pytest.fixture(scope="module")
def driver():
    return ks.build_driver()


def test_uniform_is_splitmix64():
    # splitmix64 from state 0 returns 0xE220A8397B1DCDAF first (the reference vector of the generator): seed 0, m = t = 0
    assert ks.uniform(0, 0, 0) == (0xE220A8397B1DCDAF >> 11) * 2.0 ** -53
    assert 0.0 <= min(ks.uniform(s, m, t) for s in (0, 2 ** 64 - 1) for m in (0, 31) for t in (0, 2 ** 32 - 1)) and \
        max(ks.uniform(s, m, t) for s in range(50) for m in range(4) for t in range(50)) < 1.0


@pytest.mark.parametrize("sq_count,dim", [(1, 8), (4, 20), (16, 16)])
def test_centres_are_the_named_rows_and_distinct(driver, tmp_path, sq_count, dim):
    v = ks.real_set(500, dim)
    centres, rows, fallbacks = ks.twin(driver, tmp_path, v, 16, sq_count, seed=3)
    ks.check_centres(v, centres, rows, sq_count)
    assert fallbacks == 0 and all(len(set(r)) == 16 for r in rows.tolist())


def test_the_seed_decides_and_nothing_else(driver, tmp_path):
    v = ks.real_set(300, 8)
    a, b, c = (ks.twin(driver, tmp_path, v, 8, 2, seed=s) for s in (11, 11, 12))
    ks.same(a, b)
    assert not np.array_equal(a[1], c[1])
    big = ks.twin(driver, tmp_path, v, 8, 2, seed=2 ** 64 - 1)
    ks.check_centres(v, big[0], big[1], 2)
    # sub-space m is seeded on its own columns alone: other columns may change
    w = v.copy()
    w[:, 4:] = ks.real_set(300, 4, 9)
    assert np.array_equal(ks.twin(driver, tmp_path, w, 8, 2, seed=11)[1][0], a[1][0])


@pytest.mark.parametrize("n", ks.EDGE_N)
def test_numpy_restatement_on_integer_data(driver, tmp_path, n):
    v = ks.integer_set(n, 8)
    k = min(n, 12)
    for sq_count in (1, 2):
        centres, rows, fallbacks = ks.twin(driver, tmp_path, v, k, sq_count, seed=n)
        want_rows, want_fallbacks = ks.restate(v, k, sq_count, n)
        assert np.array_equal(rows, want_rows) and fallbacks == want_fallbacks == 0
        ks.check_centres(v, centres, rows, sq_count)


def test_front_is_the_trainers(driver, tmp_path):
    # with coarse and rotation the twin seeds on pq_train_front's output: integers below 2^8, a permutation for the rotation and
    # integer coarse centroids keep every float of the front exact (every term of the expansion distances is below 2^21), so numpy
    # can restate it
    rng = np.random.default_rng(5)
    v = rng.integers(0, 256, (700, 8)).astype(np.float32)
    coarse = rng.integers(0, 256, (3, 8)).astype(np.float32)
    rot = np.eye(8, dtype=np.float32)[rng.permutation(8)]
    d = np.sort(((v[:, None, :].astype(np.float64) - coarse[None]) ** 2).sum(-1), axis=1)
    keep = d[:, 1] > d[:, 0]                                                                  # no tie: the nearest is unambiguous
    v = np.ascontiguousarray(v[keep])
    d = ((v[:, None, :].astype(np.float64) - coarse[None]) ** 2).sum(-1)
    x = np.ascontiguousarray((v - coarse[d.argmin(1)]) @ rot.T, np.float32)
    got = ks.twin(driver, tmp_path, v, 10, 2, seed=1, coarse=coarse, rotation=rot)
    ks.check_centres(x, got[0], got[1], 2)
    ks.same(got, ks.twin(driver, tmp_path, x, 10, 2, seed=1))
    assert not np.array_equal(got[1], ks.twin(driver, tmp_path, v, 10, 2, seed=1)[1])         # (the front matters)


def test_fewer_distinct_rows_than_k_fall_back_in_index_order(driver, tmp_path):
    distinct = ks.real_set(3, 4)
    v = distinct[np.random.default_rng(0).integers(0, 3, 30)]
    for seed in range(20):
        centres, rows, fallbacks = ks.twin(driver, tmp_path, v, 9, 1, seed=seed)
        r = rows[0].tolist()
        assert fallbacks == 9 - 3 and len(set(r)) == 9
        assert len({v[i].tobytes() for i in r[:3]}) == 3                                      # the D^2 picks found every distinct row
        assert r[3:] == sorted(set(range(30)) - set(r[:3]))[:6]                               # then ascending unpicked order
        ks.check_centres(v, centres, rows, 1)


def test_all_identical_rows(driver, tmp_path):
    v = np.tile(ks.real_set(1, 6), (50, 1))
    _, rows, fallbacks = ks.twin(driver, tmp_path, v, 10, 2, seed=4)
    for r in rows.tolist():
        assert r[1:] == sorted(set(range(50)) - {r[0]})[:9]
    assert fallbacks == 2 * 9


def test_nonfinite_rows_are_never_drawn_by_the_d2_rule(driver, tmp_path):
    v, bad = ks.nonfinite_set()
    hit_bad_first = 0
    for seed in range(60):
        _, rows, fallbacks = ks.twin(driver, tmp_path, v, 12, 1, seed=seed)
        r = rows[0].tolist()
        assert len(set(r)) == 12
        if bad[r[0]]:                                     # pick 0 is uniform; no distance to it is finite: one fallback, row 0
            hit_bad_first += 1
            assert fallbacks == 1 and r[1] == 0
        else:
            assert fallbacks == 0
        assert not bad[r[1:]].any()
    assert hit_bad_first >= 1                             # (the case is covered: 6 of 40 rows are bad)


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_k_equals_n(driver, tmp_path, n):
    v = ks.real_set(n, 4)
    centres, rows, fallbacks = ks.twin(driver, tmp_path, v, n, 2, seed=n)
    assert fallbacks == 0 and all(sorted(r) == list(range(n)) for r in rows.tolist())
    ks.check_centres(v, centres, rows, 2)


POINTS = np.array([0, 1, 3, 6, 10, 15, 21, 28], np.float32)     # w_j after a first pick f is (x_j - x_f)^2, an integer
LAW_SEEDS = 4000


def test_the_d2_law(driver, tmp_path):
    """Over LAW_SEEDS seeds: pick 0 is uniform (p = 1/8), and pick 1 given pick 0 = f has p_j = (x_j - x_f)^2 / sum.  Every
    frequency lies within 5 standard deviations sqrt(p (1 - p) / N) of p, with N the draws the frequency is taken over (the seeds,
    and for the conditional law the seeds whose pick 0 was f)."""
    rows = ks.twin_rows(driver, tmp_path, POINTS[:, None], 2, 1, 0, LAW_SEEDS)[:, 0, :].astype(np.int64)
    first = np.bincount(rows[:, 0], minlength=8) / LAW_SEEDS
    p = 1 / 8
    assert (np.abs(first - p) <= 5 * np.sqrt(p * (1 - p) / LAW_SEEDS)).all(), first
    for f in range(8):
        sel = rows[rows[:, 0] == f, 1]
        w = (POINTS.astype(np.float64) - float(POINTS[f])) ** 2
        pj = w / w.sum()
        freq = np.bincount(sel, minlength=8) / len(sel)
        assert freq[f] == 0                                # a picked row weighs nothing
        assert (np.abs(freq - pj) <= 5 * np.sqrt(pj * (1 - pj) / len(sel))).all(), (f, freq, pj)
