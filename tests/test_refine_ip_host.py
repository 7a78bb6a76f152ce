"""CPU: the host twin of the inner-product metric (refine::rerank, ::knn and ::knn_probed of quick-adc_amd/host/refine.hpp with metric
kIP, driver tests/cpp/refine_ip_host.cpp) — the written definition of a store under QADC_REFINE_IP, to which
the GPU is held bit for bit.

The twin is compared, bit for bit, with an independent numpy restatement (tests/refine_ip_cases.py: strips of 64, the tree, the
image, a sort of words), and with itself across the three functions: knn equals rerank fed every held key, and knn_probed at ma = K
with the keys as labels equals knn.  A cross-check that trusts neither restatement: on integer rows of one norm the key lists under
the two metrics are equal."""
import numpy as np
import pytest

import refine_ip_cases as ic


@pytest.fixture(scope="module")
def driver():
    return ic.build_driver()


def check(exe, tmp_path, cases, names=None):
    wants = ic.run_twin(exe, tmp_path, cases)
    for i, (c, got) in enumerate(zip(cases, wants)):
        ic.assert_same(got, ic.run_numpy(c), names[i] if names else "case %d" % i)
    return wants


def assert_three_agree(got, what=""):
    """operations in threes — rerank of every key, knn, knn_probed at ma = K: one result"""
    assert len(got) % 3 == 0
    for i in range(0, len(got), 3):
        for j in (1, 2):
            diff = ic.same(dict(got[i], missing=0), dict(got[i + j], missing=0))
            assert diff is None, "%s operations %d and %d: %s differs" % (what, i, i + j, diff)


@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_the_twin_equals_the_numpy_restatement(driver, tmp_path, dtype, keyed):
    rng = np.random.default_rng(11 + ic.DTYPES[dtype] + 7 * keyed)
    cases, names = [], []
    for dim in ic.DIMS:
        rows = 120 if dim < 4096 else 30
        cases += [ic.random_case(rng, dim, dtype, keyed, rows=rows), ic.random_case(rng, dim, dtype, keyed, rows=40, lo=2 ** 32 - 4 * 40 - 1, scale=100.0)]
        names += ["random dim %d" % dim, "high keys dim %d" % dim]
    wants = check(driver, tmp_path, cases, names)
    w = wants[0]
    assert w[0]["missing"] == 3 and w[1]["missing"] == 3                       # the three keys no store holds, under either metric
    for res in w[:len(w) // 2]:                                                # "ip": scores descend, fillers are -inf under key 0xFFFFFFFF
        for q in range(len(res["sizes"])):
            n = res["sizes"][q]
            assert (np.diff(res["dist"][q, :n]) <= 0).all()
            assert (res["keys"][q, n:] == ic.NO_KEY).all() and (res["dist"][q, n:].view(np.uint32) == ic.NEG_INF_BITS).all()


@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_scores_of_both_signs_and_where_R_cuts(driver, tmp_path, dtype, keyed):
    c = ic.sign_case(dtype, keyed)
    (want,) = check(driver, tmp_path, [c])
    assert_three_agree(want)
    by_R = {op[4]: res for op, res in zip(c["ops"][::3], want[::3])}
    full = by_R[9]
    assert full["keys"][0].tolist() == [10, 13, 15, 12, 16, 11, 17, 14, ic.NO_KEY]      # 3, 2, 1, +0 (key 12), +0 (key 16), -1, -2, -3
    assert full["dist"][0].view(np.uint32).tolist() == ic.bits(0x40400000, 0x40000000, 0x3F800000, 0, 0, 0xBF800000, 0xC0000000, 0xC0400000,
                                                               ic.NEG_INF_BITS).view(np.uint32).tolist()
    assert full["keys"][1].tolist() == [14, 17, 11, 12, 16, 15, 13, 10, ic.NO_KEY]      # the query negated and halved: 1.5, 1, .5, +0, +0, ...
    assert full["sizes"].tolist() == [8, 8]
    for R in (1, 2, 3, 4, 5, 6, 8):                                                      # a cut at a positive, a zero, a negative score
        assert by_R[R]["keys"][0].tolist() == full["keys"][0, :R].tolist()
        assert by_R[R]["dist"][0].view(np.uint32).tolist() == full["dist"][0, :R].view(np.uint32).tolist()


def test_no_score_is_minus_zero(driver, tmp_path):
    """a partial sum starts at +0 and an IEEE sum is -0 only where both operands are: products of -0, rows of -0 and sums that cancel
    all give +0, image 0x7FFFFFFF, and tie by key; the image of -0, 0x80000000, is never formed"""
    c = ic.zero_case()
    (want,) = check(driver, tmp_path, [c])
    assert_three_agree(want)
    for res in want:
        assert not (res["dist"].view(np.uint32) == 0x80000000).any()
    full = want[0]
    assert full["keys"][0].tolist() == [0, 1, 2, 3, 4, 5] and (full["dist"][0].view(np.uint32) == 0).all()      # q = +0: every score +0
    assert full["keys"][1].tolist() == [0, 1, 2, 3, 4, 5] and (full["dist"][1].view(np.uint32) == 0).all()      # q = -0
    assert full["keys"][2].tolist() == [0, 2, 3, 4, 5, 1] and full["dist"][2].tolist() == [0, 0, 0, 0, 0, -3]
    assert want[3]["keys"][2].tolist() == [0, 2, 3]                                                             # R = 3 cuts the tie at +0 by key


@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_non_finite_scores(driver, tmp_path, dtype):
    rng = np.random.default_rng(5)
    cases = [ic.nonfinite_case(rng, dim, dtype) for dim in ic.DIMS] + [ic.overflow_case()]
    wants = check(driver, tmp_path, cases)
    for w in wants:
        assert_three_agree(w)
    for w in wants[:-1]:
        full = w[0]
        assert (full["dist"][1].view(np.uint32)[:30] == ic.NAN_BITS).all() and full["keys"][1, :30].tolist() == list(range(30))   # a NaN query
        for q in range(5):                                                     # NaN behind everything else, -inf before it
            d = full["dist"][q, :30]
            nan = np.isnan(d)
            assert not nan[:30 - nan.sum()].any() and (d.view(np.uint32)[nan] == ic.NAN_BITS).all()
    if dtype == "f32":
        full = wants[2][0]                                                     # dim 64
        assert np.isposinf(full["dist"][0, 0]) and full["keys"][0, 0] in (4, 6)         # +inf first
        assert np.isnan(full["dist"][4, 29])                                            # 0 * inf
    over = wants[-1][0]
    assert over["keys"][0].tolist() == [0, 2, 3, 1, 4]                         # +inf (keys 0, 2), +0, -inf, NaN
    assert over["dist"][0].view(np.uint32).tolist() == [0x7F800000, 0x7F800000, 0, 0xFF800000, ic.NAN_BITS]


@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_ties_are_cut_by_key(driver, tmp_path, dtype, keyed):
    rng = np.random.default_rng(8)
    cases = [ic.tie_case(rng, dim, dtype, keyed) for dim in ic.DIMS]
    wants = check(driver, tmp_path, cases)
    for w in wants:
        assert_three_agree(w)
        assert w[0]["keys"][0, :11].tolist()[:10] == list(range(60, 70))
        assert len(set(w[0]["dist"][0, :10].view(np.uint32).tolist())) == 1
        assert w[3]["keys"][0].tolist() == [60, 61, 62, 63, 64]               # R = 5 cuts the tie, by key
        assert w[6]["keys"][0].tolist() == list(range(60, 70))
        assert w[9]["keys"][0, :10].tolist() == list(range(60, 70)) and w[9]["keys"][0, 10] not in range(60, 70)


def test_knn_is_rerank_of_every_key_and_probed_at_every_partition_is_knn(driver, tmp_path):
    rng = np.random.default_rng(9)
    for dtype in ("f32", "f16", "sq8"):
        for keyed in (False, True):
            c = ic.random_case(rng, 65, dtype, keyed, rows=150)
            (want,) = ic.run_twin(driver, tmp_path, [c])
            threes = [r for op, r in zip(c["ops"], want) if (op[0] == "rerank" and op[3].shape[1] == 150) or (op[0] != "rerank" and op[-1] is None)]
            assert len(threes) == 18
            assert_three_agree(threes, "%s keyed %d" % (dtype, keyed))


def test_on_rows_of_one_norm_the_keys_under_ip_are_the_keys_under_l2(driver, tmp_path):
    rng = np.random.default_rng(10)
    c = ic.norm_case(rng)
    (want,) = check(driver, tmp_path, [c])
    half = len(want) // 2
    assert_three_agree(want)
    tied = 0
    for ip, l2 in zip(want[:half], want[half:]):
        assert np.array_equal(ip["keys"], l2["keys"]) and np.array_equal(ip["sizes"], l2["sizes"])
        q2 = (c["ops"][0][2].astype(np.float64) ** 2).sum(axis=1, keepdims=True)
        x2 = float((c["vectors"][0].astype(np.float64) ** 2).sum())
        n = ip["keys"].shape[1]
        if n <= 200:
            assert np.array_equal(l2["dist"].astype(np.float64), q2 + x2 - 2 * ip["dist"].astype(np.float64))   # exact integers
        tied += int((np.diff(ip["dist"], axis=1) == 0).sum())
    assert tied > 0


def test_the_image_and_its_inverse(driver, tmp_path):
    bits = ic.image_sweep()
    img, back = ic.twin_images(driver, tmp_path, bits)
    assert np.array_equal(img, ic.np_img_ip(bits.view(np.float32)))
    assert np.array_equal(back, ic.np_img_ip_inverse(img))
    nan = np.isnan(bits.view(np.float32))
    assert nan.sum() >= 8 and (img[nan] == ic.NAN_IMAGE_IP).all() and (back[nan] == ic.NAN_BITS).all()
    assert np.array_equal(back[~nan], bits[~nan])                                                       # the round trip
    at = {int(b): int(i) for b, i in zip(bits[:22].tolist(), img[:22].tolist())}
    assert at[0x7F800000] == 0x007FFFFF and at[0x00000000] == 0x7FFFFFFF and at[0x80000000] == 0x80000000 and at[0xFF800000] == 0xFF800000
    assert at[0x00000001] == 0x7FFFFFFE and at[0x80000001] == 0x80000001 and at[0x007FFFFF] == 0x7F800000 and at[0x00800000] == 0x7F7FFFFF
    # the order: larger scores have smaller images, -0 directly behind +0, every image below the high half of a skipped entry's word
    f = bits[~nan].view(np.float32).astype(np.float64)
    order = np.argsort(img[~nan], kind="stable")
    assert (np.diff(f[order]) <= 0).all() and (img < 0xFFFFFFFF).all()
