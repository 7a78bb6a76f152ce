"""CPU: the inputs of tests/test_gpu_shard_forms.py and of the multi-process case "flat_forms" (tests/dist_cases.py), under the
oracle alone: every query's heap is full (rc == 0), the planted codes are in query 0's heap with the stated counts (otherwise the
shard edges they sit on would be checked by nothing), and a shard's push stream is some hundreds of entries, orders of magnitude
below the 2^18 entries the ranks' streams are collected into."""
import numpy as np

from dist_cases import SHARD_FORMS_N, TILE, build_case, shard_forms_cuts
from test_gpu_shard_forms import CAPACITY, IVF_ASSIGN, IVF_SIZES, KEEPS, M, R, flat_inputs, ivf_inputs


def test_flat_list_plants_and_stream_sizes(po):
    codes, tables, cuts, wants, refs = flat_inputs(po)
    n = len(codes)
    assert n == SHARD_FORMS_N == 12 * TILE + 37 == 196645 and len(np.unique(codes[:, :2], axis=0)) <= 1024 + 1
    assert sorted(cuts) == ["first-pos-2-mod-16", "four-ranks", "shard-ranges-2", "three-ranks", "tile-aligned"]
    for keep in KEEPS:
        want = wants[keep]
        assert [w["rc"] for w in want] == [0, 0, 0] and [len(w["keys"]) for w in want] == [R] * 3
        keys0 = want[0]["keys"]
        assert np.count_nonzero(keys0 == n - 1) == 1 + (16 - n % 16) % 16 == 12
        for name, cut in cuts.items():
            first1 = cut[1][0]
            assert np.count_nonzero(keys0 == first1 - 1) == 1 and np.count_nonzero(keys0 == first1) == 1, name
            # the planted codes share the smallest value of the heap: which of them stay, and where, is a matter of push order
            assert want[0]["values"][keys0 == first1].tolist() == [want[0]["values"].min()], name
            for first, ln in cut:
                if ln and first % 16 == 0 and (ln % 16 == 0 or first + ln == n):      # (po.shard_stream walks blocks of 16 from first)
                    for q in range(3):
                        k, _ = po.shard_stream(M, codes[first:first + ln], None, n, first, want[q]["qtables"][0], R)
                        assert len(k) * 64 < CAPACITY, (name, first, q, len(k))
        for q in range(3) if refs else ():
            assert np.array_equal(refs[keep][q][0], want[q]["keys"]) and np.array_equal(refs[keep][q][1], want[q]["values"]), q


def test_flat_forms_case_is_that_list(po):
    case = build_case("flat_forms")
    codes, tables = flat_inputs(po)[:2]
    assert np.array_equal(case["parts"][0], codes) and np.array_equal(case["tables"][:3], tables)
    assert case["tables"].shape == (32, 1, 256) and case["assign"].shape == (32, 1) and case["keep"] == 0.05 and case["slots"] == (0, 1)
    for q in range(32):
        assert po.query_scan(M, case["parts"], None, case["keep"], [0], case["tables"][q].copy(), case["R"])["rc"] == 0, q


def test_ivf_inputs(po):
    parts, labels, tables, want = ivf_inputs(po)
    assert [len(p) for p in parts] == IVF_SIZES == [8 * TILE + 53, 37, 16, 6 * TILE + 9, 0]
    assert [w["rc"] for w in want] == [0] * len(IVF_ASSIGN)
    assert np.count_nonzero(want[0]["keys"] == labels[0][-1]) >= 1 + (16 - IVF_SIZES[0] % 16) % 16 == 12
    assert np.count_nonzero(want[0]["keys"] == labels[0][43695]) == 1 and np.count_nonzero(labels[0] == labels[0][43695]) == 1
