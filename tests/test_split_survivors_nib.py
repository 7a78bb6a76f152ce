"""tools/split_survivors.py, the nibble columns: choose_nib is the rule as stated (checked against a
second, sort-based statement of it and on crafted tables), its c is the deferred rows' true minimum sum, the survivor test with
that slack drops no candidate on 10^6 random codes, and the predicted survivor rate matches a direct count within binomial error
(3 sigma of the count) at the bounds of three level starts per query, for 10, 9 and 8 streamed sub-quantizers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import split_survivors as ss  # noqa: E402

M = ss.M


def rule_by_sorting(qt, ns):
    """The same rule, stated once: order the rows by (score, -s) and defer the first 16 - ns."""
    t = qt.reshape(M, 16).astype(np.int64)
    order = sorted(range(M), key=lambda s: (int(t[s].sum()) - 16 * int(t[s].min()), -s))
    deferred = order[:M - ns]
    return sum(1 << s for s in deferred), min(127, sum(int(t[s].min()) for s in deferred))


@pytest.mark.parametrize("ns", [8, 9, 10])
def test_choose_nib_is_the_rule(ns):
    rng = np.random.default_rng(ns)
    for trial in range(200):
        hi = int(rng.integers(2, 128))
        qt = rng.integers(0, hi, (M, 16)).astype(np.int8)
        if trial % 3 == 0:
            qt[rng.integers(0, M, 5)] = qt[0]                            # equal rows: ties
        mask, c = ss.choose_nib(qt, ns)
        assert (mask, c) == rule_by_sorting(qt, ns)
        assert bin(mask).count("1") == M - ns and 0 <= c <= 127
        assert sorted(ss.nib_streamed(mask) + [s for s in range(M) if mask >> s & 1]) == list(range(M))


def test_choose_nib_nested_ties_and_clamp():
    qt = np.zeros((M, 16), np.int8)                                      # all rows equal: ties go to the highest s
    assert ss.choose_nib(qt, 10) == (0xfc00, 0) and ss.choose_nib(qt, 9) == (0xfe00, 0) and ss.choose_nib(qt, 8) == (0xff00, 0)
    qt[:] = 40                                                           # constant rows of 40: c clamps at 127
    assert ss.choose_nib(qt, 10) == (0xfc00, 127)
    rng = np.random.default_rng(3)
    qt = rng.integers(0, 100, (M, 16)).astype(np.int8)
    m10, m9, m8 = (ss.choose_nib(qt, ns)[0] for ns in (10, 9, 8))
    assert m10 & m9 == m10 and m9 & m8 == m9                             # one pick after the other: the sets are nested
    qt[(1, 4, 7, 8, 12, 15), :] = 5                                      # six flat rows (score 0) among spread ones
    assert ss.choose_nib(qt, 10) == (sum(1 << s for s in (1, 4, 7, 8, 12, 15)), 30)


@pytest.mark.parametrize("ns", [10, 9, 8])
def test_the_slack_loses_no_candidate_and_the_predicted_rate_matches_a_direct_count(ns):
    n, nq = 1_000_000, 4
    rng = np.random.default_rng(78)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    nibbles = np.empty((n, M), np.uint8)
    nibbles[:, 0::2] = codes & 15
    nibbles[:, 1::2] = codes >> 4
    tables = ss.headline_tables(nq, 99)
    for q in range(nq):
        s = ss.float_sums(tables[q], codes[:100_000])
        qt = ss.quantize(tables[q], np.partition(s, 9)[9])               # qmax: the 10th smallest of a 10 % sample
        t = qt.reshape(M, 16).astype(np.int64)
        mask, c = ss.choose_nib(qt, ns)
        subs = ss.nib_streamed(mask)
        assert len(subs) == ns
        assert c == min(127, sum(int(t[s].min()) for s in range(M) if s not in subs))
        partial = np.minimum(sum(t[s][nibbles[:, s]] for s in subs), 127)
        full = np.minimum(sum(t[s][nibbles[:, s]] for s in range(M)), 127)
        assert np.array_equal(full, np.minimum(sum(ss.pair_entries(qt)[b][codes[:, b]] for b in range(8)), 127))
        for n_before in (1 << 14, 1 << 17, 1 << 20):
            bound = ss.bound_at(qt, n_before)
            bsurv = max(bound - c, 0)
            assert not np.any((full < bound) & (partial >= bsurv)), (q, n_before)        # exact: candidates are survivors
            p = ss.survivor_rate_nib(qt, subs, bound, c)
            count = int(np.count_nonzero(partial < bsurv))
            sigma = np.sqrt(n * p * (1 - p))
            print("query %d ns %d mask %04x slack %d bound %d: predicted %.1f, counted %d, sigma %.1f" % (q, ns, mask, c, bound, n * p, count, sigma))
            assert abs(count - n * p) <= 3 * sigma, (q, n_before, count, n * p, sigma)
            assert p <= ss.survivor_rate_nib(qt, subs, bound)                             # never more survivors than without it
