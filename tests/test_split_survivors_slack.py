"""tools/split_survivors.py, the 5-plane columns: on 10^6 random codes and 4 queries, the survivor test
with slack drops no candidate (every code whose full sum is below the bound has its 5-byte partial below bound - c), c is the
deferred pair tables' true minimum sum, and the predicted survivor rate matches a direct count within binomial error (3 sigma of
the count) at the bounds of three level starts per query."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import split_survivors as ss  # noqa: E402


def test_the_slack_loses_no_candidate_and_the_predicted_rate_matches_a_direct_count():
    n, nq = 1_000_000, 4
    rng = np.random.default_rng(78)
    codes = rng.integers(0, 256, (n, ss.M // 2), dtype=np.uint8)
    tables = ss.headline_tables(nq, 99)
    for q in range(nq):
        s = ss.float_sums(tables[q], codes[:100_000])
        qt = ss.quantize(tables[q], np.partition(s, 9)[9])             # qmax: the 10th smallest of a 10 % sample
        j1, j2, c = ss.choose_planes5(qt)
        assert 0 <= j1 < j2 <= 6
        pe = ss.pair_entries(qt)
        assert c == min(127, int(pe[j1].min() + pe[j2].min() + pe[7].min())) == ss.slack(qt, (j1, j2, 7))
        planes = [b for b in range(7) if b not in (j1, j2)]
        partial = np.minimum(sum(pe[b][codes[:, b]] for b in planes), 127)
        full = np.minimum(sum(pe[b][codes[:, b]] for b in range(8)), 127)
        for n_before in (1 << 14, 1 << 17, 1 << 20):
            bound = ss.bound_at(qt, n_before)
            bsurv = max(bound - c, 0)
            assert not np.any((full < bound) & (partial >= bsurv)), (q, n_before)        # exact: candidates are survivors
            p = ss.survivor_rate(qt, planes, bound, c)
            count = int(np.count_nonzero(partial < bsurv))
            sigma = np.sqrt(n * p * (1 - p))
            print("query %d deferred %d %d slack %d bound %d: predicted %.1f, counted %d, sigma %.1f" % (q, j1, j2, c, bound, n * p, count, sigma))
            assert abs(count - n * p) <= 3 * sigma, (q, n_before, count, n * p, sigma)
            assert p <= ss.survivor_rate(qt, planes, bound)                               # never more survivors than without it
