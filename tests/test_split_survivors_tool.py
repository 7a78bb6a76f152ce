"""tools/split_survivors.py, the CPU model behind the split scan's thresholds: on 10^6 random codes
and 4 queries the predicted survivor rate of the 6 bytes the library's rule streams matches a direct count within binomial
error (3 sigma of the count), at the bounds of three level starts per query.  The full 8-byte sum is printed beside it and not
asserted: it is not the quantity the thresholds rest on, and each further 3-sigma comparison adds 0.27 % of false alarms (one
of the twelve printed here, query 1 at 2^14, sits 3.6 sigma out with these codes and inside 1.6 sigma with five other seeds)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import split_survivors as ss  # noqa: E402


def test_predicted_rate_of_the_chosen_planes_matches_a_direct_count():
    n, nq = 1_000_000, 4
    rng = np.random.default_rng(77)
    codes = rng.integers(0, 256, (n, ss.M // 2), dtype=np.uint8)
    tables = ss.headline_tables(nq, 99)
    for q in range(nq):
        s = ss.float_sums(tables[q], codes[:100_000])
        qt = ss.quantize(tables[q], np.partition(s, 9)[9])             # qmax: the 10th smallest of a 10 % sample
        assert 0 <= qt.min() and qt.max() <= 127
        j = ss.choose_plane(qt)
        planes = ss.streamed(j)
        assert len(planes) == 6 and j not in planes and 7 not in planes
        pe = ss.pair_entries(qt)
        partial = np.minimum(sum(pe[b][codes[:, b]] for b in planes), 127)
        full = np.minimum(sum(pe[b][codes[:, b]] for b in range(8)), 127)
        for n_before in (1 << 14, 1 << 17, 1 << 20):
            bound = ss.bound_at(qt, n_before)
            for sel, values in ((planes, partial), (range(8), full)):
                p = ss.survivor_rate(qt, sel, bound)
                count = int(np.count_nonzero(values < bound))
                sigma = np.sqrt(n * p * (1 - p))
                print("query %d deferred byte %d bound %d planes %s: predicted %.1f, counted %d, sigma %.1f"
                      % (q, j, bound, list(sel), n * p, count, sigma))
                if sel is planes:
                    assert abs(count - n * p) <= 3 * sigma, (q, n_before, list(sel), count, n * p, sigma)
