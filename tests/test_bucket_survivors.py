"""tools/bucket_survivors.py: choose_bkt is plane_choice_bkt's rule as stated (checked against a second,
sort-based statement of it and on crafted tables), its c is the deferred rows' true minimum sum, the survivor test with that slack
and the four free rows drops no candidate on random codes, and the nibble columns it prints are tools/split_survivors.py's own."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bucket_survivors as bs  # noqa: E402
import split_survivors as ss  # noqa: E402

M = ss.M


def rule_by_sorting(qt, nsp):
    """The rule, stated once: order rows 4..15 by (score, -s) and defer the first 12 - nsp."""
    t = qt.reshape(M, 16).astype(np.int64)
    order = sorted(range(4, M), key=lambda s: (int(t[s].sum()) - 16 * int(t[s].min()), -s))
    deferred = order[:12 - nsp]
    return sum(1 << s for s in deferred), min(127, sum(int(t[s].min()) for s in deferred))


@pytest.mark.parametrize("nsp", bs.NSPS)
def test_choose_bkt_is_the_rule(nsp):
    rng = np.random.default_rng(nsp)
    for trial in range(200):
        qt = rng.integers(0, int(rng.integers(2, 128)), (M, 16)).astype(np.int8)
        if trial % 3 == 0:
            qt[rng.integers(0, M, 5)] = qt[0]                            # equal rows: ties
        mask, c = bs.choose_bkt(qt, nsp)
        assert (mask, c) == rule_by_sorting(qt, nsp)
        assert mask & 0xf == 0 and bin(mask).count("1") == 12 - nsp and 0 <= c <= 127
        assert sorted(list(bs.FREE) + bs.bkt_paid(mask) + [s for s in range(M) if mask >> s & 1]) == list(range(M))


def test_choose_bkt_nested_ties_and_clamp():
    qt = np.zeros((M, 16), np.int8)                                      # all rows equal: ties go to the highest s
    assert [bs.choose_bkt(qt, p) for p in bs.NSPS] == [(0xff00, 0), (0xfe00, 0), (0xfc00, 0), (0xf800, 0)]
    qt[:] = 40
    assert bs.choose_bkt(qt, 7) == (0xf800, 127)
    qt = np.random.default_rng(3).integers(0, 100, (M, 16)).astype(np.int8)
    m = [bs.choose_bkt(qt, p)[0] for p in (7, 6, 5, 4)]
    assert all(a & b == a for a, b in zip(m, m[1:]))                     # one pick after the other: the sets are nested
    qt[(0, 1, 2, 3), :] = 5                                              # the free rows are never deferred, however flat
    assert bs.choose_bkt(qt, 4)[0] & 0xf == 0


@pytest.mark.parametrize("nsp", bs.NSPS)
def test_the_slack_loses_no_candidate(nsp):
    n, nq = 200_000, 3
    rng = np.random.default_rng(78)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    nibbles = np.empty((n, M), np.uint8)
    nibbles[:, 0::2] = codes & 15
    nibbles[:, 1::2] = codes >> 4
    tables = ss.headline_tables(nq, 99)
    for q in range(nq):
        s = ss.float_sums(tables[q], codes[:100_000])
        qt = ss.quantize(tables[q], np.partition(s, 9)[9])
        t = qt.reshape(M, 16).astype(np.int64)
        mask, c = bs.choose_bkt(qt, nsp)
        subs = list(bs.FREE) + bs.bkt_paid(mask)
        assert c == min(127, sum(int(t[s].min()) for s in range(M) if s not in subs))
        partial = np.minimum(sum(t[s][nibbles[:, s]] for s in subs), 127)
        full = np.minimum(sum(t[s][nibbles[:, s]] for s in range(M)), 127)
        for n_before in (1 << 14, 1 << 17, 1 << 20):
            bound = ss.bound_at(qt, n_before)
            assert not np.any((full < bound) & (partial >= max(bound - c, 0))), (q, n_before)


def test_the_nibble_columns_are_split_survivors_own():
    qts = bs.headline_qtables(10 ** 9, 4, 1234)
    for start in bs.LEVEL_STARTS:
        got = bs.nib_rates(qts, start)
        for ns in (10, 9, 8):
            want = []
            for qt in qts:
                mask, c = ss.choose_nib(qt, ns)
                want.append(ss.survivor_rate_nib(qt, ss.nib_streamed(mask), ss.bound_at(qt, start), c))
            assert got[ns] == float(np.mean(want))
