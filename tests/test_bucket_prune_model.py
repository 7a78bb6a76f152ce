"""CPU: tools/bucket_prune.py, the model of the bucket scan's group test ("pruned groups").  Its lane-group
fraction is exact for iid uniform codes (the fraction of the 2^20 keys pruned); here it is checked against a brute-force count:
sampled uniform codes, every table row looked up per code, the kernel's inequality evaluated per code's own key."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bucket_prune as bp  # noqa: E402
import bucket_survivors as bs  # noqa: E402

M = 16
N = 200_000        # sampled codes: a fraction p has sigma = sqrt(p (1 - p) / N) <= 0.5 / sqrt(N) = 0.00112, so 3 sigma <= 0.0034
THREE_SIGMA = 3 * 0.5 / np.sqrt(N)


def tables(seed):
    """Two int8 tables of different character: spread rows (a query far from most centroids), and rows with a low floor."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 40, (M, 16)).astype(np.int8)
    b = (rng.integers(0, 12, (M, 16)) + rng.integers(0, 6, (M, 1))).astype(np.int8)
    return [a, b]


def brute_force(qt, nsp, bound, codes, wide=True):
    """The fraction of sampled codes whose lane group is pruned, from the codes' own nibbles."""
    t = qt.astype(np.int64)
    nib = np.empty((len(codes), M), np.int64)
    nib[:, 0::2] = codes & 15
    nib[:, 1::2] = codes >> 4
    mask, c = (bs.choose_bktw if wide else bs.choose_bkt)(qt, nsp)
    paid = (bs.bktw_paid if wide else bs.bkt_paid)(mask)
    fuse = wide and nsp % 2 == 1
    free = range(4) if fuse or not wide else range(5)
    s0 = sum(t[s][nib[:, s]] for s in free)
    pmin = sum(int(t[s].min()) for s in paid) + (int(t[4].min()) if fuse else 0)
    return float(np.mean(s0 + pmin >= max(0, bound - c)))


@pytest.mark.parametrize("nsp", bs.NSPS_WIDE)
def test_group_fraction_matches_a_brute_force_count(nsp):
    """n = 200 000 codes per table: 3 sigma <= 0.0034 whatever the fraction."""
    codes = np.random.default_rng(7).integers(0, 256, (N, M // 2), dtype=np.uint8)
    seen = []
    for qt in tables(11):
        for bound in (60, 90, 127):
            want = brute_force(qt, nsp, bound, codes)
            got = bp.group_fraction(bp.kept_keys(bp.wide_terms(qt, nsp, bound)))
            assert abs(got - want) <= THREE_SIGMA, (bound, got, want)
            seen.append(got)
    assert min(seen) < 0.2 and max(seen) > 0.8, seen            # the bounds cover both ends


def test_narrow_group_fraction_matches_a_brute_force_count():
    codes = np.random.default_rng(8).integers(0, 256, (N, M // 2), dtype=np.uint8)
    for qt in tables(12):
        for nsp in bs.NSPS:
            want = brute_force(qt, nsp, 70, codes, wide=False)
            got = bp.group_fraction(bp.kept_keys(bp.narrow_terms(qt, nsp, 70)))
            assert abs(got - want) <= THREE_SIGMA, (nsp, got, want)


def test_wave_fraction_is_never_above_the_group_fraction():
    for qt in tables(13):
        for nsp in bs.NSPS_WIDE:
            for bound in (0, 40, 60, 80, 100, 127):
                keep = bp.kept_keys(bp.wide_terms(qt, nsp, bound))
                g = bp.group_fraction(keep)
                for cpk in (16, 100, 128, 256, 442, 5000):
                    w = bp.wave_fraction(keep, cpk)
                    assert 0.0 <= w <= g + 1e-12, (nsp, bound, cpk, w, g)
    keep = np.zeros(1 << 20, bool)
    assert bp.group_fraction(keep) == 1.0 and bp.wave_fraction(keep, 128) == 1.0      # bsurv = 0: everything
    assert bp.wave_fraction(~keep, 128) == 0.0


def test_wave_fraction_counts_windows_of_64_groups():
    """16 groups per key (256 codes): a window is 4 keys.  Keys 0-7 pruned, 8 kept, 9-15 pruned, then everything kept:
    windows 0 and 1 are skipped, window 2 holds key 8, window 3 (keys 12-15) is skipped."""
    keep = np.ones(1 << 20, bool)
    keep[:16] = False
    keep[8] = True
    nwaves = (1 << 20) * 16 // 64
    assert bp.wave_fraction(keep, 256) == pytest.approx(3 / nwaves)
    assert bp.octaves(int(1e9), 1 << 27) == [128.0, 256.0] and bp.octaves(int(1e9), 1 << 29)[0] == pytest.approx((1e9 - 2 ** 29) / 2 ** 20)


def test_terms_of_a_fused_and_an_unfused_table():
    qt = tables(14)[0]
    t = qt.astype(np.int64)
    for nsp in bs.NSPS_WIDE:
        s0, pmin, bsurv = bp.wide_terms(qt, nsp, 100)
        mask, c = bs.choose_bktw(qt, nsp)
        key = 0x5a3c7
        nibs = [(key >> (4 * s)) & 15 for s in range(5)]
        rows = 4 if nsp % 2 else 5
        assert s0[key] == sum(t[s][nibs[s]] for s in range(rows)) and bsurv == 100 - c
        assert pmin == sum(t[s].min() for s in bs.bktw_paid(mask)) + (t[4].min() if nsp % 2 else 0)
