"""CPU: the numpy model of the bucket copy with wide octaves (tests/bktw_model.py), checked on copies the model builds itself and on
broken ones, and the wide columns of tools/bucket_survivors.py: choose_bktw is plane_choice_bktw's rule as stated (against a
sort-based statement of it), its c is the deferred rows' true minimum sum and loses no candidate, the survivor rate it prints
equals a brute-force count over every code of a small sample, and expected_padding equals a simulation."""
import os
import sys

import numpy as np
import pytest

import bkt_model
import bktw_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bucket_survivors as bs  # noqa: E402
import split_survivors as ss  # noqa: E402

M = ss.M
TILE = wm.TILE


def pooled_codes(rng, n, nkeys):
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    kk = rng.permutation(1 << 20)[:nkeys][rng.integers(0, nkeys, n)]
    codes[:, 0], codes[:, 1] = kk & 255, (kk >> 8) & 255
    codes[:, 2] = (codes[:, 2] & 0xf0) | (kk >> 16)
    return codes


def model_copies(codes, W, block, max_pad):
    wide = wm.wide_layout(codes, W, max_pad)
    narrow = wm.narrow_layout(codes, block, wide)
    wc = wm.model_copy(codes, wide, wm.planes_of, W) if any(l[4] for l in wide) else None
    nc = wm.model_copy(codes, narrow, bkt_model.planes_of, block) if any(l[4] for l in narrow) else None
    return wc, nc


def test_octaves_and_layouts():
    assert wm.octaves(12 * TILE + 37, TILE) == [(TILE, 2 * TILE), (2 * TILE, 4 * TILE), (4 * TILE, 8 * TILE), (8 * TILE, 12 * TILE + 37)]
    assert wm.octaves(TILE, TILE) == [] and wm.octaves(5, 0) == [] and wm.octaves(TILE + 1, TILE) == [(TILE, TILE + 1)]
    # the headline: 10^9 codes, W = 2^27
    assert wm.octaves(10 ** 9, 1 << 27) == [(1 << 27, 1 << 28), (1 << 28, 1 << 29), (1 << 29, 10 ** 9)]
    rng = np.random.default_rng(1)
    codes = pooled_codes(rng, 8 * TILE + 37, 12)
    wide = wm.wide_layout(codes, TILE, 2.01)
    # the clipped tail of 37 codes takes a whole tile: far beyond any cap, it keeps narrow blocks
    assert [l[4] > 0 for l in wide] == [True, True, True, False]
    narrow = wm.narrow_layout(codes, TILE, wide)
    assert [l[4] > 0 for l in narrow] == [True] + [False] * 7 + [True]
    assert wm.TILE_BYTES == 93184 and wm.ID_OFF % 8 == 0


def test_the_checks_pass_on_the_models_own_copy_and_fail_on_broken_ones():
    rng = np.random.default_rng(2)
    n, W = 8 * TILE + 37, TILE
    codes = pooled_codes(rng, n, 20)
    wc, nc = model_copies(codes, W, TILE, 2.01)
    wide, narrow = wm.check_copies(wc, nc, codes, W, TILE, 2.01)
    assert sum(l[4] for l in wide) == len(wc["perm"]) and sum(l[4] for l in narrow) == len(nc["perm"])

    def broken(mutate):
        w = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in wc.items()}
        mutate(w)
        with pytest.raises(AssertionError):
            wm.check_copies(w, nc, codes, W, TILE, 2.01)

    pad = int(np.nonzero(wc["perm"] == wm.PAD)[0][0])

    def pad_is_real(w):                                           # a padding slot that claims a position: the code would be emitted twice
        w["perm"][pad] = w["perm"][pad - 1]
    broken(pad_is_real)

    def wrong_id4(w):                                             # sub-quantizer 4 of a group taken from the high nibble of byte 2
        w["tiles"][:, wm.ID4_OFF:] = (w["codes"][0::16, 2] >> 4).reshape(-1, TILE // 16)
    broken(wrong_id4)

    def other_octave(w):                                          # two real slots of different octaves swapped
        a, b = int(w["off"][0]), int(w["off"][2])
        for k in ("codes", "perm"):
            w[k][[a, b]] = w[k][[b, a]]
        w["tiles"] = wm.planes_of(w["codes"])
    broken(other_octave)

    def mixed_group(w):                                           # a group with two keys: a padding copy of another bucket's code
        other = w["codes"][np.nonzero(wm.keys_of(w["codes"]) != wm.keys_of(w["codes"][pad:pad + 1])[0])[0][0]]
        w["codes"][pad] = other
        w["tiles"] = wm.planes_of(w["codes"])
    broken(mixed_group)


def rule_by_sorting(qt, nsp):
    """The wide rule, stated once: order rows 5..15 by (score, -s) and defer the first 11 - nsp."""
    t = qt.reshape(M, 16).astype(np.int64)
    order = sorted(range(5, M), key=lambda s: (int(t[s].sum()) - 16 * int(t[s].min()), -s))
    deferred = order[:11 - nsp]
    return sum(1 << s for s in deferred), min(127, sum(int(t[s].min()) for s in deferred))


@pytest.mark.parametrize("nsp", bs.NSPS_WIDE)
def test_choose_bktw_is_the_rule(nsp):
    rng = np.random.default_rng(nsp)
    for trial in range(200):
        qt = rng.integers(0, int(rng.integers(2, 128)), (M, 16)).astype(np.int8)
        if trial % 3 == 0:
            qt[rng.integers(0, M, 5)] = qt[0]                    # equal rows: ties
        if trial % 5 == 0:
            qt[4] = 0                                            # row 4 however flat: free, never deferred (the rule among 4-15 would take it)
        mask, c = bs.choose_bktw(qt, nsp)
        assert (mask, c) == rule_by_sorting(qt, nsp)
        assert mask & 0x1f == 0 and bin(mask).count("1") == 11 - nsp and 0 <= c <= 127
        assert sorted(list(bs.FREE_WIDE) + bs.bktw_paid(mask) + [s for s in range(M) if mask >> s & 1]) == list(range(M))
    qt = np.zeros((M, 16), np.int8)
    assert [bs.choose_bktw(qt, p)[0] for p in bs.NSPS_WIDE] == [0xff00, 0xfe00, 0xfc00, 0xf800]
    qt = np.random.default_rng(3).integers(0, 100, (M, 16)).astype(np.int8)
    m = [bs.choose_bktw(qt, p)[0] for p in (6, 5, 4, 3)]
    assert all(a & b == a for a, b in zip(m, m[1:]))             # nested


@pytest.mark.parametrize("nsp", bs.NSPS_WIDE)
def test_wide_rate_equals_a_brute_force_count_and_the_slack_loses_no_candidate(nsp):
    """Every code of the 5 free and nsp paid rows enumerated is too many; the rate is a probability over uniform nibbles, so the
    count runs over a uniform sample of 400 000 codes and must agree within 5 binomial standard deviations."""
    n = 400_000
    rng = np.random.default_rng(91)
    codes = rng.integers(0, 256, (n, M // 2), dtype=np.uint8)
    nibbles = np.empty((n, M), np.uint8)
    nibbles[:, 0::2] = codes & 15
    nibbles[:, 1::2] = codes >> 4
    tables = ss.headline_tables(2, 99)
    for q in range(2):
        s = ss.float_sums(tables[q], codes[:100_000])
        qt = ss.quantize(tables[q], np.partition(s, 9)[9])
        t = qt.reshape(M, 16).astype(np.int64)
        mask, c = bs.choose_bktw(qt, nsp)
        subs = list(bs.FREE_WIDE) + bs.bktw_paid(mask)
        assert c == min(127, sum(int(t[s].min()) for s in range(M) if s not in subs))
        partial = np.minimum(sum(t[s][nibbles[:, s]] for s in subs), 127)
        full = np.minimum(sum(t[s][nibbles[:, s]] for s in range(M)), 127)
        for n_before in (1 << 14, 1 << 17, 1 << 20):
            bound = ss.bound_at(qt, n_before)
            assert not np.any((full < bound) & (partial >= max(bound - c, 0))), (q, n_before)
            rate = bs.survivor_rate_bktw(qt, nsp, bound)
            count = float(np.mean(partial < max(bound - c, 0)))
            assert abs(rate - count) <= 5 * np.sqrt(max(rate, 1e-6) / n) + 1e-9, (q, n_before, rate, count)


def test_expected_padding_equals_a_simulation():
    rng = np.random.default_rng(4)
    for lam in (32, 128, 442):
        sizes = rng.poisson(lam, 200_000)
        sim = float(((-sizes) % 16).sum() / sizes.sum())
        assert abs(bs.expected_padding(lam) - sim) < 0.02 * sim + 1e-4, (lam, sim)
    assert abs(bs.expected_padding(128) - 0.0586) < 5e-4 and abs(bs.expected_padding(442) - 0.0170) < 5e-4
