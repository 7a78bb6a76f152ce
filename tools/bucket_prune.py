"""CPU model of the bucket scan's group test ("pruned groups"), numpy only, beside tools/bucket_survivors.py.
usage: python tools/bucket_prune.py [codes=1e9] [queries=32] [seed=1234]

A 16-slot lane group of a wide octave has one 20-bit key, so the rows the pair loop starts from are known from its id:
s0 = T0 + T1 + T2 + T3 + T4 at the key's nibbles (an odd NSP fuses row 4 into the first pair table: s0 = rows 0-3 and row 4 counts
with its minimum).  With pmin = the sum of min T[s] over the other rows the loop adds, every slot has partial >= s0 + pmin; the group
is pruned when s0 + pmin >= bsurv = max(0, bound - c), and a wave iteration (64 consecutive groups in key order) is skipped when
all of its groups are.  For iid uniform codes every key has the same expected number of groups, so the fraction of lane groups
pruned is the fraction of the 2^20 keys pruned, exactly; the wave figure lays the keys out in key order, codes_per_key / 16 groups
each, and counts the windows of 64 groups that touch no kept key.

Printed per level from 2^27 on, octave (codes per key) and NSP, as means over the headline's queries: groups pruned, waves
skipped, bytes per (code, query) = (NSP / 2) x (1 - waves skipped) + 3 / 16 + 128 x survivor rate.  The narrow form (16-bit key,
4 free rows) gets the group figure only.  Compare with the library's bktw_prune_groups, bktw_prune_skipped and bktw_prune_run
(qadc_profile).  One JSON line at the end.

With bkt_prune_lanes = 16 a wave iteration that runs loads by aligned 16-lane quarters (128 contiguous bytes of a plane each): the
same count over windows of 16 groups gives the fraction of the plane bytes that is not read ("quarters skipped": the quarters of
skipped wave iterations and the idle quarters of the others), and the byte model becomes (NSP / 2) x (1 - plane bytes skipped) +
3 / 16 + 128 x survivor rate ("bytes16").  The library's bktw_prune_quarters counts the idle quarters of the wave iterations that
ran only: quarter_counter_fraction x bktw_slots / 256."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bucket_survivors as bs  # noqa: E402
import split_survivors as ss  # noqa: E402

M = bs.M
WAVE_GROUPS = 64
QUARTER_GROUPS = 16


def key_sums(qt, rows):
    """Sum of T[s][nibble s of the key] over `rows` (a prefix 0..len-1 of the sub-quantizers) for every key of 4 len bits,
    key = nibble 0 | nibble 1 << 4 | ..: int64 [16 ** len]."""
    t = qt.reshape(M, 16).astype(np.int64)
    out = np.zeros(1, np.int64)
    for s in rows:
        out = (out[None, :] + t[s][:, None]).reshape(-1)      # nibble s becomes the most significant so far
    return out


def wide_terms(qt, nsp, bound):
    """-> (s0 int64 [2^20] per key, pmin, bsurv) as the wide kernel with nsp paid planes forms them."""
    t = qt.reshape(M, 16).astype(np.int64)
    mask, c = bs.choose_bktw(qt, nsp)
    paid = bs.bktw_paid(mask)
    fuse = nsp % 2 == 1
    pmin = sum(int(t[s].min()) for s in paid) + (int(t[4].min()) if fuse else 0)
    s0 = key_sums(qt, range(4))
    s0 = np.tile(s0, 16) if fuse else key_sums(qt, range(5))
    return s0, pmin, max(0, int(bound) - c)


def narrow_terms(qt, nsp, bound):
    """The narrow form's: 16-bit key, rows 0-3 free, nsp of rows 4-15 paid."""
    t = qt.reshape(M, 16).astype(np.int64)
    mask, c = bs.choose_bkt(qt, nsp)
    pmin = sum(int(t[s].min()) for s in bs.bkt_paid(mask))
    return key_sums(qt, range(4)), pmin, max(0, int(bound) - c)


def kept_keys(terms):
    s0, pmin, bsurv = terms
    return s0 + pmin < bsurv


def group_fraction(keep):
    """Fraction of lane groups pruned on iid uniform codes = fraction of keys pruned."""
    return 1.0 - float(np.count_nonzero(keep)) / keep.size


def wave_fraction(keep, codes_per_key):
    """Fraction of the wave iterations skipped: key k's groups lie at [k g, (k + 1) g) with g = codes_per_key / 16 on an axis
    cut into windows of 64 groups; a window is skipped when no kept key overlaps it.  Never above group_fraction(keep): the
    skipped windows are disjoint stretches of pruned groups."""
    g = float(codes_per_key) / 16.0
    nwaves = int(keep.size * g // WAVE_GROUPS)
    if nwaves == 0:
        return 0.0
    w = np.arange(nwaves, dtype=np.float64)
    k0 = np.floor(w * WAVE_GROUPS / g).astype(np.int64)
    k1 = np.minimum(np.ceil((w + 1) * WAVE_GROUPS / g).astype(np.int64), keep.size)   # keys [k0, k1) overlap window w
    cum = np.concatenate([[0], np.cumsum(keep.astype(np.int64))])
    return float(np.count_nonzero(cum[k1] == cum[k0])) / nwaves


def window_fraction(keep, codes_per_key, groups):
    """wave_fraction's count over windows of `groups` consecutive lane groups (64: a wave iteration, 16: one of its quarters; a
    divisor of 64, so that the windows tile the wave iterations)."""
    g = float(codes_per_key) / 16.0
    nwin = int(keep.size * g // WAVE_GROUPS) * (WAVE_GROUPS // groups)
    if nwin == 0:
        return 0.0
    w = np.arange(nwin, dtype=np.float64)
    k0 = np.floor(w * groups / g).astype(np.int64)
    k1 = np.minimum(np.ceil((w + 1) * groups / g).astype(np.int64), keep.size)
    cum = np.concatenate([[0], np.cumsum(keep.astype(np.int64))])
    return float(np.count_nonzero(cum[k1] == cum[k0])) / nwin


def quarter_fraction(keep, codes_per_key):
    """Fraction of the 16-lane quarters that load no plane with bkt_prune_lanes = 16 = fraction of the plane bytes skipped: the
    quarters of skipped wave iterations and the idle quarters of those that run.  Between wave_fraction and group_fraction."""
    return window_fraction(keep, codes_per_key, QUARTER_GROUPS)


def quarter_counter_fraction(keep, codes_per_key):
    """What bktw_prune_quarters counts, as a fraction of all quarters: idle quarters of the wave iterations that run."""
    return quarter_fraction(keep, codes_per_key) - wave_fraction(keep, codes_per_key)


def plane_bytes(nsp, skipped, rate):
    """Bytes per (code, query): the paid planes that are read, the ids (3 / 16) and 128 bytes of side array per survivor."""
    return nsp / 2 * (1 - skipped) + 0.1875 + 128 * rate


def octaves(n, start):
    """Codes per 20-bit key of the octaves a level from `start` covers in a list of n codes (wide blocks from 2^27)."""
    stop = min(n, 4 * start)
    out, lo = [], start
    while lo < stop:
        hi = min(2 * lo, stop)
        out.append((hi - lo) / bs.WIDE_KEYS)
        lo = hi
    return out


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(1e9)
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1234
    qts = bs.headline_qtables(n, nq, seed)
    out = {"codes": n, "queries": nq, "seed": seed, "wide": [], "narrow": []}
    print("%-6s %-9s %-4s %-14s %-14s %-22s %-8s %-16s %s" % ("level", "codes/key", "NSP", "groups pruned", "waves skipped", "waves: min..max", "bytes",
                                                        "quarters skipped", "bytes16"))
    for start in (s for s in bs.WIDE_STARTS if s < n):
        for cpk in octaves(n, start):
            for nsp in bs.NSPS_WIDE:
                gf, wf, rate, qf = [], [], [], []
                for qt in qts:
                    bound = ss.bound_at(qt, start)
                    keep = kept_keys(wide_terms(qt, nsp, bound))
                    gf.append(group_fraction(keep))
                    wf.append(wave_fraction(keep, cpk))
                    qf.append(quarter_fraction(keep, cpk))
                    rate.append(bs.survivor_rate_bktw(qt, nsp, bound))
                b = plane_bytes(nsp, np.mean(wf), np.mean(rate))
                b16 = plane_bytes(nsp, np.mean(qf), np.mean(rate))
                print("2^%-4d %-9.0f %-4d %-14.3f %-14.3f %-22s %.2f B   %-16.3f %.2f B" %
                      (start.bit_length() - 1, cpk, nsp, np.mean(gf), np.mean(wf), "%.2f..%.2f" % (min(wf), max(wf)), b, np.mean(qf), b16))
                out["wide"].append({"start": start, "codes_per_key": cpk, "nsp": nsp, "groups": float(np.mean(gf)),
                                    "waves": float(np.mean(wf)), "waves_min": min(wf), "waves_max": max(wf), "bytes": float(b),
                                    "quarters": float(np.mean(qf)), "bytes16": float(b16)})
    for nsp in bs.NSPS:
        gf = [group_fraction(kept_keys(narrow_terms(qt, nsp, ss.bound_at(qt, 1 << 25)))) for qt in qts]
        print("2^25   narrow    %-4d %-14.3f" % (nsp, np.mean(gf)))
        out["narrow"].append({"start": 1 << 25, "nsp": nsp, "groups": float(np.mean(gf))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
