"""CPU model of the bucket form's survivor rates, numpy only; tools/split_survivors.py's model with
sub-quantizers 0-3 free.
usage: python tools/bucket_survivors.py [codes=1e9] [queries=32] [seed=1234]

In the bucket copy every 16-slot lane group holds codes of one key = code bytes 0 and 1, so sub-quantizers 0-3 cost 2 bytes per
16 codes and their table entries enter the partial sum exactly.  Of the other 12 the table defers 12 - NSP (choose_bkt: the rule of
choose_nib among rows 4..15) and pays for NSP = 4, 5, 6 or 7 nibble planes.  For the headline's queries and every level from 2^25
codes on, printed per NSP: the mean survivor rate P(min(127, partial over rows 0-3 and the paid rows) < bound - c) and bytes per
(code, query) = NSP / 2 + 1 / 8 + 128 x rate (padding not included: 2 to 3 % on uniform codes).  The nibble form's columns
(8, 9, 10 streamed) are split_survivors' own functions, for comparison.  Compare the rates with the library's
bkt_survivors / bkt_slots (qadc_profile).  One JSON line at the end.

Wide octaves (levels from 2^27 on): the group's key has 20 bits, sub-quantizers 0-4 are free (3 bytes per 16 slots), and NSP = 3,
4, 5 or 6 of rows 5..15 are paid (choose_bktw); bytes = NSP / 2 + 3 / 16 + 128 x rate.  Padding is not in the columns: a bucket of
Poisson(codes per key) codes rounded up to 16 slots (expected_padding) is printed per block size beside them."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_survivors as ss  # noqa: E402

M = ss.M
FREE = (0, 1, 2, 3)
NSPS = (4, 5, 6, 7)
LEVEL_STARTS = [1 << 25, 1 << 27, 1 << 29]


def choose_bkt(qt, nsp):
    """The library's rule for the bucket form with nsp paid planes (plane_choice_bkt) -> (mask, c): the 12 - nsp sub-quantizers
    of 4..15 with the smallest score_s = sum of row s - 16 min row s, one pick after the other, ties: the highest s, as a 16-bit
    mask; c = min(127, the sum of min row s over them)."""
    t = qt.reshape(M, 16).astype(np.int64)
    score = [int(t[s].sum()) - 16 * int(t[s].min()) for s in range(M)]
    mask = 0
    for _ in range(12 - nsp):
        rest = [s for s in range(4, M) if not mask >> s & 1]
        best = min(score[s] for s in rest)
        mask |= 1 << max(s for s in rest if score[s] == best)
    return mask, min(127, sum(int(t[s].min()) for s in range(M) if mask >> s & 1))


def bkt_paid(mask):
    """The paid sub-quantizers in the kernel's order: those of 4..15 outside the mask, ascending; fused in pairs from the front, an
    odd count leaves the last one as the single plane."""
    return [s for s in range(4, M) if not mask >> s & 1]


FREE_WIDE = (0, 1, 2, 3, 4)
NSPS_WIDE = (3, 4, 5, 6)
WIDE_STARTS = [1 << 27, 1 << 29]
WIDE_KEYS = 1 << 20


def choose_bktw(qt, nsp):
    """plane_choice_bktw: choose_bkt's rule among rows 5..15: the 11 - nsp smallest scores, ties: the highest s -> (mask, c)."""
    t = qt.reshape(M, 16).astype(np.int64)
    score = [int(t[s].sum()) - 16 * int(t[s].min()) for s in range(M)]
    mask = 0
    for _ in range(11 - nsp):
        rest = [s for s in range(5, M) if not mask >> s & 1]
        best = min(score[s] for s in rest)
        mask |= 1 << max(s for s in rest if score[s] == best)
    return mask, min(127, sum(int(t[s].min()) for s in range(M) if mask >> s & 1))


def bktw_paid(mask):
    """The paid sub-quantizers of the wide form in the kernel's order: those of 5..15 outside the mask, ascending.  An even count
    is fused in pairs from the front (row 4 is a lookup of its own); an odd count: row 4 is fused with the first, the rest in pairs."""
    return [s for s in range(5, M) if not mask >> s & 1]


def survivor_rate_bktw(qt, nsp, bound):
    mask, c = choose_bktw(qt, nsp)
    return ss.survivor_rate_nib(qt, list(FREE_WIDE) + bktw_paid(mask), bound, c)


def expected_padding(codes_per_key, group=16):
    """Expected padding slots per code of buckets of Poisson(codes_per_key) codes, each rounded up to `group` slots."""
    lam = float(codes_per_key)
    k = np.arange(0, int(lam + 12 * np.sqrt(lam) + 64))
    logp = k * np.log(lam) - lam - np.cumsum(np.log(np.maximum(k, 1)))
    pmf = np.exp(logp)
    return float((pmf * ((-k) % group)).sum() / lam)


def survivor_rate_bkt(qt, nsp, bound):
    mask, c = choose_bkt(qt, nsp)
    return ss.survivor_rate_nib(qt, list(FREE) + bkt_paid(mask), bound, c)


def headline_qtables(n, nq, seed):
    """The headline's int8 tables as split_survivors.main derives them."""
    tables = ss.headline_tables(nq, seed)
    starts = max(1, int(ss.KEEP * n))
    sample = min(starts, 2_000_000)
    codes = np.random.default_rng(seed + 1).integers(0, 256, (sample, M // 2), dtype=np.uint8)
    k = max(1, int(round(ss.R * sample / starts)))
    return [ss.quantize(tables[q], np.partition(s, k - 1)[k - 1]) for q in range(nq) for s in [ss.float_sums(tables[q], codes)]]


def nib_rates(qts, start):
    """{ns: mean survivor rate} of the nibble form at a level start: split_survivors' figures."""
    out = {}
    for ns in (10, 9, 8):
        r = []
        for qt in qts:
            mask, c = ss.choose_nib(qt, ns)
            r.append(ss.survivor_rate_nib(qt, ss.nib_streamed(mask), ss.bound_at(qt, start), c))
        out[ns] = float(np.mean(r))
    return out


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(1e9)
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1234
    qts = headline_qtables(n, nq, seed)
    out = {"codes": n, "queries": nq, "seed": seed, "levels": []}
    print("%-8s " % "level" + " ".join("%-24s" % ("bkt %d" % p) for p in NSPS) + " ".join("%-24s" % ("nib %d" % s) for s in (10, 9, 8)))
    for start in (s for s in LEVEL_STARTS if s < n):
        rates = {p: float(np.mean([survivor_rate_bkt(qt, p, ss.bound_at(qt, start)) for qt in qts])) for p in NSPS}
        nib = nib_rates(qts, start)
        print("2^%-6d " % (start.bit_length() - 1) +
              " ".join("%-24s" % ("%.2e -> %.2f B" % (rates[p], p / 2 + 0.125 + 128 * rates[p])) for p in NSPS) +
              " ".join("%-24s" % ("%.2e -> %.2f B" % (nib[s], s / 2 + 128 * nib[s])) for s in (10, 9, 8)))
        out["levels"].append({"start": start, "bkt_rate": {str(p): rates[p] for p in NSPS},
                              "bkt_bytes": {str(p): p / 2 + 0.125 + 128 * rates[p] for p in NSPS},
                              "nib_rate": {str(s): nib[s] for s in nib}})
    print("%-8s " % "level" + " ".join("%-24s" % ("wide %d" % p) for p in NSPS_WIDE))
    out["wide_levels"] = []
    for start in (s for s in WIDE_STARTS if s < n):
        rates = {p: float(np.mean([survivor_rate_bktw(qt, p, ss.bound_at(qt, start)) for qt in qts])) for p in NSPS_WIDE}
        print("2^%-6d " % (start.bit_length() - 1) +
              " ".join("%-24s" % ("%.2e -> %.2f B" % (rates[p], p / 2 + 0.1875 + 128 * rates[p])) for p in NSPS_WIDE))
        out["wide_levels"].append({"start": start, "wide_rate": {str(p): rates[p] for p in NSPS_WIDE},
                                   "wide_bytes": {str(p): p / 2 + 0.1875 + 128 * rates[p] for p in NSPS_WIDE}})
    out["wide_padding"] = {}
    for block in [1 << 27, 1 << 28] + ([n - (1 << 29)] if n > 1 << 29 else []):
        pad = expected_padding(block / WIDE_KEYS)
        print("block of %d codes: %.0f codes per 20-bit key, expected padding %.1f %%" % (block, block / WIDE_KEYS, 100 * pad))
        out["wide_padding"][str(block)] = pad
    print(json.dumps(out))


if __name__ == "__main__":
    main()
