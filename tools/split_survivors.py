"""CPU model of the split scan's survivor rates, numpy only.
usage: python tools/split_survivors.py [codes=1e9] [queries=32] [seed=1234]

The bench's codes are iid uniform bytes, so a code byte b contributes the pair entry P_b[x] = q[2b][x & 15] + q[2b+1][x >> 4]
of a uniform x, and the distribution of a sum over any set of bytes is the exact convolution of the per-byte histograms of
the query's int8 tables.  For the headline's queries (bench.make_tables on default_rng(seed), the first batch; qmax = the
matching quantile of the float sums of a uniform sample, QuantizerMAX as the library's quant_mode 1) and every split level
(it starts at N = 2^23, 2^25, 2^27, 2^29 codes), the bound is taken as the R/N quantile of min(127, full sum), and the
survivor rate of a set of streamed bytes is P(min(127, partial) < bound).  Printed per level: the mean (and max) rate over
the queries for 7 bytes (0-6), 6 fixed bytes (0-5), 6 bytes chosen by the library's rule (drop byte 7 and the byte of 0-6 whose
pair entries have the smallest sum; ties: the highest) and the best single deferred byte, the two ratios rule / fixed and
rule / best, and bytes per (code, query) = k + rate x G for G = 64 and 128 B per survivor, weighted over the levels.
The slack columns use the survivor test of the 5-plane form: every deferred byte b contributes at least min P_b, so with
c = min(127, the sum of min P_b over the deferred bytes) a code survives when min(127, partial) < bound - c.  "6 slack" is the
6-plane rule's choice with that test (a what-if: the library's 6-plane form tests against the bound itself), "5 slack" the
5-plane form as the library runs it (choose_planes5: byte 7 and the two bytes of 0-6 with the smallest
score_j = sum of the two rows - 16 min P_j, ties: the highest j), "5 plain" the same bytes without the slack.
"nib 10", "nib 9", "nib 8": the nibble form (choose_nib: 6, 7 or 8 of the 16 sub-quantizers deferred, any of them, byte 7's
included, by the same score per row; the test with the slack of the deferred rows' minima); 5, 4.5 and 4 bytes streamed.
Compare the rates with the library's split_survivors / split6_codes and split5_survivors / split5_codes (qadc_profile,
tools/split_ab.py parts split6 and split5).
One JSON line at the end."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 16
R, KEEP = 100, 0.01                # bench.py's
LEVEL_STARTS = [1 << 23, 1 << 25, 1 << 27, 1 << 29]


def quantize(table, qmax):
    """QuantizerMAX<int8> as the library runs it (quant_mode 1): table float32 [M*16] -> int8 [M][16]."""
    t = np.maximum(table.astype(np.float32), np.float32(0))
    qmin = np.float32(t.min())
    scale = np.float32(127.0) / (np.float32(qmax) - qmin)
    o = ((t - qmin) * scale).astype(np.float32)
    o = np.where(t >= np.float32(qmax), 127, np.minimum(np.trunc(o), 127)).astype(np.int64)
    return o.reshape(M, 16).astype(np.int8)


def pair_entries(qt):
    """[8][256]: P_b[x] for the 8 code bytes of a 16x4 code."""
    t = qt.reshape(M, 16).astype(np.int64)
    x = np.arange(256)
    return np.stack([t[2 * b][x & 15] + t[2 * b + 1][x >> 4] for b in range(M // 2)])


def choose_plane(qt):
    """The library's rule: the byte j in 0..6 with the smallest pair-entry sum, ties: the highest j."""
    sums = pair_entries(qt)[:7].sum(axis=1)
    return int(max(j for j in range(7) if sums[j] == sums.min()))


def choose_planes5(qt):
    """The library's rule for the 5-plane form -> (j1, j2, c): the two bytes of 0..6 with the smallest
    score_j = sum of rows 2j and 2j+1 - 16 (min row 2j + min row 2j+1), one pick after the other, ties: the highest j;
    c = min(127, min P_j1 + min P_j2 + min P_7)."""
    t = qt.reshape(M, 16).astype(np.int64)
    minp = [int(t[2 * j].min() + t[2 * j + 1].min()) for j in range(8)]
    score = [int(t[2 * j].sum() + t[2 * j + 1].sum()) - 16 * minp[j] for j in range(7)]
    a = max(j for j in range(7) if score[j] == min(score))
    rest = [j for j in range(7) if j != a]
    b = max(j for j in rest if score[j] == min(score[r] for r in rest))
    j1, j2 = min(a, b), max(a, b)
    return j1, j2, min(127, minp[j1] + minp[j2] + minp[7])


def slack(qt, deferred):
    """min(127, the sum over the deferred bytes of their pair table's smallest entry): a part of every code's sum."""
    return int(min(127, pair_entries(qt)[list(deferred)].min(axis=1).sum()))


def sum_distribution(qt, planes):
    """P(sum over the bytes in `planes` = v) for v = 0 .. 254 * len(planes), codes iid uniform."""
    pe = pair_entries(qt)
    d = np.ones(1)
    for b in planes:
        d = np.convolve(d, np.bincount(pe[b], minlength=255) / 256.0)
    return d


def bound_at(qt, n_before, r=R):
    """The bound a level that starts after n_before codes works with: the smallest v such that n_before codes are expected
    to hold r values <= v (values = min(127, full sum)), else 127."""
    cdf = np.cumsum(sum_distribution(qt, range(8)))[:127]
    hit = np.nonzero(cdf * n_before >= r)[0]
    return int(hit[0]) if len(hit) else 127


def survivor_rate(qt, planes, bound, c=0):
    """P(min(127, partial sum over `planes`) < bound - c); c = the slack of the deferred bytes (0: the plain test)."""
    bound = max(bound - c, 0)
    return float(sum_distribution(qt, planes)[:min(bound, 127)].sum()) if bound > 0 else 0.0


def choose_nib(qt, ns):
    """The library's rule for the nibble form with ns streamed sub-quantizers (plane_choice_nib) -> (mask, c): the 16 - ns
    sub-quantizers with the smallest score_s = sum of row s - 16 min row s, one pick after the other, ties: the highest s,
    as a 16-bit mask; c = min(127, the sum of min row s over them)."""
    t = qt.reshape(M, 16).astype(np.int64)
    score = [int(t[s].sum()) - 16 * int(t[s].min()) for s in range(M)]
    mask = 0
    for _ in range(M - ns):
        rest = [s for s in range(M) if not mask >> s & 1]
        best = min(score[s] for s in rest)
        mask |= 1 << max(s for s in rest if score[s] == best)
    return mask, min(127, sum(int(t[s].min()) for s in range(M) if mask >> s & 1))


def nib_streamed(mask):
    """The streamed sub-quantizers in the kernel's order: ascending, cyclically, from behind the highest deferred one; fused in
    pairs from the front, an odd count leaves the last one as the single plane."""
    start = mask.bit_length() & 15
    return [s for s in ((start + i) & 15 for i in range(M)) if not mask >> s & 1]


def sum_distribution_nib(qt, subs):
    """P(sum over the sub-quantizers in `subs` = v), codes iid uniform (a sub-quantizer's nibble is uniform in 0..15)."""
    t = qt.reshape(M, 16).astype(np.int64)
    d = np.ones(1)
    for s in subs:
        d = np.convolve(d, np.bincount(t[s], minlength=128) / 16.0)
    return d


def survivor_rate_nib(qt, subs, bound, c=0):
    """P(min(127, partial sum over the sub-quantizers `subs`) < bound - c)."""
    bound = max(bound - c, 0)
    return float(sum_distribution_nib(qt, subs)[:min(bound, 127)].sum()) if bound > 0 else 0.0


def streamed(j):
    return [b for b in range(7) if b != j]


def headline_tables(nq, seed):
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(seed)
    codebooks = rng.normal(size=(M, 16, 128 // M)).astype(np.float32)
    return bench.make_tables(rng, codebooks, nq)[:, 0, :]


def float_sums(table, codes):
    t = table.reshape(M, 16)
    s = np.zeros(len(codes), np.float32)
    for b in range(M // 2):
        s += t[2 * b][codes[:, b] & 15] + t[2 * b + 1][codes[:, b] >> 4]
    return s


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(1e9)
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1234
    tables = headline_tables(nq, seed)
    # qmax: the R-th smallest float sum of the KEEP x n starts = the R / (KEEP n) quantile, taken on a uniform sample
    starts = max(1, int(KEEP * n))
    sample = min(starts, 2_000_000)
    codes = np.random.default_rng(seed + 1).integers(0, 256, (sample, M // 2), dtype=np.uint8)
    k = max(1, int(round(R * sample / starts)))
    qts = []
    for q in range(nq):
        s = float_sums(tables[q], codes)
        qts.append(quantize(tables[q], np.partition(s, k - 1)[k - 1]))
    levels = [(a, min(b, n) - a) for a, b in zip(LEVEL_STARTS, LEVEL_STARTS[1:] + [1 << 62]) if a < n]
    forms = ("7 bytes", "6 fixed", "6 rule", "6 best", "6 slack", "5 slack", "5 plain", "nib 10", "nib 9", "nib 8")
    out = {"codes": n, "queries": nq, "seed": seed, "levels": []}
    print("%-10s %-12s " % ("level", "codes") + " ".join("%-22s" % f for f in forms) + " rule/fixed  rule/best")
    for start, size in levels:
        rates = {f: [] for f in forms}
        for qt in qts:
            bound = bound_at(qt, start)
            per_j = [survivor_rate(qt, streamed(j), bound) for j in range(7)]
            rates["7 bytes"].append(survivor_rate(qt, range(7), bound))
            rates["6 fixed"].append(per_j[6])
            rates["6 rule"].append(per_j[choose_plane(qt)])
            rates["6 best"].append(min(per_j))
            j = choose_plane(qt)
            rates["6 slack"].append(survivor_rate(qt, streamed(j), bound, slack(qt, (j, 7))))
            j1, j2, c = choose_planes5(qt)
            five = [b for b in range(7) if b not in (j1, j2)]
            assert c == slack(qt, (j1, j2, 7))
            rates["5 slack"].append(survivor_rate(qt, five, bound, c))
            rates["5 plain"].append(survivor_rate(qt, five, bound))
            for ns in (10, 9, 8):
                mask, cn = choose_nib(qt, ns)
                rates["nib %d" % ns].append(survivor_rate_nib(qt, nib_streamed(mask), bound, cn))
        mean = {f: float(np.mean(v)) for f, v in rates.items()}
        print("2^%-8d %-12d " % (start.bit_length() - 1, size) +
              " ".join("%-22s" % ("%.2e (max %.1e)" % (mean[f], max(rates[f]))) for f in forms) +
              " %-11.3f %.3f" % (mean["6 rule"] / mean["6 fixed"], mean["6 rule"] / mean["6 best"]))
        out["levels"].append({"start": start, "codes": size, "mean_rate": mean, "max_rate": {f: max(v) for f, v in rates.items()}})
    total = sum(size for _, size in levels)
    out["bytes_per_code"] = {}
    for f, kbytes in zip(forms, (7, 6, 6, 6, 6, 5, 5, 5, 4.5, 4)):
        p = sum(l["mean_rate"][f] * l["codes"] for l in out["levels"]) / total
        out["bytes_per_code"][f] = {"rate": p, "G64": kbytes + p * 64, "G128": kbytes + p * 128}
        print("%-8s weighted rate %.2e   bytes per (code, query): %.3f (G = 64 B)  %.3f (G = 128 B)" % (f, p, kbytes + p * 64, kbytes + p * 128))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
