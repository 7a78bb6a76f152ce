"""Same-process sweep behind the bucket form's defaults (profiles/r11_bkt_ab.txt).
usage: python tools/bkt_sweep.py [reps=2] [codes=1e9] [wide=W] [prune=1]

One index of the headline's list and mode (bench.py's one-query-per-pass options, 32-query steps pipelined three deep) holding
BOTH the bucket copy (blocks of 2^25) and the nibble-plane copy: it is finalized with bkt_min_run above every run (600 Mi), so
that finalize still builds the nibble-plane copy, and the thresholds are moved afterwards.  Arms, interleaved inside every round,
order alternated: "off" = the nibble defaults (9 / 9 / 8 streamed); "pXYZ" = X, Y and Z paid planes at the levels from 2^25, 2^27
and 2^29 (runs of 96, 384 and 421 Mi codes) with bkt_min_run = 2^25; "b27:pYZ" = bkt_min_run = 2^27 (the level from 2^25 keeps 9
nibble planes).  A first section times the PROBE builds (variant bit 16) of "off" and of two arms.  One JSON line per (section,
round, arm): ms per step and the library's bkt_* and nib_* counters per step; a last line has the copies' sizes and the finalize time.

With a third argument wide=W (W = 2^27 or 2^29; profiles/r12_bktw_ab.txt) the index is the default one with wide blocks from W on
(a range stored wide has no narrow blocks and the index no nibble-plane copy, so the narrow arms cannot run beside them): arms
"w:pYZ" = Y and Z paid planes of rows 5-15 at the levels from 2^27 and 2^29 (W = 2^29: "w:pZ", the level from 2^27 keeps the narrow
form's 5), the level from 2^25 the narrow form's 6; the PROBE section times "w:p44".  The lines carry the bktw_* counters as well.

With a fourth argument prune=1 (profiles/r13_prune_ab.txt) every wide arm runs twice, interleaved: without the wide form's group
test (Index.set_bkt_prune(0)) and, named "w:pYZ+g", with it; without the argument the arms run under the library's default, which
is the test on.  A fifth argument variant=V (default 0x0d) sets the loop form of the sweep section: 0x05 = strided tiles in place of chunks; the PROBE section times both builds of "w:p44", and the lines carry the
group test's counters (wave iterations skipped and run, lane groups pruned).

With tiles_lanes=1 anywhere after the fourth argument (profiles/r14_bkt_tiles_lanes.txt) every "+g" arm runs four times, interleaved:
"/c64" and "/c16" = the bucket launches follow the variant (Index.set_bkt_tiles(0); chunks under 0x0d) with the group test by whole waves
and by 16-lane quarters (Index.set_bkt_prune_lanes), "/s64" and "/s16" = strided tiles for the bucket launches alone
(set_bkt_tiles(1)); the lines carry the fourth counter (idle quarters of the wave iterations that ran).  arms=A,B,.. keeps only the
named arms (before the suffixes), probe=0 leaves the PROBE section out."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

MI = 1 << 20
NEVER = 1 << 40


def arm_thresholds(name):
    """-> (bkt_min_run, min_run6, min_run5, min_run4)"""
    if name == "off":
        return NEVER, 0, 0, 0
    lo = 128 * MI if name.startswith("b27:") else 32 * MI
    planes = [int(c) for c in name.split("p")[1]]
    planes = [planes[0]] * (3 - len(planes)) + planes          # per level from 2^25, 2^27, 2^29 (non-increasing)
    reach = (32 * MI, 128 * MI, 400 * MI)                        # a threshold that the level's runs and the longer ones reach
    t = {}
    for want in (6, 5, 4):
        first = [i for i, p in enumerate(planes) if p <= want]
        t[want] = reach[first[0]] if first else 0
    return lo, t[6], t[5], t[4]


def wide_thresholds(name):
    """"w:pYZ" / "w:pZ" -> (min_run5, min_run4, min_run3): thresholds that the level's runs and the longer ones reach."""
    planes = [int(c) for c in name.split("/")[0].split("+")[0].split("p")[1]]
    planes = [planes[0]] * (2 - len(planes)) + planes            # per level from 2^27, 2^29 (non-increasing)
    reach = (128 * MI, 400 * MI)
    t = {}
    for want in (5, 4, 3):
        first = [i for i, p in enumerate(planes) if p <= want]
        t[want] = reach[first[0]] if first else 0
    return t[5], t[4], t[3]


def main():
    import torch
    import pyqadc
    torch.zeros(1, device="cuda:0")
    pyqadc.device_prepare(0)
    import gc
    gc.collect(); gc.freeze(); gc.disable()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    n = int(float(sys.argv[2])) if len(sys.argv) > 2 else int(1e9)
    steps, warmup, nq, M = 10, 3, 32, 16
    rng = np.random.default_rng(1234)
    codebooks = rng.normal(size=(M, 16, 128 // M)).astype(np.float32)
    pool = [bench.make_tables(rng, codebooks, nq) for _ in range(4)]
    assign = np.zeros((nq, 1), np.int32)

    def run(idx, k):
        pending = []
        for s in range(k):
            idx.submit(s % 3, assign, pool[s % len(pool)].copy(), bench.R)
            pending.append(s % 3)
            if len(pending) == 3:
                idx.collect(pending.pop(0))
        while pending:
            idx.collect(pending.pop(0))

    wide = int(float(sys.argv[3].split("=")[1])) if len(sys.argv) > 3 and sys.argv[3].startswith("wide=") else 0
    prune = len(sys.argv) > 4 and sys.argv[4] == "prune=1"
    sweep_variant = int(sys.argv[5].split("=")[1], 0) if len(sys.argv) > 5 and sys.argv[5].startswith("variant=") else 0x0d
    extra = dict(a.split("=", 1) for a in sys.argv[5:] if "=" in a)
    tiles_lanes = extra.get("tiles_lanes") == "1"
    idx = pyqadc.Index(M, 0)
    if wide:
        idx.set_split_bkt_wide(wide, min(max(wide, 128 * MI), 400 * MI), 0, 0, 0)
    else:
        idx.set_split_bkt(600 * MI, 1 << 25)
        idx.set_split_bkt_wide(0)
    idx.add_partition_synthetic_shard(n, 0, n, bench.SEED, max(1, int(np.float32(n) * np.float32(bench.KEEP))))
    t0 = time.perf_counter()
    idx.finalize(bench.KEEP)
    finalize_s = time.perf_counter() - t0
    idx.set_option("profile", 1)
    bench.set_mode(idx, bench.MODE_ONE_QUERY_PER_PASS)
    sizes = {k: int(idx.profile()[k]) for k in ("split_copy_bytes", "nib_copy_bytes", "bkt_copy_bytes", "bkt_copy_slots",
                                               "bktw_copy_bytes", "bktw_copy_slots", "bktw_copy_fallback")}

    def measure(section, rep, name, variant):
        idx.set_option("variant", variant)
        if wide:
            idx.set_split_bkt_wide(wide, min(max(wide, 128 * MI), 400 * MI), *wide_thresholds(name))
            if prune:                                            # (without prune=1 the library's default stays)
                idx.set_bkt_prune(int("+g" in name))
            if "/" in name:                                      # tile order and granularity of the group test's loads
                idx.set_bkt_tiles(int(name.split("/")[1][0] == "s"))
                idx.set_bkt_prune_lanes(int(name.split("/")[1][1:]))
        else:
            lo, t6, t5, t4 = arm_thresholds(name)
            idx.set_split_bkt(lo, 0, t6, t5, t4)
        run(idx, warmup)
        idx.profile_reset()
        t0 = time.perf_counter()
        run(idx, steps)
        ms = (time.perf_counter() - t0) * 1e3 / steps
        pr = idx.profile()
        keys = ("bkt_launches", "bkt_codes", "bkt_slots", "bkt_survivors", "nib_codes", "nib_survivors", "nib8_codes", "nib8_survivors",
                "bktw_launches", "bktw_codes", "bktw_slots", "bktw_survivors", "bktw_prune_skipped", "bktw_prune_run", "bktw_prune_groups", "bktw_prune_quarters")
        print(json.dumps({"section": section, "round": rep, "arm": name, "ms_per_step": round(ms, 4),
                          **{k + "_per_step": int(pr[k] // steps) for k in keys}}), flush=True)

    probe = ["off", "p655", "p654"]
    arms = ["off", "p777", "p666", "p665", "p655", "p654", "p555", "p554", "p544", "p444", "p755", "p765",
            "b27:p66", "b27:p65", "b27:p55", "b27:p54"]
    if wide:
        probe = ["w:p44", "w:p66"] if wide <= 128 * MI else ["w:p4"]
        arms = ["w:p66", "w:p65", "w:p64", "w:p55", "w:p54", "w:p44", "w:p43", "w:p33"] if wide <= 128 * MI else ["w:p6", "w:p5", "w:p4", "w:p3"]
    if wide and prune:
        probe = [a + g for a in probe for g in ("", "+g")]
        arms = [a + g for a in arms for g in ("", "+g")]
    if "arms" in extra:
        arms = [a for a in arms if a.split("+")[0] in extra["arms"].split(",")]
    if tiles_lanes:
        arms = [a + t for a in arms if a.endswith("+g") for t in ("/c64", "/s64", "/c16", "/s16")]   # (needs prune=1)
    if extra.get("probe") == "0":
        probe = []
    for rep in range(reps):
        for name in (probe if rep % 2 == 0 else probe[::-1]):
            measure("probe", rep, name, 0x0d | 16)
    for rep in range(reps):
        for name in (arms if rep % 2 == 0 else arms[::-1]):
            measure("sweep", rep, name, sweep_variant)
    print(json.dumps({"section": "sizes", "codes": n, "finalize_s": round(finalize_s, 3), **sizes}), flush=True)
    idx.close()


if __name__ == "__main__":
    main()
