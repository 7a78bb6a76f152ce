"""Same-process A/B of the split scan and the sweeps behind its thresholds.
usage: python tools/split_ab.py [reps] [part]   (default 3 rounds, all parts; arms interleaved inside every round;
                                                 part = min_run | min_codes | split6 | split5 | nib: that part only)

Part 1, split_min_run: the headline's list and mode (10^9 codes, bench.py's one-query-per-pass options, 32-query steps
pipelined three deep as bench.py's run_steps), ONE index with its byte-plane copy; arms: split off (row-major scan) and
split_min_run = 2, 8, 32, 128 Mi.  Part 2, split_min_codes: lists of 1.6 x 10^7 codes (inside the 256 MiB Infinity Cache) and
4 x 10^7 codes (above it), copy built, arms split off / on at split_min_run = 2^23.  Part 3, split6_min_run: the headline's
list again at the default split_min_run, arms: 6-plane form off (7 planes everywhere) and split6_min_run = 8, 32, 128, 512 Mi,
i.e. from the level that starts at 2^23, 2^25, 2^27, 2^29 codes on.  Part 4, split5_min_run: the headline's list at the default
split_min_run and split6_min_run, arms: 5-plane form off and split5_min_run = 8 (for information), 32, 128, 400 Mi, i.e. from
the level that starts at 2^23, 2^25, 2^27, 2^29 codes on (the last level of 10^9 codes has 441.7 Mi codes: 512 Mi would be "off").
Parts 1 to 3 keep the 5-plane form off.  Part 5, nib: the headline's list at the defaults of the other thresholds, with the
nibble-plane copy built; arms: the nibble form off (5 planes), and NS = 9 and NS = 10 streamed sub-quantizers from 32, 128, 400 Mi
codes per run on, each alone and with 8 streamed from 128 or 400 Mi on (arm names ns<NS>@<Mi>[+8@<Mi>]).  Parts 1 to 4 keep the
nibble form off.
Prints one JSON line per (part, list, round, arm): ms per step over K steps and the library's split_codes, split6_codes,
split_survivors, split5_codes, split5_survivors, nib_codes, nib_survivors, nib8_codes and nib8_survivors per step."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

OFF = 1 << 40                     # split_min_run above any run: the row-major form
MI = 1 << 20


def main():
    import torch
    import pyqadc
    torch.zeros(1, device="cuda:0")
    pyqadc.device_prepare(0)
    import gc
    gc.collect(); gc.freeze(); gc.disable()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
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

    def measure(idx, min_codes, min_run, min_run6, min_run5, nib=(0, 0, 9)):
        idx.set_split(min_codes, min_run)
        idx.set_split6(min_run6)
        idx.set_split5(min_run5)
        idx.set_split_nib(*nib)
        run(idx, warmup)
        idx.profile_reset()
        t0 = time.perf_counter()
        run(idx, steps)
        ms = (time.perf_counter() - t0) * 1e3 / steps
        pr = idx.profile()
        return (ms, pr["split_codes"] // steps, pr["split6_codes"] // steps, pr["split_survivors"] // steps,
                pr["split5_codes"] // steps, pr["split5_survivors"] // steps,
                {k + "_per_step": int(pr[k] // steps) for k in ("nib_codes", "nib_survivors", "nib8_codes", "nib8_survivors")})

    # arms: (name, split_min_run, split6_min_run[, split5_min_run = 0]); parts 1 and 2 keep the 6-plane form off
    plan = [("min_run", int(1e9), [("off", OFF, 0), ("2Mi", 2 * MI, 0), ("8Mi", 8 * MI, 0), ("32Mi", 32 * MI, 0), ("128Mi", 128 * MI, 0)]),
            ("min_codes", int(1.6e7), [("off", OFF, 0), ("on", 8 * MI, 0)]),
            ("min_codes", int(4e7), [("off", OFF, 0), ("on", 8 * MI, 0)]),
            ("split6", int(1e9), [("off", 8 * MI, 0), ("8Mi", 8 * MI, 8 * MI), ("32Mi", 8 * MI, 32 * MI), ("128Mi", 8 * MI, 128 * MI),
                                  ("512Mi", 8 * MI, 512 * MI)]),
            ("split5", int(1e9), [("off", 8 * MI, 32 * MI, 0), ("8Mi", 8 * MI, 32 * MI, 8 * MI), ("32Mi", 8 * MI, 32 * MI, 32 * MI),
                                  ("128Mi", 8 * MI, 32 * MI, 128 * MI), ("400Mi", 8 * MI, 32 * MI, 400 * MI)])]
    # arms of the nibble part: (name, split_min_run, split6_min_run, split5_min_run, (nib_min_run, nib8_min_run, ns))
    nib_arms = [("off", 8 * MI, 32 * MI, 32 * MI, (0, 0, 9))]
    for ns in (9, 10):
        for thr in (32, 128, 400):
            nib_arms.append(("ns%d@%d" % (ns, thr), 8 * MI, 32 * MI, 32 * MI, (thr * MI, 0, ns)))
            nib_arms += [("ns%d@%d+8@%d" % (ns, thr, t8), 8 * MI, 32 * MI, 32 * MI, (thr * MI, t8 * MI, ns)) for t8 in (128, 400) if t8 > thr]
    nib_arms.append(("ns8@32", 8 * MI, 32 * MI, 32 * MI, (0, 32 * MI, 9)))
    plan.append(("nib", int(1e9), nib_arms))
    only = sys.argv[2] if len(sys.argv) > 2 else None
    for part, n, arms in plan:
        if only and part != only:
            continue
        idx = pyqadc.Index(M, 0)
        idx.set_split(1, OFF)                                  # build the copy whatever the list's size
        if part == "nib":
            idx.set_split_nib(1, 0, 9)                         # ... and the nibble-plane copy
        idx.add_partition_synthetic_shard(n, 0, n, bench.SEED, max(1, int(np.float32(n) * np.float32(bench.KEEP))))
        idx.finalize(bench.KEEP)
        idx.set_option("profile", 1)
        bench.set_mode(idx, bench.MODE_ONE_QUERY_PER_PASS)
        copy_bytes = idx.profile()["split_copy_bytes"]
        nib_copy_bytes = idx.profile()["nib_copy_bytes"]
        for rep in range(reps):
            order = arms if rep % 2 == 0 else arms[::-1]       # alternate the order: no arm always follows the same one
            for name, min_run, min_run6, *rest in order:
                ms, sc, sc6, surv, sc5, surv5, nib = measure(idx, 1, min_run, min_run6, rest[0] if rest else 0,
                                                             rest[1] if len(rest) > 1 else (0, 0, 9))
                print(json.dumps({"part": part, "codes": n, "round": rep, "arm": name, "ms_per_step": round(ms, 4),
                                  "codes_per_s": round(n * nq / ms * 1e3, 1), "split_codes_per_step": int(sc),
                                  "split6_codes_per_step": int(sc6), "split_survivors_per_step": int(surv),
                                  "split5_codes_per_step": int(sc5), "split5_survivors_per_step": int(surv5),
                                  "copy_bytes": int(copy_bytes), "nib_copy_bytes": int(nib_copy_bytes), **nib}), flush=True)
        idx.close()


if __name__ == "__main__":
    main()
