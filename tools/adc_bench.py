"""Float-ADC engine for whole-byte PQ codes (pyqadc.AdcIndex, the GPU scanner_simple) on its reference shapes, with the
single-thread CPU scan_standard<uint8_t, 8> of the same box in the same run.  Prints one line per leg and one JSON line.

  python tools/adc_bench.py [--legs flat1e8,batch32,lone1e6,ivf,cpu,ivf_search,lone_search,add,remove,train,opq,seed,filter,qfilter,refine,range,keyed,knn,decode,refine_sq,refine_range,probe,refine_ip] [--iters N] [--out FILE]
  python tools/adc_bench.py --bits 4 [--legs lone,ivf_search,add,remove,train,opq,seed,filter] [--iters N] [--out FILE]
  python tools/adc_bench.py --bits 16 [--legs lone,ivf_search,encode16,add,remove,train,seed,filter] [--iters N] [--out FILE]

  flat1e8   flat 8x8 list of 10^8 codes, one query per call: codes/s and its share of the 8 TB/s HBM roofline at 8 B per code
  batch32   32 queries per call on the same list
  lone1e6   the synchronous call-to-return time of one query on a 10^6-code flat list (SIFT1M shape)
  ivf       10^6 codes in K = 256 partitions, ma = 24, 1024 queries per call; the call includes the upload of the
            1024 x 24 float tables (8 KiB each).  With torch: alternated with query_scan_device on the same tables left in
            device memory (a torch tensor; heaps stay on the device), asserted equal
  cpu       the CPU scan_standard<uint8_t, 8> (the oracle's C restatement, and the reference's own build where it was
            compiled into oracle/_ref) on the 10^6-code list, one thread
  ivf_search   the ivf shape on real geometry: 10^6 clustered 128-d vectors encoded by adc_encode, K = 256, ma = 24, 1024 queries.
            Arm A = query_scan(assign, tables) with the assign and tables arm B's feeders produce (201 MB uploaded in the
            call); arm B = search(queries): coarse assignment and tables on the GPU.  The arms alternate in one process.
            Then arm B again (host finish) alternated with arm C = the same search() under set_finish(1), the device finish,
            asserted equal, and the same pair at 1, 8, 32, 128 and 1024 queries per call.
  lone_search  one synchronous search() of one query at that shape under the host finish and, alternated with it and asserted
            equal, under the device finish, beside one CPU thread scanning the same 24 partitions
  add       database build (not in the default legs; also under --bits 16, at 2x16): 10^6 clustered 128-d vectors, K = 256, 8x8.
            add_vectors, call to return, into an empty index and into one reserved to the final sizes, alternated in one process with
            the route without it: adc_encode (adc_encode16), the stable grouping by assign in numpy, add_partitions.  The partitions
            of the routes are asserted equal.  Under rocprofv3 --kernel-trace --stats the same leg gives the dispatch kernels' time
            beside the encoder's
  remove    remove by label (not in the default legs; also under --bits 4, on the 4-bit index itself at 16x4): 10^6 clustered 128-d
            vectors put into K = 256 partitions by add_vectors, 8x8.  remove_labels of a random 1 %, 10 % and 50 % of the labels, call
            to return, alternated in one process with the route without it: read_partition of every partition, np.isin on the host,
            add_partitions into a new index (on the 4-bit index without the finalize either route needs, and without the move into the
            arena only the route without the call needs).  Every arm starts from a fresh copy of the database, built outside the
            clock; the two routes' partitions are first asserted equal.  Then 10 % at K = 8: a few very long partitions, which the
            call compacts with one workgroup each
  train     learning the product quantizer (not in the default legs; also under --bits 4, at 16x4): 10^5 and 10^6 clustered 128-d
            vectors, 8x8, 10 rounds from a seed of 256 distinct rows (pyqadc.pq_seed).  train_pq, call to return (the upload of the
            learning set included), alternated in one process with the route without it: kmeans_iterations on every host slice.
            The two routes' codebooks and codes are first asserted equal bit for bit
  opq       learning the OPQ rotation (not in the default legs; also under --bits 4, at 16x4): 10^6 clustered
            128-d vectors, 8x8, train_opq(outer = 4, inner = 2) from the identity and a seed of distinct rows — ten k-means rounds with
            the closing ones — call to return, alternated in one process with the same loop composed from the public calls (train_pq
            with the rotation, opq_cross, procrustes: the learning set uploaded twice per outer round); the two routes' arrays are
            first asserted identical.  Beside it train_pq with ten rounds, and the reconstruction error
            (tests/pq_train_compose.reconstruction_error) of the learned pair against plain PQ's at those ten rounds
  --repair  the train and opq legs measure the empty-cluster repair instead (also under --bits 4 at 16x4 and
            --bits 16 at 2x16).  train: (a) on the leg's own 10^6 x 128 set (no empty cluster) the plain call and the repaired call,
            alternated in one process, and the time per round of each; with --parent-lib FILE a third arm alternates with them: the
            plain C call of that other build of the library (the parent commit's), loaded beside this one.  (b) the same set with
            REPAIR_DUP of its rows overwritten by copies of other rows and sub-space 0 zeroed on REPAIR_ZERO of the rows, seeded by
            pq_seed: empty, repaired, and the mean squared quantization error (pq_train_compose.reconstruction_error / n, the
            vectors re-encoded under the final codebooks by the index's own encoder) with and without the repair.  opq: train_opq
            with and without repair=True on set (b), times, empty and repaired
  seed      k-means++ seeding (not in the default legs; also under --bits 4 at 16x4 and --bits 16 at 2x16): 10^6
            clustered 128-d vectors; kmeans_seed per call at the index shape (and for K = 4096 coarse centroids at 8 bits), a round's
            time from the difference of a k and a k / 2 call and the bytes per second of its one pass over the learning set, one
            thread of the CPU twin per round, and the mean squared quantization error and the empty clusters after the train leg's
            rounds from kmeans_seed and from pq_seed.
  filter    filtered search (not in the default legs; also under --bits 4 at 16x4 and --bits 16 at 4x16, part (a) only; DESIGN.md
            section 11.10): (a) one synchronous query on 10^8 labelled codes (10^6 at --bits 4 and 16), unfiltered, EXCLUDE of 1 % and
            50 % of the keys, ALLOW of 1 % and 0.01 %, each checked against an index built without the dropped rows; (b) search() of
            1024 queries on the ivf_search database, unfiltered against EXCLUDE of 10 % of the keys, under both finishes; (c) the
            creation of a 10^6-key filter from host and from device memory.
  qfilter   one filter per query of a batch (not in the default legs), on the ivf_search database: 1024
            queries, K = 256, ma = 24, R = 100, every query assigned one of T distinct EXCLUDE filters, each of a random 10 % of the keys,
            T = 1, 16 and 1024.  Arm (a) = one search(filters=...) call; arm (b) = what there is without it: the batch grouped by
            filter, set_filter + search per group, the outputs scattered back.  The arms are asserted to return identical arrays and
            alternate in one process, under both finishes, with an unfiltered search() timed beside them for scale.
  range     range search (not in the default legs), on the ivf_search database: range_search() of the 1024
            queries with, per query, the radius that keeps about 100 rows (its own search() heap root at R = 100) and about 10^4 rows;
            the re-runs per call and the rows kept; beside it search() at R = 100 under both finishes and the route it replaces,
            search() at R = 65536 with a host threshold.
  refine    exact re-ranking (not in the default legs), on the ivf_search shape: recall@100 against exact
            float L2 of search() alone and of search_refined_device with r_in = 400 and 1000 over a float and a half store; the time
            of search_refined_device split into search_device and rerank_device; beside it a plain torch gather + (q - x)^2 sum +
            topk on the same candidates, the only yardstick there is.
  refine_sq SQ8 refine rows (not in the default legs), on the refine leg's shape, for f32, f16 and sq8 stores
            in the same run: recall@100 of search_refined_device (r_in 400 and 1000), rerank_device ms on the same candidates (three
            rounds of medians per store, taken in turn: the spread of the f16 figures is the yardstick's own), knn_device ms at 1024,
            32 and 1 queries, add_device rows/s, sq_range_device ms, the store's bytes and the clamp count.
  keyed     caller-chosen labels (not in the default legs), on the ivf_search / refine shape: rerank_device on a
            keyed store against the dense store holding the same vectors, alternated, at the refine leg's r_in values; put_device and
            remove_device rows/s at 10^6 keys, fresh and overwriting; add_vectors_device(labels=...) against the plain call.
  decode    PQ decode and reconstruction (not in the default legs; also under --bits 4 at 16x4 and --bits 16 at 2x16; DESIGN.md section
            11.19), dim 128, with and without a rotation: pq_decode_device on 10^6 codes, and reconstruct_device on the keys of a
            1024 x 100 search, each alternated with the route it replaces (read_partition, numpy gather and matmul, upload)
  probe     probed exact search (not in the default legs), on the ivf_search database (10^6 x 128-d rows,
            K = 256, ma = 24, R = 100) with batches of 1024, 32 and 1 queries, in one process: AdcIndex.search_exact_device beside
            Refine.knn_device on the same store (the baseline: every row) and search_refined_device at r_in = 1000; recall@100 against
            knn of the probed exact result (the coarse quantizer's loss alone) and of search_refined at r_in 400 and 1000.
  refine_ip the inner-product metric of a refine store (not in the default legs): 10^6 x 128-d rows, R = 100, f32,
            f16 and sq8 stores; knn_device at 1024, 32 and 1 queries, rerank_device at r_in 400 and 1000 and search_exact_device at K = 256,
            ma = 24, each under "ip" and under "l2" on the same store in the same process, 3 + 3 alternated runs; the reference is the L2 call
            of the same build and the margin its own run-to-run spread; beside them the share of keys knn under "ip" has in common with
            torch's (q @ x.T).topk (other arithmetic: a sanity figure)
  knn       exhaustive search over a refine store (not in the default legs): Refine.knn_device and Refine.knn
            on 10^6 rows of dim 128, float and half store, nq = 1, 32 and 1024, R = 100, from call to return, as pairs/s and as a share
            of the estimated roof of 2 x 10^11 pairs/s (3 dim component operations a pair at 32 packed non-FMA float operations per
            clock and SIMD — derived, not measured); beside it, in the same process, the route the benchmarks use for ground truth today,
            a chunked torch |x|^2 - 2 q.x and topk, and the share of queries whose key sets agree (other arithmetic: not asserted).
  --trained-codebooks   the add, remove and ivf_search legs (8 and 4 bits) learn their codebooks with train_pq (10 rounds on the
            residuals of the first 10^5 vectors) instead of sampling them; off by default, so that recorded figures stay comparable
  --bits 4   the float-ADC view of a 4-bit index instead (pyqadc.AdcIndex.view_of; legs lone,ivf_search):
  lone      one synchronous query on 10^6 and on 10^8 codes at 16x4 and 32x4: median and range of the call, codes/s, the share
            of the HBM roofline at 8 B / 16 B per code; at 16x4 alternated with the 8x8 engine on a list of the same n (the
            same bytes per code); beside one CPU thread on scan_4<M> over the 10^6 list (the reference's build where
            oracle/_ref has it, and the C restatement)
  ivf_search   10^6 clustered 128-d vectors encoded at 16x4 by ivf_encode, K = 256, ma = 24, 1024 queries: search() on the view
            under the host and the device finish, alternated and asserted equal
  add       not in the default legs: the database build of the 4-bit index itself (pyqadc.Index, 16x4) at the shape of the 8-bit `add`
            leg: ivf_encode + the stable grouping in numpy + add_partitions, alternated in one process with Index.add_vectors into
            an empty index and into one reserved to the final sizes; every arm is a whole build from an index with its quantizers
            set, and the three are first asserted to leave equal partitions
  profile   not timed: five one-query calls on 10^8 codes through the 16x4 view, the 32x4 view and the 8x8 engine, in that order —
            the workload of the rocprofv3 kernel-trace and LDS-counter runs (run it under rocprofv3, one kind of collection per run)
  --bits 16  the engine on 16-bit codes instead (pyqadc.AdcIndex.create16; legs lone,ivf_search), tables read from global memory:
  lone      one synchronous query on 10^6 and on 10^8 codes at 2x16, 4x16 and 8x16: median and range of the call, codes/s, the share
            of the HBM roofline at 4 / 8 / 16 B per code, each alternated with the 8-bit engine at the same bytes per code (4x8,
            8x8, 16x8) on a list of the same n; beside one CPU thread of the host twin's scan_standard<uint16_t, N> over the 10^6
            list (tests/cpp/scan_standard16_host.cpp: a port, not the reference's build)
  ivf_search   10^6 random codes in K = 256 partitions, random codebooks (128-d) and coarse centroids, ma = 24, 1024 queries:
            search() per shape (the tables, 0.5 / 1 / 2 MiB per (query, probe), are built and scanned in passes of the 1 GiB table
            budget), alternated with the 8-bit engine of the same bytes per code on the same partitions' sizes
            Then, per shape, the same search() on a database made by adc_encode16: 10^6 clustered 128-d vectors, K = 256 k-means
            centroids, codebooks = 65536 sampled residuals; with recall@100 of the first 64 queries against exact float L2
  encode16  adc_encode16 (host to host, flat) of 10^5 and 10^6 clustered 128-d vectors at 2x16, 4x16 and 8x16, codebooks = 65536
            sampled vectors: seconds per call, vectors/s, the share of the packed-VALU roof (2 n dim 65536 unfused multiplies and
            adds at 78.6e12 per second: half the 157.3 TFLOPS vector peak, which counts a fused multiply-add as two); beside one
            CPU thread of the host twin's pq_bytes::encode (tools/encode16_host_twin.cpp: a port, not the reference's build) timed
            on 256 of the vectors and EXTRAPOLATED to n, its codes asserted equal to the GPU's
  train     learning 16-bit sub-quantizers (not in the default legs): 10^6 clustered 128-d vectors at 2x16, 4x16 and 8x16, 2 rounds from
            a seed of 65536 distinct rows (pyqadc.pq_seed).  train_pq16, call to return (the upload of the learning set included),
            alternated in one process with the route without it: kmeans_iterations on every host slice (8.6 GB of distance scratch
            at 65536 centroids); the two routes' codebooks and codes are first asserted equal bit for bit.  Where that route cannot
            get its scratch the leg says so and times one CPU thread of the host twin (tests/cpp/pq_train16_host.cpp) on 256 vectors,
            EXTRAPOLATED to n.  A round's time is the difference of a 4-round and a 2-round call; beside it one adc_encode16 call on
            the same vectors (its upload included), which bounds the share of a round spent outside the encoder from below.  Under
            rocprofv3 --kernel-trace --stats the leg `train_profile` (one 2-round call per shape, not timed) gives the kernels' own share
  remove    the 8-bit `remove` leg on an index of 16-bit codes at 2x16 (not in the default legs)
  --trained-codebooks   the 16-bit add, remove and ivf_search (encoded database) legs learn their codebooks with train_pq16: 10 rounds
            on the residuals of the first min(n, 10^6) vectors, seeded with 65536 sampled residuals
  profile   not timed: five one-query calls on 10^8 codes at 8x16, then two search() calls of 64 queries at the ivf_search shape —
            the workload of a rocprofv3 --pmc run for the scan kernel's L2 hit rate (TCC_HIT_sum, TCC_MISS_sum)
Every time is a host clock around whole synchronous calls (median of --iters after warm-up); R = 100, sum_mode 1."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "quick-adc_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import pyqadc  # noqa: E402

HBM_BPS = 8e12
R = 100


def tables_for(rng, nq, ma, nsq=8):
    return ((rng.random((nq, ma, nsq * 256), dtype=np.float32) * np.float32(4.0)) ** 2).astype(np.float32)


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def alternated(fa, fb, iters, warmup=2):
    """medians of two arms timed in turn, A B A B ..., after a warm-up of each"""
    for _ in range(warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(iters):
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
    return float(np.median(ta)), float(np.median(tb))


def with_finish(idx, mode, fn):
    """fn() under finish `mode`, the default (host) restored"""
    def run():
        idx.set_finish(mode)
        try:
            return fn()
        finally:
            idx.set_finish(0)
    return run


def same_heaps(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a[:3], b[:3]))


def search_legs(legs, iters, res):
    """10^6 clustered vectors, encoded and partitioned on the GPU: the feeders of search() against caller-made tables"""
    rng = np.random.default_rng(1)
    n, dim, nsq, K, ma, nq = 1_000_000, 128, 8, 256, 24, 1024
    centers = (rng.normal(size=(2000, dim)) * 3).astype(np.float32)
    vectors = centers[rng.integers(0, len(centers), n)]
    vectors += rng.normal(size=(n, dim)).astype(np.float32)
    queries = (centers[rng.integers(0, len(centers), nq)] + rng.normal(size=(nq, dim))).astype(np.float32)
    coarse, _ = pyqadc.kmeans_iterations(vectors[:100000], vectors[rng.choice(n, K, replace=False)], 5)
    sample = vectors[rng.choice(n, 256, replace=False)]
    near = pyqadc.coarse_assign(sample, coarse, 1)[:, 0]
    codebooks = np.ascontiguousarray((sample - coarse[near]).reshape(256, nsq, dim // nsq).transpose(1, 0, 2), np.float32)
    if TRAINED:
        codebooks = trained_codebooks(vectors, coarse, nsq, 8, rng)
    t0 = time.perf_counter()
    part_of, codes = pyqadc.adc_encode(codebooks, vectors, coarse)
    res["adc_encode_1e6_s"] = time.perf_counter() - t0
    print("adc_encode of 10^6 128-d vectors (K = 256, 8x8), host to host: %.2f s" % res["adc_encode_1e6_s"], flush=True)
    if "refine" not in legs and "keyed" not in legs and "refine_sq" not in legs and "refine_range" not in legs and "probe" not in legs:
        del vectors
    order = np.argsort(part_of, kind="stable")
    bounds = np.searchsorted(part_of[order], np.arange(K + 1))
    parts = [codes[order[bounds[k]:bounds[k + 1]]] for k in range(K)]
    labels = [order[bounds[k]:bounds[k + 1]].astype(np.uint32) for k in range(K)]
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.add_partitions(parts, labels)
    idx.set_pq(codebooks)
    idx.set_coarse(coarse)
    if "ivf_search" in legs:
        assign, tables = idx.search_tables(queries, ma)
        got_a = idx.query_scan(assign, tables, R)
        got_b = idx.search(queries, ma, R)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got_a, got_b[:3])), "the arms disagree"
        med_a, med_b = alternated(lambda: idx.query_scan(assign, tables, R), lambda: idx.search(queries, ma, R), max(5, iters))
        res["ivf_search_arm_a_query_scan_ms"] = med_a * 1e3
        res["ivf_search_arm_b_search_ms"] = med_b * 1e3
        res["ivf_search_b_over_a"] = med_b / med_a
        res["ivf_search_table_bytes"] = int(tables.nbytes)
        res["ivf_search_codes_probed_per_call"] = int(sum(len(parts[k]) for k in assign.ravel()))
        print("IVF on encoded vectors, K=256 ma=24, 1024 queries/call: A query_scan(assign, tables) with %.0f MB uploaded %.2f ms;"
              " B search(queries) %.2f ms = %.1f us/query; B / A = %.3f"
              % (tables.nbytes / 1e6, med_a * 1e3, med_b * 1e3, med_b * 1e6 / nq, med_b / med_a), flush=True)
        sweep = {}
        for n in (1, 8, 32, 128, nq):
            qs = queries[:n]
            host = lambda: idx.search(qs, ma, R)
            dev = with_finish(idx, 1, host)
            assert same_heaps(host(), dev()), "host and device finish disagree at %d queries" % n
            med_h, med_d = alternated(host, dev, max(5, iters) if n == nq else max(20, iters))
            sweep[str(n)] = [med_h * 1e3, med_d * 1e3]
            print("search() of %d queries: host finish %.3f ms, device finish %.3f ms (device / host = %.3f)"
                  % (n, med_h * 1e3, med_d * 1e3, med_d / med_h), flush=True)
        res["ivf_search_host_finish_ms"] = sweep[str(nq)][0]
        res["ivf_search_device_finish_ms"] = sweep[str(nq)][1]
        res["ivf_search_device_over_host_finish"] = sweep[str(nq)][1] / sweep[str(nq)][0]
        res["ivf_search_finish_sweep_ms_host_device"] = sweep
        res["ivf_search_host_finishes"] = int(idx.host_finishes())
    if "refine" in legs:
        refine_leg(idx, vectors, queries, ma, iters, res)
    if "keyed" in legs:
        keyed_leg(idx, vectors, queries, ma, iters, res, codebooks, coarse)
    if "refine_sq" in legs:
        refine_sq_leg(idx, vectors, queries, ma, iters, res)
    if "refine_range" in legs:
        refine_range_search_leg(idx, vectors, queries, ma, iters, res)
    if "probe" in legs:
        probe_leg(idx, vectors, queries, ma, iters, res)
    if "refine" in legs or "keyed" in legs or "refine_sq" in legs or "refine_range" in legs or "probe" in legs:
        del vectors
    if "filter" in legs:   # (b): the same search() without a filter and with 10 % of the keys excluded, in turn, under both finishes
        S = rng.permutation(n)[:n // 10].astype(np.uint32)
        keep = ~np.isin(np.arange(n), S)
        ref = pyqadc.AdcIndex(nsq, 8)
        ref.add_partitions([p[keep[l]] for p, l in zip(parts, labels)], [l[keep[l]] for l in labels])
        ref.set_pq(codebooks)
        ref.set_coarse(coarse)
        f = pyqadc.AdcFilter(S, "exclude")
        plain = lambda: idx.search(queries, ma, R)

        def masked():
            idx.set_filter(f)
            try:
                return idx.search(queries, ma, R)
            finally:
                idx.set_filter(None)
        for finish in (0, 1):
            same = same_heaps(with_finish(idx, finish, masked)(), with_finish(ref, finish, lambda: ref.search(queries, ma, R))())
            med_p, med_f = alternated(with_finish(idx, finish, plain), with_finish(idx, finish, masked), max(5, iters))
            tag = "filter_ivf_search_%s_finish" % ("device" if finish else "host")
            res[tag + "_unfiltered_ms"] = med_p * 1e3
            res[tag + "_exclude10_ms"] = med_f * 1e3
            res[tag + "_same_heaps"] = bool(same)
            print("search() of 1024 queries, K=256 ma=24 on 10^6 codes, %s finish, alternated: unfiltered %.2f ms, EXCLUDE of 10 %% of the "
                  "keys %.2f ms (filtered / unfiltered = %.3f); same heaps as an index without the rows: %s"
                  % ("device" if finish else "host", med_p * 1e3, med_f * 1e3, med_f / med_p, same), flush=True)
        ref.close()
        f.close()
    if "qfilter" in legs:
        qfilter_leg(idx, len(part_of), queries, ma, iters, res, rng)
    if "range" in legs:
        range_leg(idx, queries, ma, iters, res)
    if "lone_search" in legs:
        q1 = queries[:1]
        med, best = timed(lambda: idx.search(q1, ma, R), max(iters, 50), warmup=5)
        res["lone_search_call_us"] = med * 1e6
        print("one synchronous search() of one query, K=256 ma=24 on 10^6 codes: %.1f us (best %.1f)" % (med * 1e6, best * 1e6), flush=True)
        host = lambda: idx.search(q1, ma, R)
        dev = with_finish(idx, 1, host)
        assert same_heaps(host(), dev()), "host and device finish disagree on the lone query"
        med_h, med_d = alternated(host, dev, max(iters, 50), warmup=5)
        res["lone_search_host_finish_us"] = med_h * 1e6
        res["lone_search_device_finish_us"] = med_d * 1e6
        print("the same alternated: host finish %.1f us, device finish %.1f us" % (med_h * 1e6, med_d * 1e6), flush=True)
        import pyoracle as po
        a1, t1 = idx.search_tables(q1, ma)
        pp, ll = [parts[k] for k in a1[0]], [labels[k] for k in a1[0]]
        scan = po.reff_scan_standard_u8 if po.have_ref_float() else po.scan_standard_u8
        med_c, _ = timed(lambda: scan(nsq, pp, ll, t1[0], R), 20, warmup=2)
        res["lone_search_cpu_scan_24_partitions_us"] = med_c * 1e6
        res["lone_search_codes_probed"] = int(sum(len(p) for p in pp))
        print("CPU scan_standard<uint8_t,8> over the same 24 partitions (%d codes), 1 thread, tables given (%s): %.1f us"
              % (res["lone_search_codes_probed"], "reference build" if po.have_ref_float() else "C restatement", med_c * 1e6), flush=True)
    idx.close()


def range_leg(idx, queries, ma, iters, res):
    """range_search() against the top-R calls it stands beside, in one process: each query's radius is the largest value of its own
    search() heap at R = rows, so it keeps about `rows` rows (rows 100: the short segments sorted in LDS; 10^4: the radix passes)"""
    nq = len(queries)
    flt_max = np.float32(np.finfo(np.float32).max)
    for rows in (100, 10000):
        _, v, _, _ = idx.search(queries, ma, rows)
        radius = np.ascontiguousarray(v.max(axis=1), np.float32)                 # the heap's root (FLT_MAX where fewer rows were probed)
        before = idx.reruns()
        lims, keys, vals = idx.range_search(queries, ma, radius)
        reruns = int(idx.reruns() - before)
        sizes = np.diff(lims)
        full = radius < flt_max
        assert (sizes[full] <= rows - 1).all() and (vals < np.repeat(radius, sizes)).all(), "a query keeps a row at or beyond its radius"
        med, best = timed(lambda: idx.range_search(queries, ma, radius), max(5, iters))
        tag = "range_%d" % rows
        res[tag + "_range_search_ms"] = med * 1e3
        res[tag + "_range_search_best_ms"] = best * 1e3
        res[tag + "_reruns_per_call"] = reruns
        res[tag + "_rows_min_median_max_total"] = [int(sizes.min()), float(np.median(sizes)), int(sizes.max()), int(sizes.sum())]
        print("range_search() of %d queries, K=256 ma=%d on 10^6 codes, radius = the query's own R=%d heap root: %.2f ms (best %.2f), %d re-run(s) "
              "per call, rows per query min %d median %.0f max %d, %d in all"
              % (nq, ma, rows, med * 1e3, best * 1e3, reruns, sizes.min(), np.median(sizes), sizes.max(), sizes.sum()), flush=True)
        if rows == 100:
            host = lambda: idx.search(queries, ma, 100)
            med_h, med_d = alternated(host, with_finish(idx, 1, host), max(5, iters))
            res["range_search_R100_host_finish_ms"] = med_h * 1e3
            res["range_search_R100_device_finish_ms"] = med_d * 1e3
            print("search() at R = 100 beside it: host finish %.2f ms, device finish %.2f ms" % (med_h * 1e3, med_d * 1e3), flush=True)

            def replaced():                                                     # the route range_search replaces: the widest heap, cut on the host
                k, vv, _, _ = idx.search(queries, ma, 65536)
                keep = vv < radius[:, None]
                return k[keep], vv[keep], keep.sum(axis=1)
            got = replaced()
            med_r, best_r = timed(replaced, max(3, iters // 3), warmup=0)
            res["range_100_search_R65536_threshold_ms"] = med_r * 1e3
            res["range_100_search_R65536_threshold_same_counts"] = bool(np.array_equal(got[2], sizes))
            print("search() at R = 65536 and a host threshold at the same radii: %.1f ms (best %.1f); same row counts as range_search: %s"
                  % (med_r * 1e3, best_r * 1e3, res["range_100_search_R65536_threshold_same_counts"]), flush=True)


def qfilter_leg(idx, n, queries, ma, iters, res, rng):
    """one search(filters=...) call against the batch grouped by filter, T distinct filters over the 1024 queries"""
    nq = len(queries)
    it = max(5, iters)
    for T in (1, 16, 1024):
        made = [pyqadc.AdcFilter(rng.permutation(n)[:n // 10].astype(np.uint32), "exclude") for _ in range(T)]
        of_query = rng.integers(0, T, nq) if T < nq else rng.permutation(nq)                  # T = nq: one filter per query
        groups = [np.flatnonzero(of_query == t) for t in range(T)]
        filters = [made[t] for t in of_query]

        def one_call():
            return idx.search(queries, ma, R, filters=filters)

        def grouped():
            out = None
            try:
                for t, rows in enumerate(groups):
                    if not len(rows):
                        continue
                    idx.set_filter(made[t])
                    got = idx.search(queries[rows], ma, R)
                    if out is None:
                        out = [np.zeros((nq,) + g.shape[1:], g.dtype) for g in got]
                    for o, g in zip(out, got):
                        o[rows] = g
            finally:
                idx.set_filter(None)
            return out

        for finish in (0, 1):
            name = "device" if finish else "host"
            a, b = with_finish(idx, finish, one_call), with_finish(idx, finish, grouped)
            got_a, got_b = a(), b()
            assert same_heaps(got_a, got_b) and np.array_equal(got_a[3], got_b[3]), "T = %d, %s finish: the arms disagree" % (T, name)
            ta, tb, tp = [], [], []
            plain = with_finish(idx, finish, lambda: idx.search(queries, ma, R))
            plain()
            for _ in range(it):                                                                   # (both arms ran once above: the warm-up)
                for f, ts in ((a, ta), (b, tb), (plain, tp)):
                    t0 = time.perf_counter()
                    f()
                    ts.append(time.perf_counter() - t0)
            tag = "qfilter_T%d_%s_finish" % (T, name)
            for arm, ts in (("one_call", ta), ("grouped", tb), ("unfiltered", tp)):
                res["%s_%s_ms_median_min_max" % (tag, arm)] = [float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, float(np.max(ts)) * 1e3]
            res[tag + "_grouped_over_one_call"] = float(np.median(tb) / np.median(ta))
            print("search() of %d queries under %d distinct EXCLUDE filters of 10 %% of the keys, %s finish, %d alternations: one call with "
                  "filters= %.2f ms (%.2f .. %.2f); grouped by filter %.2f ms (%.2f .. %.2f), grouped / one call = %.2f; unfiltered %.2f ms; "
                  "identical arrays" % (nq, T, name, it, np.median(ta) * 1e3, min(ta) * 1e3, max(ta) * 1e3, np.median(tb) * 1e3, min(tb) * 1e3,
                                        max(tb) * 1e3, np.median(tb) / np.median(ta), np.median(tp) * 1e3), flush=True)
        res["qfilter_T%d_bitmap_bytes_in_all" % T] = int(sum(f.info()["bitmap_bytes"] for f in made))
        for f in made:
            f.close()


def refine_leg(idx, vectors, queries, ma, iters, res):
    """search, then exact re-ranking on the GPU (pyqadc.Refine): what it buys in recall and what it costs"""
    import torch
    dev = torch.device("cuda", 0)
    n, dim = vectors.shape
    nq = len(queries)
    tq = torch.from_numpy(queries).to(dev)
    tx = torch.from_numpy(vectors).to(dev)
    # ground truth: the R nearest by float L2 (||x||^2 - 2 q.x in chunks; the query's own norm does not change the order)
    best_d = torch.full((nq, R), float("inf"), device=dev)
    best_k = torch.zeros((nq, R), dtype=torch.int64, device=dev)
    for first in range(0, n, 1 << 17):
        x = tx[first:first + (1 << 17)]
        d = (x * x).sum(1)[None, :] - 2.0 * (tq @ x.T)
        cd, ck = torch.cat([best_d, d], 1).topk(R, dim=1, largest=False)
        best_k = torch.cat([best_k, torch.arange(first, first + len(x), device=dev).expand(nq, -1)], 1).gather(1, ck)
        best_d = cd
    truth = best_k.cpu().numpy()

    def recall(keys):
        return float(np.mean([len(set(truth[q].tolist()) & set(np.asarray(keys[q]).tolist())) for q in range(nq)])) / R

    plain = idx.search(queries, ma, R)
    res["refine_recall_plain"] = recall(plain[0])
    print("recall@%d of search() alone: %.4f" % (R, res["refine_recall_plain"]), flush=True)
    for dtype in ("f32", "f16"):
        st = pyqadc.Refine(dim, dtype)
        st.add_device(tx)
        for r_in in (400, 1000):
            keys, dist, sizes, missing = idx.search_refined_device(tq, ma, R, r_in, st)
            assert missing == 0
            tag = "refine_%s_rin%d" % (dtype, r_in)
            res[tag + "_recall"] = recall(keys.cpu().numpy().view(np.uint32))
            ck, cv, _ = idx.search_device(tq, ma, r_in)
            t_search, _ = timed(lambda: idx.search_device(tq, ma, r_in), max(5, iters))
            t_rerank, _ = timed(lambda: st.rerank_device(tq, ck, R, values=cv), max(5, iters))
            t_both, _ = timed(lambda: idx.search_refined_device(tq, ma, R, r_in, st), max(5, iters))
            rows = tx if dtype == "f32" else tx.half()
            ckl = ck.long() & 0xFFFFFFFF

            def yardstick():
                x = rows[ckl].float()                                       # gather [nq][r_in][dim]
                d = ((tq[:, None, :] - x) ** 2).sum(-1)
                d = torch.where(cv == 3.4028234663852886e38, torch.full_like(d, float("inf")), d)
                out = d.topk(R, dim=1, largest=False)
                torch.cuda.synchronize()
                return out
            t_torch, _ = timed(yardstick, max(5, iters))
            res[tag + "_search_ms"], res[tag + "_rerank_ms"] = t_search * 1e3, t_rerank * 1e3
            res[tag + "_search_refined_ms"], res[tag + "_torch_gather_topk_ms"] = t_both * 1e3, t_torch * 1e3
            res[tag + "_gather_bytes"] = int(nq) * r_in * dim * (4 if dtype == "f32" else 2)
            print("%s store, r_in %d: recall@%d %.4f; search_device %.3f ms + rerank_device %.3f ms (search_refined_device %.3f ms); torch "
                  "gather + topk on the same candidates %.3f ms; %.0f MB gathered = %.2f TB/s in the rerank"
                  % (dtype, r_in, R, res[tag + "_recall"], t_search * 1e3, t_rerank * 1e3, t_both * 1e3, t_torch * 1e3,
                     res[tag + "_gather_bytes"] / 1e6, res[tag + "_gather_bytes"] / t_rerank / 1e12), flush=True)
        st.close()


def probe_leg(idx, vectors, queries, ma, iters, res):
    """exact search over the probed partitions beside the exhaustive search and the re-ranked PQ search"""
    import torch
    dev = torch.device("cuda", 0)
    n, dim = vectors.shape
    tx = torch.from_numpy(vectors).to(dev)
    out = res.setdefault("probe", {"rows": n, "dim": dim, "K": idx.partition_count(), "ma": ma, "R": R})
    for dtype in ("f32", "f16"):
        st = pyqadc.Refine(dim, dtype)
        st.add_device(tx)
        for nq in (1024, 32, 1):
            tq = torch.from_numpy(queries[:nq]).to(dev)
            truth = st.knn_device(tq, R)[0].cpu().numpy().view(np.uint32)

            def recall(keys):
                keys = keys.cpu().numpy().view(np.uint32)
                return float(np.mean([len(set(truth[q].tolist()) & set(keys[q].tolist())) for q in range(nq)])) / R
            keys, _, _, missing, assign = idx.search_exact_device(tq, ma, R, st)
            assert missing == 0
            probed_rows = float(np.mean([sum(idx.partition_size(int(p)) for p in row) for row in assign.cpu().numpy()]))
            its = max(5, iters)
            t_exact, best_exact = timed(lambda: idx.search_exact_device(tq, ma, R, st), its)
            t_knn, best_knn = timed(lambda: st.knn_device(tq, R), its)
            t_ref, _ = timed(lambda: idx.search_refined_device(tq, ma, R, 1000, st), its)
            t_assign, _ = timed(lambda: idx.assign_device(tq, ma), its)
            row = {"search_exact_device_ms": t_exact * 1e3, "search_exact_device_best_ms": best_exact * 1e3, "knn_device_ms": t_knn * 1e3,
                   "knn_device_best_ms": best_knn * 1e3, "search_refined_device_rin1000_ms": t_ref * 1e3, "assign_device_ms": t_assign * 1e3,
                   "rows_probed_per_query": probed_rows, "share_of_rows_probed": probed_rows / n, "recall_probed_exact": recall(keys),
                   "recall_search_refined_rin400": recall(idx.search_refined_device(tq, ma, R, 400, st)[0]),
                   "recall_search_refined_rin1000": recall(idx.search_refined_device(tq, ma, R, 1000, st)[0])}
            out["%s_nq%d" % (dtype, nq)] = row
            print("probe %s, 10^6 x %d, K %d, ma %d, nq %4d, R %d: search_exact_device %.3f ms (best %.3f; assign alone %.3f) over %.1f %% of the "
                  "rows; knn_device %.3f ms (best %.3f); search_refined_device(r_in 1000) %.3f ms; recall@%d against knn: probed exact %.4f, "
                  "search_refined r_in 400 %.4f, r_in 1000 %.4f"
                  % (dtype, dim, out["K"], ma, nq, R, t_exact * 1e3, best_exact * 1e3, t_assign * 1e3, 100 * probed_rows / n, t_knn * 1e3,
                     best_knn * 1e3, t_ref * 1e3, R, row["recall_probed_exact"], row["recall_search_refined_rin400"],
                     row["recall_search_refined_rin1000"]), flush=True)
        st.close()


def refine_sq_leg(idx, vectors, queries, ma, iters, res):
    """SQ8 refine rows beside float and half rows in one run: recall, rerank and knn time, fill rate, bytes"""
    import torch
    dev = torch.device("cuda", 0)
    n, dim = vectors.shape
    nq = len(queries)
    tq = torch.from_numpy(queries).to(dev)
    tx = torch.from_numpy(vectors).to(dev)
    best_d = torch.full((nq, R), float("inf"), device=dev)
    best_k = torch.zeros((nq, R), dtype=torch.int64, device=dev)
    for first in range(0, n, 1 << 17):                                          # ground truth as in refine_leg: float L2
        x = tx[first:first + (1 << 17)]
        d = (x * x).sum(1)[None, :] - 2.0 * (tq @ x.T)
        cd, ck = torch.cat([best_d, d], 1).topk(R, dim=1, largest=False)
        best_k = torch.cat([best_k, torch.arange(first, first + len(x), device=dev).expand(nq, -1)], 1).gather(1, ck)
        best_d = cd
    truth = best_k.cpu().numpy()

    def recall(keys):
        return float(np.mean([len(set(truth[q].tolist()) & set(np.asarray(keys[q]).tolist())) for q in range(nq)])) / R

    t_range, _ = timed(lambda: pyqadc.refine_sq_range_device(tx), max(5, iters))
    vmin, step = pyqadc.refine_sq_range_device(tx)
    res["refine_sq_range_device_ms"] = t_range * 1e3
    print("sq_range_device of %d x %d floats: %.3f ms = %.2f TB/s" % (n, dim, t_range * 1e3, n * dim * 4 / t_range / 1e12), flush=True)
    dtypes = ("f32", "f16", "sq8")
    stores = {}
    for dtype in dtypes:
        def fill():
            st = pyqadc.Refine(dim, dtype, vmin=vmin, step=step) if dtype == "sq8" else pyqadc.Refine(dim, dtype)
            st.reserve(n)
            t0 = time.perf_counter()
            st.add_device(tx)
            return st, time.perf_counter() - t0
        fill()[0].close()                                                       # warm-up
        fills = [fill() for _ in range(3)]
        for st, _ in fills[1:]:
            st.close()
        stores[dtype] = fills[0][0]
        t_add = float(np.median([t for _, t in fills]))
        res["refine_sq_%s_add_device_rows_per_s" % dtype] = n / t_add
        res["refine_sq_%s_bytes" % dtype] = stores[dtype].info()["bytes"]
        print("%s store: add_device of %d rows %.3f ms = %.1f M rows/s; %d bytes" % (dtype, n, t_add * 1e3, n / t_add / 1e6,
                                                                                      stores[dtype].info()["bytes"]), flush=True)
    res["refine_sq_clamped"] = stores["sq8"].sq_info()["clamped"]
    print("sq8 store: %d of %d components clamped" % (res["refine_sq_clamped"], n * dim), flush=True)
    for r_in in (400, 1000):
        ck, cv, _ = idx.search_device(tq, ma, r_in)
        for dtype in dtypes:
            keys, _, _, missing = idx.search_refined_device(tq, ma, R, r_in, stores[dtype])
            assert missing == 0
            res["refine_sq_%s_rin%d_recall" % (dtype, r_in)] = recall(keys.cpu().numpy().view(np.uint32))
        rounds = {d: [] for d in dtypes}
        for _ in range(3):                                                      # rounds in turn: drift shows in every store alike
            for dtype in dtypes:
                rounds[dtype].append(timed(lambda: stores[dtype].rerank_device(tq, ck, R, values=cv), max(5, iters))[0] * 1e3)
        for dtype in dtypes:
            res["refine_sq_%s_rin%d_rerank_ms_rounds" % (dtype, r_in)] = rounds[dtype]
            print("%s store, r_in %d: recall@%d %.4f; rerank_device %s ms" % (dtype, r_in, R, res["refine_sq_%s_rin%d_recall" % (dtype, r_in)],
                                                                             ", ".join("%.3f" % t for t in rounds[dtype])), flush=True)
    for n_q in (1024, 32, 1):
        qs = tq[:n_q].contiguous()
        rounds = {d: [] for d in dtypes}
        for _ in range(3):
            for dtype in dtypes:
                rounds[dtype].append(timed(lambda: stores[dtype].knn_device(qs, R), max(5, iters))[0] * 1e3)
        for dtype in dtypes:
            res["refine_sq_%s_knn_device_nq%d_ms_rounds" % (dtype, n_q)] = rounds[dtype]
        print("knn_device, %d queries over %d rows: %s" % (n_q, n, "; ".join("%s %s ms" % (d, ", ".join("%.3f" % t for t in rounds[d]))
                                                                              for d in dtypes)), flush=True)
    for st in stores.values():
        st.close()


def keyed_leg(idx, vectors, queries, ma, iters, res, codebooks, coarse):
    """caller-chosen labels: what the keyed store's probe costs beside the dense store's range test, what
    put and remove sustain, and what a label array costs add_vectors"""
    import torch
    dev = torch.device("cuda", 0)
    n, dim = vectors.shape
    nq = len(queries)
    tq = torch.from_numpy(queries).to(dev)
    tx = torch.from_numpy(vectors).to(dev)
    positions = torch.arange(n, dtype=torch.int32, device=dev)                  # the index's keys are positions: both stores hold them
    rng = np.random.default_rng(7)
    # 1. the same vectors under the same keys in a dense and in a keyed store: rerank_device in turn
    for dtype in ("f32", "f16"):
        dense, keyed = pyqadc.Refine(dim, dtype), pyqadc.Refine(dim, dtype, keyed=True)
        dense.add_device(tx)
        keyed.put_device(tx, positions)
        info = keyed.keyed_info()
        res["keyed_%s_table_and_row_state_bytes_per_key" % dtype] = (12 * info["table_slots"] + 8 * info["rows_allocated"]) / info["live"]
        for r_in in (400, 1000):
            ck, cv, _ = idx.search_device(tq, ma, r_in)
            a, b = dense.rerank_device(tq, ck, R, values=cv), keyed.rerank_device(tq, ck, R, values=cv)
            assert a[3] == b[3] == 0 and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:3], b[:3])), "the stores disagree"
            t_dense, t_keyed = alternated(lambda: dense.rerank_device(tq, ck, R, values=cv), lambda: keyed.rerank_device(tq, ck, R, values=cv),
                                          max(10, iters))
            tag = "keyed_%s_rin%d" % (dtype, r_in)
            res[tag + "_dense_rerank_ms"], res[tag + "_keyed_rerank_ms"] = t_dense * 1e3, t_keyed * 1e3
            res[tag + "_keyed_over_dense"] = t_keyed / t_dense
            print("%s stores, r_in %d, rerank_device of %d queries, alternated: dense %.3f ms, keyed %.3f ms (keyed / dense = %.3f); table of %d "
                  "slots, %d used" % (dtype, r_in, nq, t_dense * 1e3, t_keyed * 1e3, t_keyed / t_dense, info["table_slots"], info["table_used"]),
                  flush=True)
        dense.close()
        keyed.close()
    # 2. put_device and remove_device at 10^6 keys drawn from all 32 bits
    sparse = np.unique(rng.integers(0, 0xFFFFFFFF, 2 * n, dtype=np.uint64).astype(np.uint32))
    tl = torch.from_numpy(rng.permutation(sparse)[:n].view(np.int32).copy()).to(dev)
    for dtype in ("f32", "f16"):
        fresh, reserved, over, gone, again = [], [], [], [], []
        for _ in range(max(3, iters // 3)):
            for bucket, reserve in ((fresh, False), (reserved, True)):
                st = pyqadc.Refine(dim, dtype, keyed=True)
                if reserve:
                    st.reserve(n)
                t0 = time.perf_counter()
                st.put_device(tx, tl)
                bucket.append(time.perf_counter() - t0)
                if not reserve:
                    st.close()
            t0 = time.perf_counter()
            st.put_device(tx, tl)                                               # every key is held: an overwrite
            over.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            removed = st.remove_device(tl)
            gone.append(time.perf_counter() - t0)
            assert removed == n
            t0 = time.perf_counter()
            st.put_device(tx, tl)                                               # into dead slots and freed rows
            again.append(time.perf_counter() - t0)
            st.close()
        for name, ts in (("put_fresh", fresh), ("put_reserved", reserved), ("put_overwrite", over), ("remove", gone), ("put_after_remove", again)):
            res["keyed_%s_%s_rows_per_s" % (dtype, name)] = n / float(np.median(ts))
        print("%s keyed store, 10^6 keys of dim %d in one call (device forms): put into an empty store %.3g rows/s, after reserve %.3g, overwriting "
              "%.3g, remove %.3g, put after the remove %.3g" % ((dtype, dim) + tuple(res["keyed_%s_%s_rows_per_s" % (dtype, k)] for k in
              ("put_fresh", "put_reserved", "put_overwrite", "remove", "put_after_remove"))), flush=True)
    # 3. add_vectors_device with a label array against the plain call
    def build(labels):
        ix = pyqadc.AdcIndex(idx.sq_count, 8)
        ix.set_pq(codebooks)
        ix.set_coarse(coarse)
        t0 = time.perf_counter()
        ix.add_vectors_device(tx, labels=labels)
        t = time.perf_counter() - t0
        ix.close()
        return t
    build(None), build(tl)
    plain, labelled = [], []
    for _ in range(max(3, iters // 3)):
        plain.append(build(None))
        labelled.append(build(tl))
    res["keyed_add_vectors_device_plain_s"], res["keyed_add_vectors_device_labelled_s"] = float(np.median(plain)), float(np.median(labelled))
    res["keyed_add_labelled_over_plain"] = res["keyed_add_vectors_device_labelled_s"] / res["keyed_add_vectors_device_plain_s"]
    print("add_vectors_device of 10^6 vectors into an empty index, alternated: plain %.3f s, labels=... %.3f s (labelled / plain = %.3f)"
          % (res["keyed_add_vectors_device_plain_s"], res["keyed_add_vectors_device_labelled_s"], res["keyed_add_labelled_over_plain"]), flush=True)


def filter_leg(bits, iters, res, torch=None):
    """(a) one synchronous query on labelled codes under key filters of several selectivities, each against an index built without
    the dropped rows; (c) (torch given) the creation of a 10^6-key filter from host and from device memory"""
    rng = np.random.default_rng(110)
    zero = np.zeros((1, 1), np.int32)
    n = 100_000_000 if bits == 8 else 1_000_000
    shape = {8: (8, 8), 4: (16, 4), 16: (4, 16)}[bits]
    nsq = shape[0]

    def build(codes, labels):
        if bits == 4:
            src = pyqadc.Index(nsq)
            src.add_partitions([codes], [labels])
            src.finalize(0.01)
            return pyqadc.AdcIndex.view_of(src), src
        idx = pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)
        idx.add_partitions([codes], [labels])
        return idx, None

    def close(pair):
        pair[0].close()
        if pair[1] is not None:
            pair[1].close()

    if bits == 16:
        codes = rng.integers(0, 65536, (n, nsq), dtype=np.uint16)
    else:
        codes = rng.integers(0, 256, (n, nsq if bits == 8 else nsq // 2), dtype=np.uint8)
    labels = ((np.arange(n, dtype=np.uint64) * np.uint64(1000003)) % np.uint64(n)).astype(np.uint32)   # a permutation of 0 .. n - 1
    tb = ((rng.random((1, 1, nsq << bits), dtype=np.float32) * np.float32(4.0)) ** 2).astype(np.float32)
    full = build(codes, labels)
    idx = full[0]
    it = iters if n > 1_000_000 else max(iters, 50)
    tag = "filter_lone_%dx%d_%.0e" % (nsq, bits, n)
    med0, lo0, hi0 = spread(lambda: idx.query_scan(zero, tb, R), it)
    res[tag + "_unfiltered_ms_median_min_max"] = [med0 * 1e3, lo0 * 1e3, hi0 * 1e3]
    print("%dx%d, %.0e labelled codes, one synchronous query, no filter: %.3f ms (%.3f .. %.3f)" % (nsq, bits, n, med0 * 1e3, lo0 * 1e3, hi0 * 1e3),
          flush=True)
    for mode, share in (("exclude", 0.01), ("exclude", 0.5), ("allow", 0.01), ("allow", 0.0001)):
        inside = rng.random(n) < share
        S = labels[inside]
        f = pyqadc.AdcFilter(S, mode)
        idx.set_filter(f)
        got = idx.query_scan(zero, tb, R)
        med, lo, hi = spread(lambda: idx.query_scan(zero, tb, R), it)
        med_u, med_f = alternated(lambda: (idx.set_filter(None), idx.query_scan(zero, tb, R)),
                                  lambda: (idx.set_filter(f), idx.query_scan(zero, tb, R)), it, warmup=2)
        idx.set_filter(None)
        keep = ~inside if mode == "exclude" else inside
        ref = build(codes[keep], labels[keep])
        same = same_heaps(got, ref[0].query_scan(zero, tb, R))
        close(ref)
        name = "%s_%s_%g_percent" % (tag, mode, share * 100)
        res[name + "_ms_median_min_max"] = [med * 1e3, lo * 1e3, hi * 1e3]
        res[name + "_alternated_unfiltered_filtered_ms"] = [med_u * 1e3, med_f * 1e3]
        res[name + "_keys"] = int(len(S))
        res[name + "_bitmap_bytes"] = f.info()["bitmap_bytes"]
        res[name + "_same_heaps"] = bool(same)
        print("  %s of %g %% of the keys (%d keys, bitmap %.1f MiB): %.3f ms (%.3f .. %.3f); alternated with no filter: %.3f against %.3f ms "
              "(filtered / unfiltered = %.3f); same heaps as an index of the %d surviving rows: %s"
              % (mode.upper(), share * 100, len(S), f.info()["bitmap_bytes"] / 2 ** 20, med * 1e3, lo * 1e3, hi * 1e3, med_f * 1e3, med_u * 1e3,
                 med_f / med_u, int(keep.sum()), same), flush=True)
        f.close()
    close(full)
    if torch is not None:   # (c)
        keys = rng.permutation(10_000_000)[:1_000_000].astype(np.uint32)
        d_keys = torch.from_numpy(keys.view(np.int32)).cuda()
        torch.cuda.synchronize()
        med_h, _ = timed(lambda: pyqadc.AdcFilter(keys, "exclude").close(), max(iters, 20))
        med_d, _ = timed(lambda: pyqadc.AdcFilter.from_device(d_keys, "exclude").close(), max(iters, 20))
        res["filter_create_1e6_keys_host_ms"] = med_h * 1e3
        res["filter_create_1e6_keys_device_ms"] = med_d * 1e3
        print("creating (and destroying) a filter of 10^6 keys spread over 10^7 (bitmap 1.2 MiB): from host memory %.3f ms, from device memory "
              "%.3f ms" % (med_h * 1e3, med_d * 1e3), flush=True)


def spread(fn, iters, warmup=3):
    """(median, min, max) seconds of fn()"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def view_legs(legs, iters, res):
    """--bits 4: the float-ADC view of a 4-bit index"""
    import pyoracle as po
    rng = np.random.default_rng(4)
    zero = np.zeros((1, 1), np.int32)
    if "lone" in legs:
        for n in (1_000_000, 100_000_000):
            for M in (16, 32):
                cs = M // 2
                src = pyqadc.Index(M)
                src.add_partition_synthetic(n, 1234 + M)
                src.finalize(0.01)
                view = pyqadc.AdcIndex.view_of(src)
                tb = ((rng.random((1, 1, M * 16), dtype=np.float32) * np.float32(4.0)) ** 2).astype(np.float32)
                it = max(iters, 50) if n <= 1_000_000 else iters
                tag = "view%dx4_%.0e" % (M, n)
                if M == 16:   # the 8x8 engine on as many codes of as many bytes, in turn with the view
                    adc8 = pyqadc.AdcIndex(8, 8)
                    adc8.add_partitions([rng.integers(0, 256, (n, 8), dtype=np.uint8)])
                    tb8 = tables_for(rng, 1, 1)
                    med_v, med_8 = alternated(lambda: view.query_scan(zero, tb, R), lambda: adc8.query_scan(zero, tb8, R), it, warmup=3)
                    res[tag + "_alternated_ms"] = med_v * 1e3
                    res["adc8x8_%.0e_alternated_ms" % n] = med_8 * 1e3
                    print("n = %.0e, one query/call, alternated: 16x4 view %.3f ms, 8x8 engine %.3f ms (view / 8x8 = %.3f)"
                          % (n, med_v * 1e3, med_8 * 1e3, med_v / med_8), flush=True)
                    adc8.close()
                med, lo, hi = spread(lambda: view.query_scan(zero, tb, R), it)
                res[tag + "_ms_median_min_max"] = [med * 1e3, lo * 1e3, hi * 1e3]
                res[tag + "_codes_per_s"] = n / med
                res[tag + "_hbm_roofline_share"] = n * cs / med / HBM_BPS
                print("%dx4 view, %.0e codes, one synchronous query: %.3f ms (%.3f .. %.3f) = %.3g codes/s = %.3f of the HBM roofline "
                      "at %d B per code" % (M, n, med * 1e3, lo * 1e3, hi * 1e3, n / med, n * cs / med / HBM_BPS, cs), flush=True)
                if n == 1_000_000:
                    codes = src.read_codes(0, 0, n)
                    tt = tb.reshape(1, -1)
                    med_c, _ = timed(lambda: po.scan4_start(M, [codes], None, tt, R), 5, warmup=1)
                    res["cpu_scan_4_%d_restatement_us" % M] = med_c * 1e6
                    print("CPU scan_4<%d>, 10^6 codes, 1 thread (C restatement): %.1f us" % (M, med_c * 1e6), flush=True)
                    if po.have_ref_float():
                        med_c, _ = timed(lambda: po.reff_scan4_start(M, [codes], None, tt, R), 5, warmup=1)
                        res["cpu_scan_4_%d_reference_build_us" % M] = med_c * 1e6
                        print("CPU scan_4<%d>, 10^6 codes, 1 thread (reference build, -O3 -ffast-math AVX2): %.1f us = %.1fx the view's call"
                              % (M, med_c * 1e6, med_c / med), flush=True)
                view.close()
                src.close()
    if "profile" in legs:
        n = 100_000_000
        for M in (16, 32):
            src = pyqadc.Index(M)
            src.add_partition_synthetic(n, 1234 + M)
            src.finalize(0.01)
            view = pyqadc.AdcIndex.view_of(src)
            tb = ((rng.random((1, 1, M * 16), dtype=np.float32) * np.float32(4.0)) ** 2).astype(np.float32)
            for _ in range(5):
                view.query_scan(zero, tb, R)
            view.close()
            src.close()
        adc8 = pyqadc.AdcIndex(8, 8)
        adc8.add_partitions([rng.integers(0, 256, (n, 8), dtype=np.uint8)])
        tb8 = tables_for(rng, 1, 1)
        for _ in range(5):
            adc8.query_scan(zero, tb8, R)
        adc8.close()
    if "ivf_search" in legs:
        n, dim, M, K, ma, nq = 1_000_000, 128, 16, 256, 24, 1024
        centers = (rng.normal(size=(2000, dim)) * 3).astype(np.float32)
        vectors = centers[rng.integers(0, len(centers), n)]
        vectors += rng.normal(size=(n, dim)).astype(np.float32)
        queries = (centers[rng.integers(0, len(centers), nq)] + rng.normal(size=(nq, dim))).astype(np.float32)
        coarse, _ = pyqadc.kmeans_iterations(vectors[:100000], vectors[rng.choice(n, K, replace=False)], 5)
        sample = vectors[rng.choice(n, 16, replace=False)]
        near = pyqadc.coarse_assign(sample, coarse, 1)[:, 0]
        codebooks = np.ascontiguousarray((sample - coarse[near]).reshape(16, M, dim // M).transpose(1, 0, 2), np.float32)
        if TRAINED:
            codebooks = trained_codebooks(vectors, coarse, M, 4, rng)
        part_of, codes = pyqadc.ivf_encode(codebooks, vectors, coarse)
        del vectors
        order = np.argsort(part_of, kind="stable")
        bounds = np.searchsorted(part_of[order], np.arange(K + 1))
        src = pyqadc.Index(M)
        src.add_partitions([codes[order[bounds[k]:bounds[k + 1]]] for k in range(K)],
                           [order[bounds[k]:bounds[k + 1]].astype(np.uint32) for k in range(K)])
        src.finalize(0.01)
        src.set_pq(codebooks)
        src.set_coarse(coarse)
        view = pyqadc.AdcIndex.view_of(src)
        host = lambda: view.search(queries, ma, R)
        dev = with_finish(view, 1, host)
        assert same_heaps(host(), dev()), "host and device finish disagree"
        med_h, med_d = alternated(host, dev, max(5, iters))
        res["view16x4_ivf_search_host_finish_ms"] = med_h * 1e3
        res["view16x4_ivf_search_device_finish_ms"] = med_d * 1e3
        res["view16x4_ivf_search_host_finishes"] = int(view.host_finishes())
        print("IVF 16x4 view on encoded vectors, K=256 ma=24, search() of 1024 queries: host finish %.2f ms = %.2f us/query, device finish "
              "%.2f ms = %.2f us/query" % (med_h * 1e3, med_h * 1e6 / nq, med_d * 1e3, med_d * 1e6 / nq), flush=True)
        view.close()
        src.close()
    if "filter" in legs:
        filter_leg(4, iters, res)
    if "add" in legs:
        add_leg(4, iters, res)
    if "remove" in legs:
        remove_leg(4, iters, res)
    if "train" in legs:
        train_leg(4, iters, res)
    if "opq" in legs:
        opq_leg(4, iters, res)
    if "seed" in legs:
        seed_leg(4, iters, res)


def cpu_twin_u16_us(nsq, codes, table, repeat=5):
    """one thread of the host twin's scan_standard<uint16_t, nsq> (tests/cpp/scan_standard16_host.cpp) on one flat list: median us"""
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "tests", "cpp", "scan_standard16_host")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", exe + ".cpp", "-o", exe])
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            np.array([nsq, 1, 0, R, 1], np.int32).tofile(f)
            np.array([len(codes)], np.uint32).tofile(f)
            np.ascontiguousarray(codes, "<u2").tofile(f)
            np.ascontiguousarray(table, np.float32).tofile(f)
        out = subprocess.run([exe, fin, fout, str(repeat)], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    return float(out[out.index("us") + 1])


PACKED_VALU_OPS = 78.6e12   # unfused f32 multiplies or adds per second with packed instructions: half the 157.3 TFLOPS vector peak


def clustered(rng, n, dim, nq=0):
    """n (and nq) vectors around 2000 centres"""
    centers = (rng.normal(size=(2000, dim)) * 3).astype(np.float32)
    vectors = centers[rng.integers(0, len(centers), n)]
    vectors += rng.normal(size=(n, dim)).astype(np.float32)
    queries = (centers[rng.integers(0, len(centers), nq)] + rng.normal(size=(nq, dim))).astype(np.float32)
    return vectors, queries


def cpu_twin_encode16(codebooks, vectors):
    """one thread of the host twin's pq_bytes::encode (tools/encode16_host_twin.cpp) -> (seconds, codes uint16 [n][nsq])"""
    import subprocess
    import tempfile
    nsq, dim = codebooks.shape[0], vectors.shape[1]
    with tempfile.TemporaryDirectory() as d:
        exe, fin, fout = os.path.join(d, "twin"), os.path.join(d, "in"), os.path.join(d, "out")
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", os.path.join(ROOT, "tools", "encode16_host_twin.cpp"), "-o", exe])
        with open(fin, "wb") as f:
            np.array([nsq, dim, len(vectors)], np.int32).tofile(f)
            np.ascontiguousarray(codebooks, np.float32).tofile(f)
            np.ascontiguousarray(vectors, np.float32).tofile(f)
        out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, check=True).stdout.decode().split()
        codes = np.fromfile(fout, "<u2").reshape(len(vectors), nsq)
    return float(out[out.index("us") + 1]) * 1e-6, codes


TRAINED = False   # --trained-codebooks


def trained_codebooks(vectors, coarse, nsq, bits, rng):
    """--trained-codebooks: 10 rounds of train_pq on the residuals of the first 10^5 vectors, seeded with 2^bits sampled residuals"""
    learn = vectors[:100000]
    sample = learn[rng.choice(len(learn), 1 << bits, replace=False)]
    near = pyqadc.coarse_assign(sample, coarse, 1)[:, 0]
    seed = np.ascontiguousarray((sample - coarse[near]).reshape(1 << bits, nsq, vectors.shape[1] // nsq).transpose(1, 0, 2), np.float32)
    t0 = time.perf_counter()
    codebooks, _, empty = pyqadc.train_pq(learn, seed, 10, coarse=coarse)
    print("codebooks %dx%d learned by train_pq on %d residuals in %.2f s (%d empty clusters)" % (nsq, bits, len(learn), time.perf_counter() - t0, empty),
          flush=True)
    return codebooks


def trained_codebooks16(vectors, coarse, nsq, rng):
    """--trained-codebooks at 16 bits: 10 rounds of train_pq16 on the residuals of the first min(n, 10^6) vectors (at least 65536),
    seeded with 65536 sampled residuals"""
    learn = vectors[:1_000_000]
    assert len(learn) >= 65536, "learning 16-bit sub-quantizers takes at least 65536 vectors"
    sample = learn[rng.choice(len(learn), 65536, replace=False)]
    near = pyqadc.coarse_assign(sample, coarse, 1)[:, 0]
    seed = np.ascontiguousarray((sample - coarse[near]).reshape(65536, nsq, vectors.shape[1] // nsq).transpose(1, 0, 2), np.float32)
    t0 = time.perf_counter()
    codebooks, _, empty = pyqadc.train_pq16(learn, seed, 10, coarse=coarse)
    print("codebooks %dx16 learned by train_pq16 on %d residuals in %.2f s (%d empty clusters)" % (nsq, len(learn), time.perf_counter() - t0, empty),
          flush=True)
    if empty:                                                    # an empty cluster is NaN and not repaired: it keeps its seed row here
        nan = np.isnan(codebooks).any(axis=2)
        codebooks[nan] = seed[nan]
    return codebooks


def cpu_twin_train16(vectors, seed, rounds):
    """one thread of the host twin's pq_train16_iterations (tests/cpp/pq_train16_host.cpp) -> seconds"""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe, fin, fout = os.path.join(d, "twin"), os.path.join(d, "in"), os.path.join(d, "out")
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "pq_train16_host.cpp"), "-o", exe])
        with open(fin, "wb") as f:
            np.array([len(vectors), vectors.shape[1], seed.shape[0], 0, 0, rounds, 1], np.int32).tofile(f)
            np.ascontiguousarray(vectors, np.float32).tofile(f)
            np.ascontiguousarray(seed, np.float32).tofile(f)
        t0 = time.perf_counter()
        subprocess.run([exe, "run", fin, fout], stdout=subprocess.PIPE, check=True)
        return time.perf_counter() - t0


def same_bits(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


def train16_leg(iters, res, profile_only=False):
    """train_pq16 alternated with the route without it: kmeans_iterations on every host slice"""
    rng = np.random.default_rng(1916)
    n, dim, rounds, twin_n = 1_000_000, 128, 2, 256
    vectors, _ = clustered(rng, n, dim)
    for nsq in (2, 4, 8):
        ds = dim // nsq
        seed = pyqadc.pq_seed(vectors, nsq, 16, rng)
        tag = "train_%dx16_n%d" % (nsq, n)

        def new_route(r=rounds):
            return pyqadc.train_pq16(vectors, seed, r)

        def slice_route():
            cb = np.zeros_like(seed)
            assign = np.zeros((n, nsq), np.uint16)
            for m in range(nsq):
                cb[m], a = pyqadc.kmeans_iterations(np.ascontiguousarray(vectors[:, m * ds:(m + 1) * ds]), seed[m], rounds)
                assign[:, m] = a
            return cb, assign

        cb, codes, empty = new_route()
        if profile_only:
            continue
        res[tag + "_empty_clusters"] = int(empty)
        try:
            cb2, assign = slice_route()
        except pyqadc.QadcError as e:
            twin_s = cpu_twin_train16(vectors[:twin_n], seed, rounds)
            med_new, lo, hi = spread(new_route, max(5, iters // 2), warmup=1)
            res[tag + "_train_pq16_s_median_min_max"] = [med_new, lo, hi]
            res[tag + "_host_twin_thread_extrapolated_s"] = twin_s * n / twin_n
            print("PQ training %dx16, %.0e clustered 128-d vectors, %d rounds: kmeans_iterations per host slice cannot run here (%s); train_pq16 "
                  "%.3f s (%.3f .. %.3f); one CPU thread of the host twin, %d vectors in %.2f s, EXTRAPOLATED to n: %.0f s"
                  % (nsq, n, rounds, e, med_new, lo, hi, twin_n, twin_s, twin_s * n / twin_n), flush=True)
        else:
            assert same_bits(cb, cb2), "the routes' codebooks differ"
            assert np.array_equal(codes, assign), "the routes' codes differ"
            count = max(5, iters // 2)
            tn, to = [], []
            for _ in range(count):                               # A B A B ...; the calls above were the warm-up of each arm
                for f, ts in ((new_route, tn), (slice_route, to)):
                    t0 = time.perf_counter()
                    f()
                    ts.append(time.perf_counter() - t0)
            med_new, med_old = float(np.median(tn)), float(np.median(to))
            res[tag + "_train_pq16_s_median_min_max"] = [med_new, min(tn), max(tn)]
            res[tag + "_kmeans_per_slice_s_median_min_max"] = [med_old, min(to), max(to)]
            res[tag + "_slices_over_train_pq16"] = med_old / med_new
            print("PQ training %dx16, %.0e clustered 128-d vectors, %d rounds, host to host, %d alternations: train_pq16 %.3f s (%.3f .. %.3f); "
                  "kmeans_iterations on %d host slices %.3f s (%.3f .. %.3f) = %.2fx (equal bits; %d empty clusters)"
                  % (nsq, n, rounds, count, med_new, min(tn), max(tn), nsq, med_old, min(to), max(to), med_old / med_new, empty), flush=True)
        # a round = the difference of a 2 * rounds call and a rounds call (the upload and the fixed costs cancel); the encoder's call
        # carries its own upload, so 1 - encode / round is a lower bound of the share spent outside the encoder
        long_s, _ = timed(lambda: new_route(2 * rounds), 3, warmup=0)
        short_s, _ = timed(new_route, 3, warmup=0)
        enc_s, _ = timed(lambda: pyqadc.adc_encode16(seed, vectors), 3, warmup=0)
        round_s = (long_s - short_s) / rounds
        roof = 2.0 * n * dim * 65536 / PACKED_VALU_OPS
        res[tag + "_round_s"] = round_s
        res[tag + "_adc_encode16_call_s"] = enc_s
        outside = max(0.0, 1.0 - enc_s / round_s) if round_s > 0 else float("nan")      # (nan: the difference drowned in the clock's noise)
        res[tag + "_share_outside_encoder_at_least"] = outside
        print("  a round (4-round call minus 2-round call, halved): %.3f s; one adc_encode16 call, upload included: %.3f s (packed-VALU roof "
              "%.3f s): the share of a round outside the encoder is at least %.3f" % (round_s, enc_s, roof, outside), flush=True)


REPAIR = False      # --repair
PARENT_LIB = None   # --parent-lib
REPAIR_DUP, REPAIR_ZERO = 0.10, 0.30


def repair_sets(bits):
    """-> (nsq, rounds, healthy set, dying set, rng): the train leg's 10^6 x 128 set, and the same with REPAIR_DUP of its rows
    overwritten by copies of other rows and sub-space 0 zeroed on REPAIR_ZERO of the rows"""
    rng = np.random.default_rng(1900 + bits)
    n, dim = 1_000_000, 128
    nsq, rounds = {4: (16, 10), 8: (8, 10), 16: (2, 2)}[bits]
    vectors, _ = clustered(rng, n, dim)
    dying = vectors.copy()
    dup = rng.choice(n, int(n * REPAIR_DUP), replace=False)
    dying[dup] = vectors[rng.integers(0, n, len(dup))]
    dying[rng.choice(n, int(n * REPAIR_ZERO), replace=False), :dim // nsq] = 0
    return nsq, rounds, vectors, dying, rng


def repair_leg(bits, iters, res):
    """the empty-cluster repair: its cost where no cluster is empty, its effect where clusters die"""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pq_train_compose as ptc
    import pq_train16_compose as pt16
    nsq, rounds, vectors, dying, rng = repair_sets(bits)
    n, dim = vectors.shape
    train = pyqadc.train_pq16 if bits == 16 else pyqadc.train_pq
    encode = {4: pyqadc.pq_encode, 8: pyqadc.adc_encode, 16: pyqadc.adc_encode16}[bits]
    error = (pt16 if bits == 16 else ptc).reconstruction_error
    tag = "repair_%dx%d_n%d" % (nsq, bits, n)
    seed = pyqadc.pq_seed(vectors, nsq, bits, rng)
    plain = train(vectors, seed, rounds)
    fixed = train(vectors, seed, rounds, repair=True)
    arms = {"plain": lambda: train(vectors, seed, rounds), "repair": lambda: train(vectors, seed, rounds, repair=True)}
    if PARENT_LIB:                                             # the other build's plain C call, in this process, in turn with ours
        old = C.CDLL(PARENT_LIB)
        f32p = C.POINTER(C.c_float)
        fn = old.qadc_pq_train16_host if bits == 16 else old.qadc_pq_train_host
        fn.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int] + ([C.c_int] if bits != 16 else []) + [C.c_int, f32p, f32p, f32p, C.c_int, C.c_void_p,
                                                                                                  C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int]
        cols = nsq // 2 if bits == 4 else nsq

        def parent():
            cb = seed.copy()
            codes = np.zeros((n, cols), "<u2" if bits == 16 else np.uint8)
            empty = C.c_uint64(0)
            head = (vectors.ctypes.data_as(f32p), n, dim, nsq) + ((bits,) if bits != 16 else ())
            assert fn(*head, 0, None, None, cb.ctypes.data_as(f32p), rounds, codes.ctypes.data_as(C.c_void_p), C.byref(empty), 1, 1, 0) == 0
            return cb, codes, empty.value
        assert np.array_equal(parent()[0].view(np.uint32), plain[0].view(np.uint32)), "the parent build's codebooks differ from the plain call's"
        arms["parent"] = parent
    times = {k: [] for k in arms}
    for f in arms.values():
        f()
    for _ in range(max(3, iters // 2)):                        # A B C A B C ...
        for k, f in arms.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    for k, ts in times.items():
        res[tag + "_healthy_%s_s" % k] = float(np.median(ts))
        res[tag + "_healthy_%s_all_s" % k] = [float(t) for t in ts]
    base = res[tag + "_healthy_%s_s" % ("parent" if PARENT_LIB else "plain")]
    res[tag + "_healthy_rounds"] = rounds
    res[tag + "_healthy_repair_over_%s" % ("parent" if PARENT_LIB else "plain")] = res[tag + "_healthy_repair_s"] / base
    res[tag + "_healthy_empty"] = [int(plain[2]), int(fixed[2])]
    res[tag + "_healthy_repaired"] = int(fixed[3])
    print("repair %dx%d, %.0e clustered 128-d vectors, %d rounds, call to return (upload included): %s; repaired / %s = %.4f; empty %d and %d, "
          "repaired %d" % (nsq, bits, n, rounds, ", ".join("%s %.4f s" % (k, float(np.median(ts))) for k, ts in times.items()),
                           "parent" if PARENT_LIB else "plain", res[tag + "_healthy_repair_s"] / base, plain[2], fixed[2], fixed[3]), flush=True)
    seed = pyqadc.pq_seed(dying, nsq, bits, rng)
    for name, kw in (("plain", {}), ("repair", {"repair": True})):
        out = train(dying, seed, rounds, **kw)
        with np.errstate(all="ignore"):
            codes = encode(out[0], dying)
            codes = codes[-1] if isinstance(codes, tuple) else codes
            mse = error(dying, out[0], codes) / n
        res[tag + "_dying_%s_empty" % name] = int(out[2])
        res[tag + "_dying_%s_repaired" % name] = int(out[3]) if kw else 0
        res[tag + "_dying_%s_mse" % name] = float(mse)
        print("repair %dx%d, the same set with %.0f %% of the rows duplicated and sub-space 0 zeroed on %.0f %%, %d rounds, %s: empty %d, repaired "
              "%d, mean squared quantization error %.6g" % (nsq, bits, 100 * REPAIR_DUP, 100 * REPAIR_ZERO, rounds, name, out[2], int(out[3]) if kw else 0,
                                                            mse), flush=True)


def opq_repair_leg(bits, iters, res):
    """train_opq with and without the repair on the train leg's dying set"""
    nsq, _, _, dying, rng = repair_sets(bits)
    seed = pyqadc.pq_seed(dying, nsq, bits, rng)
    tag = "repair_opq_%dx%d_n%d" % (nsq, bits, len(dying))
    plain, fixed = pyqadc.train_opq(dying, seed, 4, 2), pyqadc.train_opq(dying, seed, 4, 2, repair=True)
    t_plain, t_fixed = alternated(lambda: pyqadc.train_opq(dying, seed, 4, 2), lambda: pyqadc.train_opq(dying, seed, 4, 2, repair=True), 3, warmup=0)
    res[tag + "_plain_s"], res[tag + "_repair_s"] = t_plain, t_fixed
    res[tag + "_empty"] = [int(plain[3]), int(fixed[3])]
    res[tag + "_repaired"] = int(fixed[5])
    print("repair, OPQ %dx%d on the dying set, outer 4 x inner 2: train_opq %.3f s, with repair %.3f s; empty %d and %d, repaired %d"
          % (nsq, bits, t_plain, t_fixed, plain[3], fixed[3], fixed[5]), flush=True)


def train_leg(bits, iters, res):
    """train_pq alternated with the route without it: kmeans_iterations on every host slice"""
    rng = np.random.default_rng(1900 + bits)
    if REPAIR:
        return repair_leg(bits, iters, res)
    dim, rounds = 128, 10
    nsq = {4: 16, 8: 8}[bits]
    ds = dim // nsq
    for n in (100_000, 1_000_000):
        vectors, _ = clustered(rng, n, dim)
        seed = pyqadc.pq_seed(vectors, nsq, bits, rng)

        def new_route():
            return pyqadc.train_pq(vectors, seed, rounds)

        def slice_route():
            cb = np.zeros_like(seed)
            assign = np.zeros((n, nsq), np.uint8)
            for m in range(nsq):
                cb[m], a = pyqadc.kmeans_iterations(np.ascontiguousarray(vectors[:, m * ds:(m + 1) * ds]), seed[m], rounds)
                assign[:, m] = a
            return cb, assign

        cb, codes, empty = new_route()
        cb2, assign = slice_route()
        packed = assign if bits == 8 else assign[:, 0::2] | (assign[:, 1::2] << 4)
        nan = np.isnan(cb)
        assert np.array_equal(nan, np.isnan(cb2)) and ((cb.view(np.uint32) == cb2.view(np.uint32)) | nan).all(), "the routes' codebooks differ"
        assert np.array_equal(codes, packed), "the routes' codes differ"
        med_new, med_old = alternated(new_route, slice_route, max(3, iters // 2), warmup=1)
        tag = "train_%dx%d_n%d" % (nsq, bits, n)
        res[tag + "_train_pq_s"] = med_new
        res[tag + "_kmeans_per_slice_s"] = med_old
        res[tag + "_slices_over_train_pq"] = med_old / med_new
        res[tag + "_empty_clusters"] = int(empty)
        print("PQ training %dx%d, %.0e clustered 128-d vectors, %d rounds, host to host: train_pq %.3f s; kmeans_iterations on %d host slices "
              "%.3f s = %.2fx (equal bits; %d empty clusters)" % (nsq, bits, n, rounds, med_new, nsq, med_old, med_old / med_new, empty), flush=True)


def opq_leg(bits, iters, res):
    """train_opq alternated with the same loop composed from the public calls; the learned pair's reconstruction error beside plain PQ's"""
    if REPAIR:
        return opq_repair_leg(bits, iters, res)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pq_train_compose as ptc
    rng = np.random.default_rng(2100 + bits)
    n, dim, outer, inner = 1_000_000, 128, 4, 2                  # 4 x 2 rounds and 2 closing ones: 10 k-means rounds
    nsq = {4: 16, 8: 8}[bits]
    vectors, _ = clustered(rng, n, dim)
    seed = pyqadc.pq_seed(vectors, nsq, bits, rng)
    eye = np.eye(dim, dtype=np.float32)

    def new_route():
        return pyqadc.train_opq(vectors, seed, outer, inner)

    def composed_route():
        rot, cb = eye, seed
        for _ in range(outer):
            cb, codes, _ = pyqadc.train_pq(vectors, cb, inner, rotation=rot)
            rot = pyqadc.procrustes(pyqadc.opq_cross(vectors, codes, cb))[0]
        cb, codes, empty = pyqadc.train_pq(vectors, cb, inner, rotation=rot)
        return rot, cb, codes, empty, outer

    got, want = new_route(), composed_route()
    nan = np.isnan(got[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "the routes' rotations differ"
    assert np.array_equal(nan, np.isnan(want[1])) and ((got[1].view(np.uint32) == want[1].view(np.uint32)) | nan).all(), "the routes' codebooks differ"
    assert np.array_equal(got[2], want[2]) and got[3:] == want[3:], "the routes' codes differ"
    med_new, med_old = alternated(new_route, composed_route, max(3, iters // 2), warmup=1)
    rounds = (outer + 1) * inner
    pq_cb, pq_codes, pq_empty = pyqadc.train_pq(vectors, seed, rounds)
    err_pq = ptc.reconstruction_error(vectors, pq_cb, pq_codes)
    err_opq = ptc.reconstruction_error(vectors.astype(np.float64) @ got[0].astype(np.float64).T, got[1], got[2])
    t_pq, _ = timed(lambda: pyqadc.train_pq(vectors, seed, rounds), 3, warmup=0)
    tag = "opq_%dx%d_n%d" % (nsq, bits, n)
    res[tag + "_train_opq_s"] = med_new
    res[tag + "_composed_s"] = med_old
    res[tag + "_composed_over_train_opq"] = med_old / med_new
    res[tag + "_train_pq_same_rounds_s"] = t_pq
    res[tag + "_error_opq"] = err_opq
    res[tag + "_error_pq"] = err_pq
    res[tag + "_empty_clusters"] = [int(got[3]), int(pq_empty)]
    print("OPQ training %dx%d, %.0e clustered 128-d vectors, outer %d x inner %d + %d closing = %d rounds, host to host: train_opq %.3f s; "
          "the loop of train_pq / opq_cross / procrustes %.3f s = %.2fx (equal bits); train_pq with %d rounds %.3f s.  Reconstruction error: "
          "OPQ %.4g, PQ %.4g (%.3f of it; %d and %d empty clusters)"
          % (nsq, bits, n, outer, inner, inner, rounds, med_new, med_old, med_old / med_new, rounds, t_pq, err_opq, err_pq, err_opq / err_pq,
             got[3], pq_empty), flush=True)


def cpu_twin_seed_round_s(vectors, sq_count):
    """seconds per round of one thread of the host twin (host/kmeans_seed.hpp through tests/cpp/kmeans_seed_host.cpp): the
    difference of a k = 5 and a k = 3 run of its driver, halved — the file's read and the process start cancel"""
    import subprocess
    import tempfile
    n, dim = vectors.shape
    with tempfile.TemporaryDirectory() as d:
        exe, fin, fout = os.path.join(d, "twin"), os.path.join(d, "in"), os.path.join(d, "out")
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "kmeans_seed_host.cpp"), "-o", exe])
        ts = []
        for k in (3, 5):
            with open(fin, "wb") as f:
                np.array([n, dim, sq_count, k, 0, 0, 1, 1], np.uint64).tofile(f)
                vectors.tofile(f)
            t0 = time.perf_counter()
            subprocess.run([exe, "rows", fin, fout], stdout=subprocess.PIPE, check=True)
            ts.append(time.perf_counter() - t0)
    return (ts[1] - ts[0]) / 2


def seed_leg(bits, iters, res):
    """k-means++ seeding: kmeans_seed per call, the update launches' bytes per second, the CPU twin per
    round, and the quantization error and empty clusters after the leg's usual training rounds from kmeans_seed and from pq_seed"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pq_train16_compose as p16c
    import pq_train_compose as ptc
    rng = np.random.default_rng(2300 + bits)
    n, dim = 1_000_000, 128
    nsq, rounds = {4: (16, 10), 8: (8, 10), 16: (2, 2)}[bits]
    vectors, _ = clustered(rng, n, dim)
    shapes = [("pq_%dx%d" % (nsq, bits), nsq, 1 << bits)] + ([("coarse_K4096", 1, 4096)] if bits == 8 else [])
    for name, S, k in shapes:
        tag = "seed_%s_n%d" % (name, n)
        count = 1 if k > 4096 else max(3, iters // 3)
        full_s, _ = timed(lambda: pyqadc.kmeans_seed(vectors, k, sq_count=S, seed=1), count, warmup=0 if k > 4096 else 1)
        half_s, _ = timed(lambda: pyqadc.kmeans_seed(vectors, k // 2, sq_count=S, seed=1), count, warmup=0)
        round_s = (full_s - half_s) / (k - k // 2)                # the upload and the fixed costs cancel
        round_bytes = n * dim * 4 + 2 * n * S * 4
        twin_s = cpu_twin_seed_round_s(vectors, S)
        res[tag + "_call_s"] = full_s
        res[tag + "_half_k_call_s"] = half_s
        res[tag + "_round_s"] = round_s
        res[tag + "_round_bytes"] = round_bytes
        res[tag + "_round_bytes_per_s"] = round_bytes / round_s
        res[tag + "_cpu_twin_round_s"] = twin_s
        print("k-means++ seeding %s, k = %d in %d sub-spaces, %.0e clustered 128-d vectors, host to host: %.3f s per call (k / 2: %.3f s); a "
              "round (update + pick) %.1f us = %.2f TB/s of its %d MB; the CPU twin on one thread %.3f s per round"
              % (name, k, S, n, full_s, half_s, round_s * 1e6, round_bytes / round_s / 1e12, round_bytes >> 20, twin_s), flush=True)
    # the quality after the leg's usual rounds, from both seeds on the same data
    K = 1 << bits
    seeds = {"kmeans_seed": pyqadc.pq_seed_pp(vectors, nsq, bits, 1), "pq_seed": pyqadc.pq_seed(vectors, nsq, bits, rng)}
    for who, seed in seeds.items():
        if bits == 16:
            cb, codes, empty = pyqadc.train_pq16(vectors, seed, rounds)
            codes = pyqadc.adc_encode16(np.nan_to_num(cb, nan=1e18), vectors)[1]      # the codes under the final codebooks (empty clusters far away)
            err = p16c.reconstruction_error(vectors, np.nan_to_num(cb, nan=1e18), codes)
        else:
            cb, codes, empty = pyqadc.train_pq(vectors, seed, rounds)
            final = np.nan_to_num(cb, nan=1e18)
            codes = pyqadc.pq_encode(final, vectors) if bits == 4 else pyqadc.adc_encode(final, vectors)[1]
            err = ptc.reconstruction_error(vectors, final, codes)
        tag = "seed_quality_%dx%d_n%d_%s" % (nsq, bits, n, who)
        res[tag + "_mse"] = err / n
        res[tag + "_empty_clusters"] = int(empty)
        print("  %d rounds of train_pq%s from %s: mean squared quantization error %.4f, %d of %d clusters empty"
              % (rounds, "16" if bits == 16 else "", who, err / n, empty, nsq * K), flush=True)


def add_leg(bits, iters, res):
    """database build: add_vectors (empty / reserved index) alternated with encode + numpy grouping + add_partitions"""
    rng = np.random.default_rng(1700 + bits)
    n, dim, K = 1_000_000, 128, 256
    nsq = {4: 16, 8: 8, 16: 2}[bits]
    vectors, _ = clustered(rng, n, dim)
    coarse, _ = pyqadc.kmeans_iterations(vectors[:100000], vectors[rng.choice(n, K, replace=False)], 5)
    sample = vectors[rng.choice(n, 1 << bits, replace=False)]
    codebooks = np.ascontiguousarray(sample.reshape(1 << bits, nsq, dim // nsq).transpose(1, 0, 2), np.float32)
    if TRAINED:
        codebooks = trained_codebooks16(vectors, coarse, nsq, rng) if bits == 16 else trained_codebooks(vectors, coarse, nsq, bits, rng)
    encode = {4: pyqadc.ivf_encode, 8: pyqadc.adc_encode, 16: pyqadc.adc_encode16}[bits]

    def make():
        idx = pyqadc.Index(nsq) if bits == 4 else pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)
        idx.set_pq(codebooks)
        idx.set_coarse(coarse)
        return idx

    kept = {}

    def parent_route():
        idx = make()
        a, codes = encode(codebooks, vectors, coarse)
        order = np.argsort(a, kind="stable")
        bounds = np.searchsorted(a[order], np.arange(K + 1))
        idx.add_partitions([codes[order[bounds[k]:bounds[k + 1]]] for k in range(K)],
                           [order[bounds[k]:bounds[k + 1]].astype(np.uint32) for k in range(K)])
        kept["sizes"] = np.diff(bounds)
        return idx

    def new_route(reserve):
        idx = make()
        if reserve:
            idx.reserve(kept["sizes"])
        idx.add_vectors(vectors)
        return idx

    # the routes build the same database
    a, b = parent_route(), new_route(False)
    c = new_route(True)
    for k in range(K):
        (ca, la), (cb, lb), (cc, lc) = a.read_partition(k), b.read_partition(k), c.read_partition(k)
        assert np.array_equal(ca, cb) and np.array_equal(la, lb), "partition %d differs between the routes" % k
        assert np.array_equal(ca, cc) and np.array_equal(la, lc), "partition %d of the reserved index differs" % k
    relocations = b.relocations()
    assert c.relocations() == 0, "the reserved build relocated"
    a.close()
    b.close()
    c.close()

    def timed_build(route):
        def run():                                                           # the index's creation and release are outside the clock
            t0 = time.perf_counter()
            idx = route()
            t = time.perf_counter() - t0
            idx.close()
            return t
        return run

    arms = {"parent_route": timed_build(parent_route), "add_vectors_empty": timed_build(lambda: new_route(False)),
            "add_vectors_reserved": timed_build(lambda: new_route(True))}
    times = dict((name, []) for name in arms)
    for it in range(1 + max(3, iters // 2)):                                 # one warm-up round, then the arms in turn
        for name, run in arms.items():
            t = run()
            if it:
                times[name].append(t)
    tag = "add_%dx%d" % (nsq, bits)
    for name, ts in times.items():
        res["%s_%s_s_median_min_max" % (tag, name)] = [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]
    res[tag + "_relocations_of_the_unreserved_call"] = int(relocations)
    med = dict((name, float(np.median(ts))) for name, ts in times.items())
    print("database build %dx%d, %.0e clustered 128-d vectors, K = %d (index creation and set_pq / set_coarse inside every arm): encode + numpy "
          "grouping + add_partitions %.3f s; add_vectors into an empty index %.3f s (%d relocating passes' call); into a reserved one %.3f s "
          "= %.2fx / %.2fx the route without it" % (nsq, bits, n, K, med["parent_route"], med["add_vectors_empty"], relocations,
                                                     med["add_vectors_reserved"], med["parent_route"] / med["add_vectors_empty"],
                                                     med["parent_route"] / med["add_vectors_reserved"]), flush=True)


def remove_leg(bits, iters, res):
    """remove_labels alternated with the route without it: read_partition of every partition, the filter on the host, add_partitions"""
    rng = np.random.default_rng(1800 + bits)
    n, dim = 1_000_000, 128
    nsq = {4: 16, 8: 8, 16: 2}[bits]
    vectors, _ = clustered(rng, n, dim)
    coarse, _ = pyqadc.kmeans_iterations(vectors[:100000], vectors[rng.choice(n, 256, replace=False)], 5)
    sample = vectors[rng.choice(n, 1 << bits, replace=False)]
    codebooks = np.ascontiguousarray(sample.reshape(1 << bits, nsq, dim // nsq).transpose(1, 0, 2), np.float32)
    if TRAINED:
        codebooks = trained_codebooks16(vectors, coarse, nsq, rng) if bits == 16 else trained_codebooks(vectors, coarse, nsq, bits, rng)

    def make():
        return pyqadc.Index(nsq) if bits == 4 else pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)

    def read_all(idx):
        return [idx.read_partition(k) for k in range(idx.partition_count())]

    for K, fractions in ((256, (0.01, 0.1, 0.5)), (8, (0.1,))):                   # K = 8: a few very long partitions, one workgroup each
        src = make()
        src.set_pq(codebooks)
        src.set_coarse(coarse[:K])
        src.add_vectors(vectors)
        base = read_all(src)                                                     # the database every arm starts from
        src.close()
        longest = max(len(c) for c, _ in base)

        def fresh():
            idx = make()
            idx.add_partitions([c for c, _ in base], [l for _, l in base])
            return idx

        for f in fractions:
            removed = rng.choice(n, int(f * n), replace=False).astype(np.uint32)

            def new_route(idx):
                assert idx.remove_labels(removed) == len(removed)
                return idx

            def old_route(idx):
                parts = read_all(idx)
                keep = [~np.isin(l, removed) for _, l in parts]
                out = make()
                out.add_partitions([c[m] for (c, _), m in zip(parts, keep)], [l[m] for (_, l), m in zip(parts, keep)])
                return out

            a, b = fresh(), fresh()                                              # both ends hold the same partitions
            got, want = read_all(new_route(a)), read_all(old_route(b))
            for k in range(K):
                assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), "partition %d differs between the routes" % k
            a.close()
            b.close()
            times = {"remove_labels": [], "read_filter_add_partitions": []}
            for it in range(1 + max(3, iters // 2)):                             # one warm-up round, then the arms in turn
                for name, route in (("remove_labels", new_route), ("read_filter_add_partitions", old_route)):
                    idx = fresh()                                                # (outside the clock, as its release is)
                    t0 = time.perf_counter()
                    out = route(idx)
                    t = time.perf_counter() - t0
                    if out is not idx:
                        out.close()
                    idx.close()
                    if it:
                        times[name].append(t)
            tag = "remove_%dx%d_K%d_%g" % (nsq, bits, K, f)
            for name, ts in times.items():
                res["%s_%s_ms_median_min_max" % (tag, name)] = [float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, float(np.max(ts)) * 1e3]
            res[tag + "_longest_partition"] = int(longest)
            med_new, med_old = (float(np.median(times[k])) for k in ("remove_labels", "read_filter_add_partitions"))
            print("remove %dx%d, %.0e codes in K = %d partitions (longest %d), %g of the labels: remove_labels %.3f ms; read_partition of every "
                  "partition + np.isin + add_partitions into a new index %.3f ms = %.1fx the call"
                  % (nsq, bits, n, K, longest, f, med_new * 1e3, med_old * 1e3, med_old / med_new), flush=True)


def encode16_leg(iters, res):
    rng = np.random.default_rng(1616)
    dim, twin_n = 128, 256
    vectors, _ = clustered(rng, 1_000_000, dim)
    for nsq in (2, 4, 8):
        codebooks = np.ascontiguousarray(vectors[rng.choice(len(vectors), 65536, replace=False)].reshape(65536, nsq, dim // nsq)
                                         .transpose(1, 0, 2))
        twin_s, twin_codes = cpu_twin_encode16(codebooks, vectors[:twin_n])
        for n in (100_000, 1_000_000):
            v = vectors[:n]
            codes = pyqadc.adc_encode16(codebooks, v)[1]
            assert np.array_equal(codes[:twin_n], twin_codes), "the GPU's codes differ from the host twin's"
            med, lo, hi = spread(lambda: pyqadc.adc_encode16(codebooks, v), max(3, iters // 3), warmup=1)
            roof = 2.0 * n * dim * 65536 / PACKED_VALU_OPS
            tag = "encode16_%dx16_%.0e" % (nsq, n)
            res[tag + "_s_median_min_max"] = [med, lo, hi]
            res[tag + "_vectors_per_s"] = n / med
            res[tag + "_packed_valu_roof_s"] = roof
            res[tag + "_share_of_packed_valu_roof"] = roof / med
            res[tag + "_host_twin_thread_extrapolated_s"] = twin_s * n / twin_n
            print("adc_encode16 %dx16, %.0e 128-d vectors, host to host: %.3f s (%.3f .. %.3f) = %.3g vectors/s = %.3f of the packed-VALU "
                  "roof (%.3f s); one CPU thread of the host twin's pq_bytes::encode (a port), %d vectors in %.2f s, EXTRAPOLATED to n: "
                  "%.0f s = %.0fx the GPU call" % (nsq, n, med, lo, hi, n / med, roof / med, roof, twin_n, twin_s, twin_s * n / twin_n,
                                                   twin_s * n / twin_n / med), flush=True)


def encoded_search_leg(iters, res):
    """search() at the ivf_search shape on a database adc_encode16 made, with recall against exact float L2"""
    rng = np.random.default_rng(1617)
    n, dim, K, ma, nq, nq_exact = 1_000_000, 128, 256, 24, 1024, 64
    vectors, queries = clustered(rng, n, dim, nq)
    coarse, _ = pyqadc.kmeans_iterations(vectors[:100000], vectors[rng.choice(n, K, replace=False)], 5)
    sample = vectors[rng.choice(n, 65536, replace=False)]
    residual = sample - coarse[pyqadc.coarse_assign(sample, coarse, 1)[:, 0]]
    vnorm = (vectors.astype(np.float64) ** 2).sum(axis=1)
    exact = [np.argpartition(vnorm - 2.0 * (vectors @ queries[q]), R)[:R] for q in range(nq_exact)]
    for nsq in (2, 4, 8):
        codebooks = np.ascontiguousarray(residual.reshape(65536, nsq, dim // nsq).transpose(1, 0, 2), np.float32)
        if TRAINED:
            codebooks = trained_codebooks16(vectors, coarse, nsq, rng)
        t0 = time.perf_counter()
        part_of, codes = pyqadc.adc_encode16(codebooks, vectors, coarse)
        t_enc = time.perf_counter() - t0
        order = np.argsort(part_of, kind="stable")
        bounds = np.searchsorted(part_of[order], np.arange(K + 1))
        idx = pyqadc.AdcIndex.create16(nsq)
        idx.add_partitions([codes[order[bounds[k]:bounds[k + 1]]] for k in range(K)],
                           [order[bounds[k]:bounds[k + 1]].astype(np.uint32) for k in range(K)])
        idx.set_pq(codebooks)
        idx.set_coarse(coarse)
        keys, _, sizes, _ = idx.search(queries, ma, R)
        hits = sum(len(np.intersect1d(exact[q], keys[q, :sizes[q]])) for q in range(nq_exact))
        med, _ = timed(lambda: idx.search(queries, ma, R), max(3, iters // 2), warmup=1)
        idx.close()
        tag = "adc%dx16_encoded" % nsq
        res[tag + "_ivf_encode_s"] = t_enc
        res[tag + "_ivf_search_ms"] = med * 1e3
        res[tag + "_recall_at_100"] = hits / float(nq_exact * R)
        print("IVF K=256 ma=24 on 10^6 clustered vectors encoded by adc_encode16 at %dx16 (%.2f s, coarse assignment included): search() of "
              "1024 queries %.2f ms = %.1f us/query; recall@100 against exact float L2 over %d queries: %.3f"
              % (nsq, t_enc, med * 1e3, med * 1e6 / nq, nq_exact, hits / float(nq_exact * R)), flush=True)


def word_legs(legs, iters, res):
    """--bits 16: the engine on 16-bit codes, beside the 8-bit engine at equal code bytes"""
    rng = np.random.default_rng(16)
    zero = np.zeros((1, 1), np.int32)

    def tables16(nq, ma, nsq):
        return ((rng.random((nq, ma, nsq * 65536), dtype=np.float32) * np.float32(4.0)) ** 2).astype(np.float32)

    if "lone" in legs:
        for n in (1_000_000, 100_000_000):
            for nsq in (2, 4, 8):
                cs = 2 * nsq
                codes = rng.integers(0, 65536, (n, nsq), dtype=np.uint16)
                idx = pyqadc.AdcIndex.create16(nsq)
                idx.add_partitions([codes])
                adc8 = pyqadc.AdcIndex(cs, 8)
                adc8.add_partitions([codes.view(np.uint8)])             # the same bytes read as cs one-byte codes
                tb, tb8 = tables16(1, 1, nsq), tables_for(rng, 1, 1, cs)
                it = max(iters, 50) if n <= 1_000_000 else iters
                tag = "adc%dx16_%.0e" % (nsq, n)
                med_w, med_8 = alternated(lambda: idx.query_scan(zero, tb, R), lambda: adc8.query_scan(zero, tb8, R), it, warmup=3)
                res[tag + "_alternated_ms"] = med_w * 1e3
                res["adc%dx8_%.0e_alternated_ms" % (cs, n)] = med_8 * 1e3
                print("n = %.0e, one query/call, alternated: %dx16 %.3f ms, %dx8 %.3f ms (16-bit / 8-bit = %.3f)"
                      % (n, nsq, med_w * 1e3, cs, med_8 * 1e3, med_w / med_8), flush=True)
                adc8.close()
                med, lo, hi = spread(lambda: idx.query_scan(zero, tb, R), it)
                res[tag + "_ms_median_min_max"] = [med * 1e3, lo * 1e3, hi * 1e3]
                res[tag + "_codes_per_s"] = n / med
                res[tag + "_hbm_roofline_share"] = n * cs / med / HBM_BPS
                print("%dx16, %.0e codes, one synchronous query (%.1f MiB table uploaded in the call): %.3f ms (%.3f .. %.3f) = %.3g codes/s "
                      "= %.3f of the HBM roofline at %d B per code"
                      % (nsq, n, tb.nbytes / 2 ** 20, med * 1e3, lo * 1e3, hi * 1e3, n / med, n * cs / med / HBM_BPS, cs), flush=True)
                if n == 1_000_000:
                    us = cpu_twin_u16_us(nsq, codes, tb[0, 0])
                    res["cpu_host_twin_scan_standard_u16_%d_us" % nsq] = us
                    print("CPU host twin scan_standard<uint16_t,%d> (a port, -O2), 10^6 codes, 1 thread: %.1f us = %.1fx the GPU call"
                          % (nsq, us, us / (med * 1e6)), flush=True)
                idx.close()
                del codes
    if "ivf_search" in legs or "profile" in legs:
        n, dim, K, ma, nq = 1_000_000, 128, 256, 24, 1024
        part_of = rng.integers(0, K, n)
        order = np.argsort(part_of, kind="stable")
        bounds = np.searchsorted(part_of[order], np.arange(K + 1))
        labels = [order[bounds[k]:bounds[k + 1]].astype(np.uint32) for k in range(K)]
        coarse = (rng.normal(size=(K, dim)) * 3).astype(np.float32)
        queries = (coarse[rng.integers(0, K, nq)] + rng.normal(size=(nq, dim))).astype(np.float32)

        def make(nsq, bits):
            cents = 1 << bits
            idx = pyqadc.AdcIndex.create16(nsq) if bits == 16 else pyqadc.AdcIndex(nsq, 8)
            codes = rng.integers(0, cents, (n, nsq), dtype=np.uint16 if bits == 16 else np.uint8)
            idx.add_partitions([codes[order[bounds[k]:bounds[k + 1]]] for k in range(K)], labels)
            idx.set_pq(rng.standard_normal((nsq, cents, dim // nsq), dtype=np.float32))
            idx.set_coarse(coarse)
            return idx

        if "ivf_search" in legs:
            for nsq in (2, 4, 8):
                idx, adc8 = make(nsq, 16), make(2 * nsq, 8)
                host = lambda: idx.search(queries, ma, R)
                dev = with_finish(idx, 1, host)
                assert same_heaps(host(), dev()), "host and device finish disagree"
                med_w, med_8 = alternated(host, lambda: adc8.search(queries, ma, R), max(3, iters // 2), warmup=1)
                res["adc%dx16_ivf_search_ms" % nsq] = med_w * 1e3
                res["adc%dx8_ivf_search_ms" % (2 * nsq)] = med_8 * 1e3
                res["adc%dx16_ivf_search_table_bytes_per_call" % nsq] = nq * ma * nsq * 65536 * 4
                print("IVF K=256 ma=24 on 10^6 random codes, search() of 1024 queries: %dx16 %.2f ms = %.1f us/query (%.1f GiB of tables "
                      "built and scanned in passes); %dx8 %.2f ms = %.1f us/query"
                      % (nsq, med_w * 1e3, med_w * 1e6 / nq, nq * ma * nsq * 65536 * 4 / 2 ** 30, 2 * nsq, med_8 * 1e3, med_8 * 1e6 / nq),
                      flush=True)
                idx.close()
                adc8.close()
            encoded_search_leg(iters, res)
        if "profile" in legs:
            idx = make(8, 16)
            for _ in range(2):
                idx.search(queries[:64], ma, R)
            idx.close()
    if "encode16" in legs:
        encode16_leg(iters, res)
    if "filter" in legs:
        filter_leg(16, iters, res)
    if "add" in legs:
        add_leg(16, iters, res)
    if "remove" in legs:
        remove_leg(16, iters, res)
    if "train" in legs and REPAIR:
        repair_leg(16, iters, res)
    elif "train" in legs or "train_profile" in legs:
        train16_leg(iters, res, profile_only="train" not in legs)
    if "seed" in legs:
        seed_leg(16, iters, res)
    if "profile" in legs:
        n = 100_000_000
        idx = pyqadc.AdcIndex.create16(8)
        idx.add_partitions([rng.integers(0, 65536, (n, 8), dtype=np.uint16)])
        tb = tables16(1, 1, 8)
        for _ in range(5):
            idx.query_scan(zero, tb, R)
        idx.close()


KNN_ROOF_PAIRS_PER_S = 2e11   # estimated: 3 * 128 component operations a pair, 32 packed non-FMA f32 operations per clock and SIMD


def knn_leg(iters, res, torch):
    """Refine.knn / knn_device over 10^6 rows of dim 128 beside a chunked torch |x|^2 - 2 q.x + topk on the same rows"""
    if torch is None:
        print("knn leg: needs torch on the GPU (the rows are made there and the yardstick is torch)", flush=True)
        return
    n, dim, chunk = 1_000_000, 128, 1 << 18
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((n, dim), generator=gen, device="cuda", dtype=torch.float32)
    out = res.setdefault("knn", {"rows": n, "dim": dim, "R": R, "roof_pairs_per_s_estimated": KNN_ROOF_PAIRS_PER_S})
    for dtype in ("f32", "f16"):
        st = pyqadc.Refine(dim, dtype)
        st.add_device(x, 0)
        held = x if dtype == "f32" else x.half().float()                   # the values the store holds
        norms = (held * held).sum(1)

        def torch_route(q):
            best_d = best_k = None
            for first in range(0, n, chunk):
                d = norms[first:first + chunk][None, :] - 2.0 * (q @ held[first:first + chunk].T)
                dd, kk = torch.topk(d, R, dim=1, largest=False)
                kk = kk + first
                if best_d is not None:
                    dd, kk = torch.cat([best_d, dd], 1), torch.cat([best_k, kk], 1)
                    dd, pick = torch.topk(dd, R, dim=1, largest=False)
                    kk = torch.gather(kk, 1, pick)
                best_d, best_k = dd, kk
            torch.cuda.synchronize()
            return best_k

        for nq in (1, 32, 1024):
            q = torch.randn((nq, dim), generator=gen, device="cuda", dtype=torch.float32)
            q_host = q.cpu().numpy()
            its = max(3, iters if nq < 1024 else iters // 2)
            med_d, best_d = timed(lambda: st.knn_device(q, R), its)
            med_h, _ = timed(lambda: st.knn(q_host, R), its)
            med_t, _ = timed(lambda: torch_route(q), its)
            keys = st.knn_device(q, R)[0].cpu().numpy().view(np.uint32)
            want = torch_route(q).cpu().numpy()
            agree = float(np.mean([set(a.tolist()) == set(b.tolist()) for a, b in zip(keys, want)]))
            pairs = nq * n / med_d
            out["%s_nq%d" % (dtype, nq)] = {"knn_device_ms": med_d * 1e3, "knn_device_best_ms": best_d * 1e3, "knn_host_arrays_ms": med_h * 1e3,
                                            "torch_route_ms": med_t * 1e3, "pairs_per_s": pairs, "share_of_estimated_roof": pairs / KNN_ROOF_PAIRS_PER_S,
                                            "queries_whose_key_sets_agree": agree}
            print("knn %s, 10^6 x 128, nq %4d, R %d: knn_device %.3f ms (best %.3f; host arrays %.3f) = %.3g pairs/s = %.3f of the estimated roof; "
                  "torch |x|^2 - 2 q.x + topk %.3f ms; key sets agree on %.3f of the queries"
                  % (dtype, nq, R, med_d * 1e3, best_d * 1e3, med_h * 1e3, pairs, pairs / KNN_ROOF_PAIRS_PER_S, med_t * 1e3, agree), flush=True)
        st.close()
        del held, norms


def refine_ip_leg(res, torch, runs=3):
    """Every exact call of a refine store under "ip" beside the same call under "l2" — the same store, the same process, `runs` + `runs`
    alternated runs after one warm-up of each: the L2 call of the same build is the reference and its own spread the margin"""
    if torch is None:
        print("refine_ip leg: needs torch on the GPU (the rows are made there)", flush=True)
        return
    n, dim, K, ma = 1_000_000, 128, 256, 24
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((n, dim), generator=gen, device="cuda", dtype=torch.float32)
    q_all = torch.randn((1024, dim), generator=gen, device="cuda", dtype=torch.float32)
    centroids = x[torch.randperm(n, generator=gen, device="cuda")[:K]].contiguous()
    part_of = torch.cat([torch.cdist(x[i:i + (1 << 17)], centroids).argmin(1) for i in range(0, n, 1 << 17)]).cpu().numpy()
    rng = np.random.default_rng(11)
    labels = [np.nonzero(part_of == k)[0].astype(np.uint32) for k in range(K)]
    idx = pyqadc.AdcIndex(8, 8)
    idx.add_partitions([rng.integers(0, 256, (len(l), 8), dtype=np.uint8) for l in labels], labels)   # (codes no call of this leg reads)
    idx.set_pq(rng.normal(size=(8, 256, dim // 8)).astype(np.float32))
    idx.set_coarse(centroids.cpu().numpy())
    cand = {r_in: torch.from_numpy(rng.integers(0, n, (1024, r_in)).astype(np.int32)).to(dev) for r_in in (400, 1000)}
    out = res.setdefault("refine_ip", {"rows": n, "dim": dim, "R": R, "K": K, "ma": ma, "runs_per_arm": runs})

    def both(st, call):
        """call() under "ip" and under "l2" in turn -> (times ip, times l2), seconds"""
        def arm(metric):
            st.set_metric(metric)
            t0 = time.perf_counter()
            call()
            return time.perf_counter() - t0
        arm("ip"), arm("l2")
        t = {"ip": [], "l2": []}
        for _ in range(runs):
            for metric in ("ip", "l2"):
                t[metric].append(arm(metric))
        return t["ip"], t["l2"]

    for dtype in ("f32", "f16", "sq8"):
        if dtype == "sq8":
            vmin, step = pyqadc.refine_sq_range_device(x)
            st = pyqadc.Refine(dim, "sq8", vmin=vmin, step=step)
        else:
            st = pyqadc.Refine(dim, dtype)
        st.add_device(x, 0)
        calls = [("knn_device_nq%d" % nq, (lambda tq: lambda: st.knn_device(tq, R))(q_all[:nq].contiguous())) for nq in (1024, 32, 1)]
        calls += [("rerank_device_rin%d" % r_in, (lambda k: lambda: st.rerank_device(q_all, k, R))(cand[r_in])) for r_in in (400, 1000)]
        calls.append(("search_exact_device_ma%d" % ma, lambda: idx.search_exact_device(q_all, ma, R, st)))
        for name, call in calls:
            t_ip, t_l2 = both(st, call)
            med_ip, med_l2 = float(np.median(t_ip)), float(np.median(t_l2))
            spread = max(t_l2) - min(t_l2)
            verdict = "no slower" if med_ip <= med_l2 + spread else "slower"
            out["%s_%s" % (dtype, name)] = {"ip_ms": [t * 1e3 for t in t_ip], "l2_ms": [t * 1e3 for t in t_l2], "ip_median_ms": med_ip * 1e3,
                                            "l2_median_ms": med_l2 * 1e3, "l2_spread_ms": spread * 1e3, "verdict": verdict}
            print("refine_ip %s %s: ip %.3f ms, l2 %.3f ms (medians of %d alternated runs; l2 ran %.3f .. %.3f): ip is %s than l2 within l2's spread"
                  % (dtype, name, med_ip * 1e3, med_l2 * 1e3, runs, min(t_l2) * 1e3, max(t_l2) * 1e3, verdict), flush=True)
        st.set_metric("ip")
        tq = q_all[:32].contiguous()
        keys = st.knn_device(tq, R)[0].cpu().numpy().view(np.uint32)
        want = torch.topk(tq @ x.T, R, dim=1).indices.cpu().numpy()
        share = float(np.mean([len(set(a.tolist()) & set(b.tolist())) for a, b in zip(keys, want)])) / R
        out["%s_share_of_keys_in_common_with_torch_topk" % dtype] = share
        print("refine_ip %s: knn under ip shares %.4f of its keys with torch's (q @ x.T).topk over the float rows (32 queries)" % (dtype, share),
              flush=True)
        st.close()
    idx.close()


def refine_range_leg(iters, res, torch):
    """Exact range search over 10^6 rows of dim 128, F32 and F16, in one process:
    (a) Refine.range_device under radii that keep about 100 and about 10^4 rows per query beside Refine.knn_device(R = 100) at the same
        shapes — the same distance pass without the mid-selects — three rounds of each, so that knn's own run-to-run spread is on record;
        and a torch route (|x|^2 - 2 q.x, a compare, nonzero, a sort) as other arithmetic, not a parity target;
    (b) Refine.rerank_range_device on 1024 x 1000 candidates beside Refine.rerank_device at r_in = 1000, R = 1000."""
    if torch is None:
        print("refine_range leg: needs torch on the GPU (the rows are made there)", flush=True)
        return
    n, dim, chunk = 1_000_000, 128, 1 << 18
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((n, dim), generator=gen, device="cuda", dtype=torch.float32)
    out = res.setdefault("refine_range", {"rows": n, "dim": dim})
    for dtype in ("f32", "f16"):
        st = pyqadc.Refine(dim, dtype)
        st.add_device(x, 0)
        held = x if dtype == "f32" else x.half().float()
        norms = (held * held).sum(1)

        def torch_route(q, radius):
            r = torch.from_numpy(radius).cuda()
            qn = (q * q).sum(1)
            rows = []
            for first in range(0, n, chunk):
                d = qn[:, None] + norms[first:first + chunk][None, :] - 2.0 * (q @ held[first:first + chunk].T)
                hit = torch.nonzero(d < r[:, None])
                rows.append(torch.stack([hit[:, 0].double(), d[hit[:, 0], hit[:, 1]].double(), (hit[:, 1] + first).double()], 1))
            rows = torch.cat(rows)
            order = torch.argsort(rows[:, 1], stable=True)
            order = order[torch.argsort(rows[order, 0], stable=True)]
            torch.cuda.synchronize()
            return rows[order]

        for nq in (1024, 32, 1):
            q = torch.randn((nq, dim), generator=gen, device="cuda", dtype=torch.float32)
            its = max(3, iters if nq < 1024 else iters // 2)
            _, kd, _ = st.knn_device(q, R)
            r100 = np.nextafter(kd[:, R - 1].cpu().numpy(), np.float32(np.inf))            # keeps the knn's 100 rows (and their ties)
            sample = held[torch.randint(0, n, (100_000,), generator=gen, device="cuda")]
            ds = (q * q).sum(1)[:, None] + (sample * sample).sum(1)[None, :] - 2.0 * (q @ sample.T)
            r1e4 = torch.kthvalue(ds, 1000, dim=1).values.cpu().numpy().astype(np.float32)   # 1 % of a sample: about 10^4 of 10^6 rows
            entry = {}
            knn_rounds, rng_rounds = [], []
            for _ in range(3):
                mk, mr = alternated(lambda: st.knn_device(q, R), lambda: st.range_device(q, r100), its)
                knn_rounds.append(mk * 1e3)
                rng_rounds.append(mr * 1e3)
            before = st.range_reruns()
            big, _ = timed(lambda: st.range_device(q, r1e4), its)
            reruns = st.range_reruns() - before
            lims100 = st.range_device(q, r100)[0]
            lims1e4, k1e4, _ = st.range_device(q, r1e4)
            t_its = 2 if nq == 1024 else its
            med_t, _ = timed(lambda: torch_route(q, r100), t_its, warmup=1)
            want = torch_route(q, r1e4)
            agree = "%d against %d" % (int(want.shape[0]), int(lims1e4[-1]))   # (other arithmetic: rows at the radius may fall either way)
            entry.update({"knn_device_R100_ms_rounds": knn_rounds, "range_device_keep100_ms_rounds": rng_rounds,
                          "knn_spread_ms": max(knn_rounds) - min(knn_rounds), "range_minus_knn_ms": float(np.median(rng_rounds) - np.median(knn_rounds)),
                          "rows_kept_per_query_keep100": float(lims100[-1]) / nq, "range_device_keep1e4_ms": big * 1e3,
                          "rows_kept_per_query_keep1e4": float(lims1e4[-1]) / nq, "reruns_per_call_keep1e4": reruns / (its + 2),
                          "torch_route_keep100_ms": med_t * 1e3, "torch_route_rows_against_range_rows_keep1e4": agree})
            out["%s_nq%d" % (dtype, nq)] = entry
            print("range %s, 10^6 x 128, nq %4d: knn_device(R=100) %s ms; range_device keeping %.1f rows/query %s ms (range - knn %.3f ms, knn's "
                  "spread %.3f ms); keeping %.0f rows/query %.3f ms (%.1f re-runs per call); torch route %.3f ms; rows the torch route and range keep: %s"
                  % (dtype, nq, ["%.3f" % v for v in knn_rounds], entry["rows_kept_per_query_keep100"], ["%.3f" % v for v in rng_rounds],
                     entry["range_minus_knn_ms"], entry["knn_spread_ms"], entry["rows_kept_per_query_keep1e4"], big * 1e3,
                     entry["reruns_per_call_keep1e4"], med_t * 1e3, agree), flush=True)
        # (b) candidates: 1024 x 1000 random keys
        nq, r_in = 1024, 1000
        q = torch.randn((nq, dim), generator=gen, device="cuda", dtype=torch.float32)
        keys = torch.randint(0, n, (nq, r_in), generator=gen, device="cuda", dtype=torch.int32)
        flat = keys.reshape(-1).contiguous()
        lims = np.arange(nq + 1, dtype=np.uint64) * r_in
        rr_rounds, rk_rounds = [], []
        for _ in range(3):
            mk, mr = alternated(lambda: st.rerank_device(q, keys, r_in), lambda: st.rerank_range_device(q, lims, flat, np.float32(np.inf)), max(3, iters))
            rk_rounds.append(mk * 1e3)
            rr_rounds.append(mr * 1e3)
        a, b = st.rerank_device(q, keys, r_in), st.rerank_range_device(q, lims, flat, np.float32(np.inf))
        same = bool(np.array_equal(np.cumsum(a[2].cpu().numpy()), b[0][1:])) and bool(torch.equal(a[0][0, :int(b[0][1])], b[1][:int(b[0][1])]))
        out["%s_rerank_1024x1000" % dtype] = {"rerank_device_ms_rounds": rk_rounds, "rerank_range_device_ms_rounds": rr_rounds, "results_agree": same}
        print("rerank %s, 1024 x 1000 candidates: rerank_device(R = r_in) %s ms; rerank_range_device(+inf) %s ms; results agree: %s"
              % (dtype, ["%.3f" % v for v in rk_rounds], ["%.3f" % v for v in rr_rounds], same), flush=True)
        st.close()
        del held, norms


def refine_range_search_leg(idx, vectors, queries, ma, iters, res):
    """AdcIndex.range_search_refined_device on the IVF index of search_legs (10^6 codes, K = 256, ma = 24, 1024 queries) beside the host
    route it replaces — range_search to the host, every query padded to 8192 candidates (the rest dropped), Refine.rerank with
    R = r_in, a threshold in numpy — and the range recall against Refine.range as ground truth for adc_radius = c * radius."""
    import torch
    nq, dim = queries.shape
    out = res.setdefault("refine_range", {})
    st = pyqadc.Refine(dim, "f32")
    st.add(vectors, 0)
    dq = torch.from_numpy(queries).cuda()
    _, kd, _ = st.knn_device(dq, R)
    radius = np.nextafter(kd[:, R - 1].cpu().numpy(), np.float32(np.inf))                   # the exact radius of each query's 100 nearest rows
    _, vals, _, _ = idx.search(queries, ma, 1000)
    adc_radius = vals.max(axis=1).astype(np.float32)                                        # about 1000 ADC rows per query
    MAXIN = pyqadc.QADC_REFINE_MAX_IN

    def host_route():
        lims, keys, _ = idx.range_search(queries, ma, adc_radius)
        padded = np.full((nq, MAXIN), 0xFFFFFFFF, np.uint32)
        counts = np.minimum(np.diff(lims), MAXIN).astype(np.int32)
        for i in range(nq):
            padded[i, :counts[i]] = keys[lims[i]:lims[i] + counts[i]]
        k, d, s, _ = st.rerank(queries, padded, MAXIN, counts=counts)
        keep = d < radius[:, None]
        return k, keep, int((np.diff(lims) > MAXIN).sum())

    dev = lambda: idx.range_search_refined_device(dq, ma, adc_radius, radius, st)
    lims, keys, dist, missing = dev()
    hk, keep, truncated = host_route()
    agree = all(np.array_equal(hk[i][keep[i]], keys[lims[i]:lims[i + 1]].cpu().numpy().view(np.uint32)) for i in range(0, nq, 37))
    its = max(3, iters // 2)
    med_d, _ = timed(dev, its)
    med_h, _ = timed(host_route, 2, warmup=1)
    out["range_search_refined"] = {"device_chain_ms": med_d * 1e3, "host_route_ms": med_h * 1e3, "queries_the_host_route_truncates": truncated,
                                   "adc_rows_per_query": float(idx.range_search(queries, ma, adc_radius)[0][-1]) / nq,
                                   "rows_kept_per_query": float(lims[-1]) / nq, "missing": missing, "sampled_queries_agree": bool(agree)}
    print("range_search_refined_device, 10^6 codes K=256 ma=%d, %d queries (%.0f ADC rows/query, %.1f kept): %.2f ms; the host route (collect, pad to "
          "%d, rerank, threshold) %.2f ms, truncating %d queries; sampled queries agree: %s"
          % (ma, nq, out["range_search_refined"]["adc_rows_per_query"], float(lims[-1]) / nq, med_d * 1e3, MAXIN, med_h * 1e3, truncated, agree), flush=True)
    # range recall: the rows truly within the radius (Refine.range) that the composition returns under adc_radius = c * radius
    sub = 128
    tl, tk, _ = st.range_device(dq[:sub].contiguous(), radius[:sub])
    tk = tk.cpu().numpy()
    recall = {}
    for c in (0.8, 1.0, 1.2, 1.5, 2.0):
        gl, gk, _, _ = idx.range_search_refined_device(dq[:sub].contiguous(), ma, (radius[:sub] * np.float32(c)).astype(np.float32), radius[:sub], st)
        gk = gk.cpu().numpy()
        hit = sum(len(np.intersect1d(tk[tl[i]:tl[i + 1]], gk[gl[i]:gl[i + 1]])) for i in range(sub))
        recall["%.1f" % c] = hit / max(1, int(tl[-1]))
    out["range_recall_by_c"] = recall
    print("range recall of range_search_refined against Refine.range (%d queries, %.1f true rows each), adc_radius = c * radius: %s"
          % (sub, float(tl[-1]) / sub, recall), flush=True)
    st.close()


VALU_FMA_PER_S = 157.3e12 / 2   # the FP32 vector peak (spec), in fused multiply-adds


def decode_leg(bits, iters, res, torch):
    """PQ decode and reconstruction at 16x4, 8x8 or 2x16, dim 128, with and without a rotation:
    (a) pq_decode_device on 10^6 x 128 with K = 256 coarse centroids, codes and assignment in device memory;
    (b) reconstruct_device on the keys of a 1024 x 100 search_device over 10^6 encoded vectors (K = 256, ma = 8).
    Each against the route it replaces, alternated in the same process: the codes fetched to the host (read_partition), a numpy gather
    (+ a matmul under a rotation, + the coarse centroid), and the upload of the result.  Whole synchronous calls under a host clock."""
    if torch is None:
        raise SystemExit("the decode leg hands torch tensors over: torch with a GPU is required")
    nsq = {4: 16, 8: 8, 16: 2}[bits]
    dim, n, K, nq, ma = 128, 1_000_000, 256, 1024, 8
    ds, cent = dim // nsq, 1 << bits
    code_bytes = nsq // 2 if bits == 4 else nsq * bits // 8
    rng = np.random.default_rng(7)
    coarse = (rng.normal(size=(K, dim)) * 4).astype(np.float32)
    cb = rng.normal(size=(nsq, cent, ds)).astype(np.float32)
    rot = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(dim, dim)))[0], np.float32)
    vec = (coarse[rng.integers(0, K, n)] + rng.normal(size=(n, dim))).astype(np.float32)
    labels = rng.permutation(n).astype(np.uint32)

    def unpacked(codes):
        c = np.asarray(codes)
        if bits == 4:
            out = np.empty((c.shape[0], nsq), np.int64)
            out[:, 0::2], out[:, 1::2] = c & 15, c >> 4
            return out
        return c.astype(np.int64)

    def host_decode(codes, assign, rotation):
        a = unpacked(codes)
        y = np.concatenate([cb[m][a[:, m]] for m in range(nsq)], axis=1)
        if rotation is not None:
            y = y @ rotation                                               # z[c] = sum_r y[r] rotation[r][c]
        return y + coarse[assign]

    for rotated in (False, True):
        tag = "decode%d_%s" % (bits, "opq" if rotated else "pq")
        rotation = rot if rotated else None
        if bits == 4:
            base = pyqadc.Index(nsq)
        else:
            base = pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)
        base.set_pq(cb)
        if rotated:
            base.set_rotation(rot)
        base.set_coarse(coarse)
        base.add_vectors(vec, labels=labels)
        if bits == 4:
            base.finalize(0.01)
        idx = pyqadc.AdcIndex.view_of(base) if bits == 4 else base
        parts = [base.read_partition(p) for p in range(K)]
        codes = np.concatenate([c for c, _ in parts])
        assign = np.concatenate([np.full(len(c), p, np.int32) for p, (c, _) in enumerate(parts)])
        # (a) stateless
        d_codes = torch.from_numpy(np.ascontiguousarray(codes).view(np.uint8).reshape(n, code_bytes)).cuda()
        d_assign = torch.from_numpy(assign).cuda()
        d_out = torch.zeros((n, dim), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gpu = lambda: pyqadc.pq_decode_device(cb, d_codes, assign=d_assign, coarse=coarse, rotation=rotation, out=d_out)

        def route():
            c = d_codes.cpu().numpy()                                      # what read_partition costs: the codes to the host
            c = c.view("<u2").reshape(n, nsq) if bits == 16 else c
            t = torch.from_numpy(host_decode(c, assign, rotation).astype(np.float32)).cuda()
            torch.cuda.synchronize()
            return t
        got, want = gpu().cpu().numpy(), route().cpu().numpy()
        err = float(np.abs(got - want).max())
        assert err < 1e-3 * (1 + float(np.abs(want).max())), "the two routes disagree: %g" % err
        med_r, med_g = alternated(route, gpu, max(3, iters // 2), warmup=1)
        res[tag + "_stateless_ms"] = med_g * 1e3
        res[tag + "_stateless_route_ms"] = med_r * 1e3
        res[tag + "_stateless_rows_per_s"] = n / med_g
        res[tag + "_stateless_out_bytes_per_s"] = n * dim * 4 / med_g
        line = "decode %dx%d%s, 10^6 x 128: pq_decode_device %.3f ms = %.3g rows/s = %.3g B/s written; host route %.1f ms (x%.0f)" % (
            nsq, bits, " + rotation" if rotated else "", med_g * 1e3, n / med_g, n * dim * 4 / med_g, med_r * 1e3, med_r / med_g)
        if rotated:
            res[tag + "_stateless_fma_per_s"] = n * dim * dim / med_g
            res[tag + "_stateless_valu_peak_share"] = n * dim * dim / med_g / VALU_FMA_PER_S
            line += "; %.3g fmaf/s = %.3f of the FP32 vector peak" % (n * dim * dim / med_g, n * dim * dim / med_g / VALU_FMA_PER_S)
        else:
            share = (n * dim * 4 + n * code_bytes) / med_g / HBM_BPS
            res[tag + "_stateless_hbm_peak_share"] = share
            line += "; out + code bytes = %.3f of the HBM peak" % share
        print(line, flush=True)
        # (b) the keys of a search
        q = torch.from_numpy((coarse[rng.integers(0, K, nq)] + rng.normal(size=(nq, dim))).astype(np.float32)).cuda()
        keys, _, _ = idx.search_device(q, ma, R)
        rec = lambda: idx.reconstruct_device(keys)

        def lookup_route():
            got = [base.read_partition(p) for p in range(K)]
            all_codes = np.concatenate([c for c, _ in got])
            all_labels = np.concatenate([l for _, l in got])
            owner = np.concatenate([np.full(len(c), p, np.int32) for p, (c, _) in enumerate(got)])
            order = np.argsort(all_labels, kind="stable")
            k = keys.cpu().numpy().view(np.uint32).reshape(-1)
            rows = order[np.minimum(np.searchsorted(all_labels[order], k), len(order) - 1)]
            t = torch.from_numpy(host_decode(all_codes[rows], owner[rows], rotation).astype(np.float32)).cuda()
            torch.cuda.synchronize()
            return t
        got, where = rec()
        found = (where.reshape(-1) != -1).cpu().numpy()
        want = lookup_route().cpu().numpy()
        err = float(np.abs(got.reshape(-1, dim).cpu().numpy()[found] - want[found]).max())
        assert err < 1e-3 * (1 + float(np.abs(want).max())), "the two lookup routes disagree: %g" % err
        med_r, med_g = alternated(lookup_route, rec, max(3, iters // 2), warmup=1)
        res[tag + "_reconstruct_ms"] = med_g * 1e3
        res[tag + "_reconstruct_route_ms"] = med_r * 1e3
        res[tag + "_reconstruct_rows_per_s"] = nq * R / med_g
        print("decode %dx%d%s, the %d keys of a 1024 x 100 search over 10^6 rows: reconstruct_device %.3f ms = %.3g rows/s = %.3g B/s written; "
              "read_partition + numpy route %.1f ms (x%.0f)" % (nsq, bits, " + rotation" if rotated else "", nq * R, med_g * 1e3, nq * R / med_g,
                                                               nq * R * dim * 4 / med_g, med_r * 1e3, med_r / med_g), flush=True)
        if bits == 4:
            idx.close()
        base.close()
        del d_codes, d_assign, d_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=None)
    ap.add_argument("--bits", type=int, default=8, choices=(4, 8, 16))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trained-codebooks", action="store_true")
    ap.add_argument("--repair", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    global TRAINED, REPAIR, PARENT_LIB
    TRAINED, REPAIR, PARENT_LIB = a.trained_codebooks, a.repair, a.parent_lib
    if a.legs is None:
        a.legs = "flat1e8,batch32,lone1e6,ivf,cpu,ivf_search,lone_search" if a.bits == 8 else "lone,ivf_search"
    legs = a.legs.split(",")
    if a.bits != 8:
        res = {"R": R, "sum_mode": 1, "bits": a.bits, "cpus_allowed": len(os.sched_getaffinity(0))}
        if "decode" in legs:                                               # (torch's HIP runtime has to come up before the library's)
            import torch
            torch.zeros(1, device="cuda")
            decode_leg(a.bits, a.iters, res, torch)
        (view_legs if a.bits == 4 else word_legs)([l for l in legs if l != "decode"], a.iters, res)
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    torch = None
    if "ivf" in legs or "filter" in legs or "refine" in legs or "keyed" in legs or "knn" in legs or "decode" in legs or "refine_sq" in legs or "refine_range" in legs or "probe" in legs or "refine_ip" in legs:   # the device-memory arm hands a torch tensor over; torch's HIP runtime has to come up before the library's
        try:
            import torch
            torch.zeros(1, device="cuda")
        except Exception:
            torch = None
    rng = np.random.default_rng(0)
    res = {"R": R, "sum_mode": 1, "cpus_allowed": len(os.sched_getaffinity(0))}

    if "flat1e8" in legs or "batch32" in legs:
        n = 100_000_000
        codes = rng.integers(0, 256, (n, 8), dtype=np.uint8)
        idx = pyqadc.AdcIndex(8, 8)
        idx.add_partitions([codes])
        del codes
        if "flat1e8" in legs:
            tb = tables_for(rng, 1, 1)
            med, best = timed(lambda: idx.query_scan(np.zeros((1, 1), np.int32), tb, R), a.iters)
            res["flat1e8_one_query_ms"] = med * 1e3
            res["flat1e8_codes_per_s"] = n / med
            res["flat1e8_hbm_roofline_share"] = n * 8 / med / HBM_BPS
            print("flat 8x8, 10^8 codes, 1 query/call: %.3f ms (best %.3f) = %.3g codes/s = %.3f of the HBM roofline"
                  % (med * 1e3, best * 1e3, n / med, n * 8 / med / HBM_BPS), flush=True)
        if "batch32" in legs:
            tb = tables_for(rng, 32, 1)
            med, best = timed(lambda: idx.query_scan(np.zeros((32, 1), np.int32), tb, R), max(3, a.iters // 2))
            res["flat1e8_batch32_ms"] = med * 1e3
            res["flat1e8_batch32_query_codes_per_s"] = 32 * n / med
            print("flat 8x8, 10^8 codes, 32 queries/call: %.3f ms (best %.3f) = %.3g query-codes/s"
                  % (med * 1e3, best * 1e3, 32 * n / med), flush=True)
        idx.close()

    n1 = 1_000_000
    codes1 = rng.integers(0, 256, (n1, 8), dtype=np.uint8)
    tb1 = tables_for(rng, 1, 1)
    if "lone1e6" in legs:
        idx = pyqadc.AdcIndex(8, 8)
        idx.add_partitions([codes1])
        med, best = timed(lambda: idx.query_scan(np.zeros((1, 1), np.int32), tb1, R), max(a.iters, 50), warmup=5)
        res["lone1e6_call_us"] = med * 1e6
        print("flat 8x8, 10^6 codes, one synchronous query: %.1f us (best %.1f)" % (med * 1e6, best * 1e6), flush=True)
        idx.close()
    if "cpu" in legs:
        import pyoracle as po
        parts = [codes1]
        tt = tb1.reshape(1, -1)
        med, _ = timed(lambda: po.scan_standard_u8(8, parts, None, tt, R), 5, warmup=1)
        res["cpu_scan_standard_u8_8_restatement_us"] = med * 1e6
        print("CPU scan_standard<uint8_t,8>, 10^6 codes, 1 thread (C restatement, -O2): %.1f us" % (med * 1e6), flush=True)
        if po.have_ref_float():
            med, _ = timed(lambda: po.reff_scan_standard_u8(8, parts, None, tt, R), 5, warmup=1)
            res["cpu_scan_standard_u8_8_reference_build_us"] = med * 1e6
            print("CPU scan_standard<uint8_t,8>, 10^6 codes, 1 thread (reference build, -O3 -ffast-math AVX2): %.1f us"
                  % (med * 1e6), flush=True)
        if "lone1e6_call_us" in res:
            cpu = min(v for k, v in res.items() if k.startswith("cpu_scan_standard"))
            res["lone1e6_speedup_vs_fastest_cpu_thread"] = cpu / res["lone1e6_call_us"]
            print("GPU one-query call vs the faster single CPU thread: %.1fx" % res["lone1e6_speedup_vs_fastest_cpu_thread"])
    if "ivf" in legs:
        K, ma, nq = 256, 24, 1024
        part_of = rng.integers(0, K, n1)
        parts = [codes1[part_of == k] for k in range(K)]
        labels = [np.nonzero(part_of == k)[0].astype(np.uint32) for k in range(K)]
        idx = pyqadc.AdcIndex(8, 8)
        idx.add_partitions(parts, labels)
        assign = np.stack([rng.permutation(K)[:ma] for _ in range(nq)]).astype(np.int32)
        tb = tables_for(rng, nq, ma)
        med, best = timed(lambda: idx.query_scan(assign, tb, R), max(3, a.iters // 2), warmup=1)
        probed = sum(len(parts[k]) for k in assign.ravel())
        res["ivf_batch1024_ms"] = med * 1e3
        res["ivf_us_per_query"] = med * 1e6 / nq
        res["ivf_table_bytes_uploaded_per_call"] = int(tb.nbytes)
        res["ivf_codes_probed_per_call"] = int(probed)
        print("IVF K=256 ma=24, 1024 queries/call (with %.0f MB of float tables uploaded): %.2f ms = %.1f us/query"
              % (tb.nbytes / 1e6, med * 1e3, med * 1e6 / nq), flush=True)
        if torch is not None:
            d_tb = torch.from_numpy(tb).cuda()
            torch.cuda.synchronize()
            host = lambda: idx.query_scan(assign, tb, R)
            dev = lambda: idx.query_scan_device(assign, d_tb, R)
            got = dev()
            got = (got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy())
            assert same_heaps(host(), got), "query_scan and query_scan_device disagree"
            med_h, med_d = alternated(host, dev, max(3, a.iters // 2), warmup=1)
            res["ivf_query_scan_upload_ms"] = med_h * 1e3
            res["ivf_query_scan_device_ms"] = med_d * 1e3
            print("the same alternated with query_scan_device (tables and heaps stay in device memory): %.2f ms against %.2f ms"
                  % (med_d * 1e3, med_h * 1e3), flush=True)
        idx.close()
    if "ivf_search" in legs or "lone_search" in legs or "filter" in legs or "qfilter" in legs or "refine" in legs or "range" in legs or "keyed" in legs or "refine_sq" in legs or "refine_range" in legs or "probe" in legs:
        search_legs(legs, a.iters, res)
    if "filter" in legs:
        filter_leg(8, a.iters, res, torch)
    if "add" in legs:
        add_leg(8, a.iters, res)
    if "remove" in legs:
        remove_leg(8, a.iters, res)
    if "train" in legs:
        train_leg(8, a.iters, res)
    if "opq" in legs:
        opq_leg(8, a.iters, res)
    if "seed" in legs:
        seed_leg(8, a.iters, res)
    if "knn" in legs:
        knn_leg(a.iters, res, torch)
    if "refine_range" in legs:
        refine_range_leg(a.iters, res, torch)
    if "refine_ip" in legs:
        refine_ip_leg(res, torch)
    if "decode" in legs:
        decode_leg(8, a.iters, res, torch)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
