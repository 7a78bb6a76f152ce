"""What a float-ADC view of a 4-bit index (pyqadc.AdcIndex.view_of, qadc_adc_index_create_view) must return, composed from the
oracle's functions: the heap arrays of scanner_simple::query_scan (db_query.cpp:26-45) over scan_4<M> (query_common.hpp:59-90).

Per probed partition, in assign order, scan_4 pushes (key, candidate) for every code, candidate = the code's float sum in the
compiled grouping (sum_mode 1) or in source order (0), key = the label, else key_base + position.  The heap holds R sentinels
(0, FLT_MAX - t) first and is therefore full: push accepts exactly when candidate < max, which is scan_4's own test against
bh.max().  So the arrays are heap_replay_f32 of the sentinels followed by all candidates.  Both halves are pinned to the
reference's binary elsewhere (tests/test_oracle_float_ref.py, the golden heaps); for R = 1 and sum_mode 1 the reference's own
compiled scan in scanner_simple's start state — one sentinel (0, FLT_MAX) in a full heap — is used directly where it is built."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def sentinels(R):
    return np.zeros(R, np.uint32), (FLT_MAX - np.arange(R, dtype=np.float32)).astype(np.float32)


def stream(po, M, parts, labels, tables, sum_mode=1, key_bases=None):
    """every (key, candidate) of one query in scan order: parts / labels / key_bases = the probed partitions in assign
    order, tables [ma][M*16]"""
    tables = np.ascontiguousarray(tables, np.float32).reshape(len(parts), M * 16)
    keys, vals = [], []
    for a, codes in enumerate(parts):
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, M // 2)
        n = codes.shape[0]
        vals.append(po.candidates_f32(M, codes, tables[a], sum_mode) if n else np.zeros(0, np.float32))
        if labels is not None and labels[a] is not None:
            keys.append(np.ascontiguousarray(labels[a], np.uint32))
        else:
            base = 0 if key_bases is None else int(key_bases[a])
            keys.append((np.arange(n, dtype=np.uint64) + base).astype(np.uint32))
    return np.concatenate(keys).astype(np.uint32), np.concatenate(vals).astype(np.float32)


def replay(po, keys, vals, R):
    """the heap arrays after the R sentinels and the given pushes"""
    sk, sv = sentinels(R)
    return po.heap_replay_f32(np.concatenate([sk, keys]), np.concatenate([sv, vals]), R)


def expected(po, M, parts, labels, tables, R, sum_mode=1, key_bases=None):
    """heap arrays (keys, values) of one query"""
    plain = key_bases is None or not any(key_bases)
    if R == 1 and sum_mode == 1 and plain and po.have_ref_float():
        tb = np.ascontiguousarray(tables, np.float32).reshape(len(parts), M * 16)
        return po.reff_scan4_start(M, [np.ascontiguousarray(p, np.uint8).reshape(-1, M // 2) for p in parts], labels, tb, 1)
    k, v = stream(po, M, parts, labels, tables, sum_mode, key_bases)
    return replay(po, k, v, R)


def assert_heap(got, want, q, what=""):
    keys, vals, sizes = got
    wk, wv = want
    n = int(sizes[q])
    assert n == len(wk), "%s query %d: heap size %d, expected %d" % (what, q, n, len(wk))
    assert np.array_equal(np.asarray(keys[q, :n]).view(np.uint32), wk), "%s query %d: keys differ" % (what, q)
    assert np.array_equal(np.asarray(vals[q, :n]).view(np.uint32), wv.view(np.uint32)), "%s query %d: values differ" % (what, q)


def rand_tables(rng, nq, ma, M, kind="dist"):
    """[nq][ma][M*16]; the kinds of tests/test_gpu_adc.py"""
    shape = (nq, ma, M, 16)
    if kind == "dist":           # squared-distance-like, continuous
        t = (rng.random(shape, dtype=np.float32) * np.float32(4.0)) ** 2
    elif kind == "ties":         # small integers: massive ties among candidates
        t = rng.integers(0, 4, shape).astype(np.float32)
    elif kind == "negative":
        t = rng.normal(size=shape).astype(np.float32)
    elif kind == "constant":
        t = np.full(shape, np.float32(1.5))
    elif kind == "nonfinite":    # NaN of either sign, +-inf, +-FLT_MAX in some entries
        t = rng.random(shape, dtype=np.float32)
        specials = np.array([np.nan, -np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX], np.float32)
        m = rng.random(shape) < 0.01
        t[m] = specials[rng.integers(0, len(specials), int(m.sum()))]
        neg = rng.random(shape) < 0.002
        t[neg] = -np.abs(np.float32(np.nan))        # NaN with the sign bit set
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(t.reshape(nq, ma, M * 16), np.float32)


def ivf_db(rng, M, K=64, n=60000):
    """K partitions of skewed sizes, six of them empty, labels = a permutation of 0 .. n-1"""
    w = rng.pareto(1.2, K) + 0.05
    w[rng.choice(K, 6, replace=False)] = 0
    sizes = np.floor(w / w.sum() * n).astype(np.int64)
    perm = rng.permutation(int(sizes.sum())).astype(np.uint32)
    parts, labels, o = [], [], 0
    for s in sizes:
        parts.append(rng.integers(0, 256, (int(s), M // 2), dtype=np.uint8))
        labels.append(perm[o:o + s].copy())
        o += s
    return parts, labels
