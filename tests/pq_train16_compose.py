"""What PQ training at 16 bits (qadc_pq_train16_host, qadc_pq_update16_host, the host twins pq_train16_iterations / pq_update16)
must compute, composed from the oracle's functions and numpy.  The assignment is adc16_encode_compose.codes16 (the oracle's
cross_dists + select_k_neighbors(.., 1) on the 65536 rows of a sub-quantizer).  The update sorts the vectors by code with a
stable argsort, so that a cluster is a run in ascending vector index, and sums each run one member at a time in float32; a mask
per centroid (pq_train_compose.update_slice) would cost 65536 * n here.  Every float is compared bit for bit."""
import numpy as np

import adc16_encode_compose as a16e

K16 = 65536


def seed_rows(vectors, sq_count, rows):
    """the sub-vectors of the given 65536 rows -> float32 [sq_count][65536][dsub]"""
    v = np.ascontiguousarray(vectors, np.float32)
    ds = v.shape[1] // sq_count
    assert len(rows) == K16
    return np.ascontiguousarray(v[np.asarray(rows)].reshape(K16, sq_count, ds).transpose(1, 0, 2))


def update_slice(sub, assign, div_mode=1, descending=False):
    """sub [n][ds], assign [n] in [0, 65536) -> (centroids float32 [65536][ds], counts uint32 [65536]): centroid k = (members of k
    summed into one running float32 starting at 0.0f, in ascending vector index — descending on request) * (float32(1) / count),
    or / count; an empty cluster is 0 * inf = NaN, or 0 / 0"""
    sub = np.ascontiguousarray(sub, np.float32)
    assign = np.asarray(assign).astype(np.int64)
    n, ds = sub.shape
    order = np.argsort(assign, kind="stable")
    if descending:
        order = order[::-1]
        order = order[np.argsort(assign[order], kind="stable")]              # runs by code, descending index inside a run
    counts = np.bincount(assign, minlength=K16).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(counts)])
    total = np.zeros((K16, ds), np.float32)
    srt = sub[order]
    zero = np.zeros((1, ds), np.float32)
    with np.errstate(all="ignore"):
        # a long run: cumsum adds one by one, in order (as pq_train_compose.update_slice)
        for k in np.flatnonzero(counts > 64):
            total[k] = np.cumsum(np.concatenate([zero, srt[first[k]:first[k + 1]]]), axis=0, dtype=np.float32)[-1]
        # the short ones together: step t adds the t-th member of every cluster that has one, so each running sum still takes its
        # members one by one, in order
        alive = np.flatnonzero((counts > 0) & (counts <= 64))
        t = 0
        while len(alive):
            total[alive] = total[alive] + srt[first[alive] + t]
            t += 1
            alive = alive[counts[alive] > t]
        cnt = counts.astype(np.float32)[:, None]
        out = total * (np.float32(1) / cnt) if div_mode else total / cnt
    return np.ascontiguousarray(out, np.float32), counts.astype(np.uint32)


def update(x, codes, div_mode=1, descending=False):
    """x [n][dim], codes [n][nsq] -> (codebooks [nsq][65536][ds], counts [nsq][65536])"""
    x = np.ascontiguousarray(x, np.float32)
    nsq = codes.shape[1]
    ds = x.shape[1] // nsq
    cbs, cnts = zip(*(update_slice(x[:, m * ds:(m + 1) * ds], codes[:, m], div_mode, descending) for m in range(nsq)))
    return np.stack(cbs), np.stack(cnts)


def train(po, x, seed, iters, div_mode=1, sum_mode=1, descending=False):
    """x [n][dim]: the vectors as the quantizer sees them (already residuals, already rotated).  -> (codebooks, codes uint16
    [n][nsq] of the last round, the codebooks of before the last update)"""
    x = np.ascontiguousarray(x, np.float32)
    cb = np.array(seed, np.float32, order="C", copy=True)
    codes = np.zeros((x.shape[0], cb.shape[0]), np.uint16)
    before = cb.copy()
    for _ in range(iters):
        before = cb.copy()
        codes = a16e.codes16(po, cb, x, sum_mode)
        cb = update(x, codes, div_mode, descending)[0]
    return cb, codes, before


def empty_count(codebooks):
    return int(np.isnan(codebooks).any(axis=2).sum())


def reconstruction_error(x, codebooks, codes):
    """sum ||x - codebook[code]||^2 in float64"""
    nsq, _, ds = codebooks.shape
    x = np.asarray(x, np.float64)
    err = 0.0
    for m in range(nsq):
        err += float(((x[:, m * ds:(m + 1) * ds] - codebooks[m].astype(np.float64)[codes[:, m]]) ** 2).sum())
    return err
