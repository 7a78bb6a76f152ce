"""What PQ training (qadc_pq_train_host, the host twin pq_train_iterations) must compute, composed from the oracle's functions and
numpy: per round and sub-space the oracle's cross_dists + select_k_neighbors(.., 1), as adc_compose.codes composes them, then a
sequential float32 sum per cluster in ascending vector index and a multiplication by float32(1) / count (div_mode 1) or a division
by the count (div_mode 0).  Every float is compared bit for bit."""
import numpy as np


def seed_rows(vectors, sq_count, bits, rows):
    """the sub-vectors of the given 2^bits rows -> float32 [sq_count][2^bits][dsub]"""
    v = np.ascontiguousarray(vectors, np.float32)
    K, ds = 1 << bits, v.shape[1] // sq_count
    assert len(rows) == K
    return np.ascontiguousarray(v[np.asarray(rows)].reshape(K, sq_count, ds).transpose(1, 0, 2))


def assign_slice(po, centroids, sub, sum_mode=1):
    """find_k_neighbors with k = 1 of the rows of sub [n][ds] among centroids [K][ds] -> int32 [n]"""
    return po.select_k_neighbors(po.cross_dists(centroids, sub, sum_mode), 1)[0][:, 0].astype(np.int32)


def update_slice(sub, assign, K, div_mode=1, descending=False):
    """centroid k = (members of k summed into one running float32 starting at 0.0f, in ascending vector index — descending on
    request) * (float32(1) / count), or / count; an empty cluster is 0 * inf = NaN, or 0 / 0"""
    sub = np.ascontiguousarray(sub, np.float32)
    out = np.zeros((K, sub.shape[1]), np.float32)
    zero = np.zeros((1, sub.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for k in range(K):
            mem = sub[assign == k]
            if descending:
                mem = mem[::-1]
            total = np.cumsum(np.concatenate([zero, mem]), axis=0, dtype=np.float32)[-1]      # cumsum adds one by one, in order
            cnt = np.float32(len(mem))
            out[k] = total * (np.float32(1) / cnt) if div_mode else total / cnt
    return out


def pack(assign, bits):
    """assign [n][sq_count] -> the encoder's layout: bytes, or nibbles with the even sub-quantizer in the low one"""
    a = np.ascontiguousarray(assign).astype(np.uint8)
    if bits == 8:
        return a
    return np.ascontiguousarray(a[:, 0::2] | (a[:, 1::2] << 4), np.uint8)


def unpack(codes, bits):
    c = np.ascontiguousarray(codes, np.uint8)
    if bits == 8:
        return c
    out = np.zeros((c.shape[0], c.shape[1] * 2), np.uint8)
    out[:, 0::2] = c & 15
    out[:, 1::2] = c >> 4
    return out


def train(po, x, seed, iters, div_mode=1, sum_mode=1, descending=False):
    """x [n][dim]: the vectors as the quantizer sees them (already residuals, already rotated).  -> (codebooks, codes of the last
    round in the encoder's layout, the codebooks of before the last update)"""
    x = np.ascontiguousarray(x, np.float32)
    cb = np.array(seed, np.float32, order="C", copy=True)
    nsq, K, ds = cb.shape
    bits = {16: 4, 256: 8}[K]
    assign = np.zeros((x.shape[0], nsq), np.int32)
    before = cb.copy()
    for _ in range(iters):
        before = cb.copy()
        for m in range(nsq):
            sub = np.ascontiguousarray(x[:, m * ds:(m + 1) * ds])
            assign[:, m] = assign_slice(po, cb[m], sub, sum_mode)
            cb[m] = update_slice(sub, assign[:, m], K, div_mode, descending)
    return cb, pack(assign, bits), before


def empty_count(codebooks):
    return int(np.isnan(codebooks).any(axis=2).sum())


def reconstruction_error(x, codebooks, codes):
    """sum ||x - codebook[code]||^2 in float64"""
    nsq, K, ds = codebooks.shape
    a = unpack(codes, {16: 4, 256: 8}[K])
    x = np.asarray(x, np.float64)
    err = 0.0
    for m in range(nsq):
        err += float(((x[:, m * ds:(m + 1) * ds] - codebooks[m].astype(np.float64)[a[:, m]]) ** 2).sum())
    return err
