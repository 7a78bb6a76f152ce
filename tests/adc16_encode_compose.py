"""What the 16-bit encoder (qadc_adc_encode16_host, pyqadc.adc_encode16) must return, composed from the oracle's functions:
encode_multiple_vectors for 65536 centroids per sub-quantizer is find_k_neighbors(k = 1) over the expansion distances, so a
code is po.select_k_neighbors — the reference's own capacity-1 heap as compiled, fed in centroid order — on po.cross_dists of
the sub-quantizer's 65536 rows.  adc_compose's assign and rotate come first, as in adc_compose.encode."""
import numpy as np

import adc_compose as ac


def codes16(po, codebooks, x, sum_mode=1):
    """vectors already made residuals and rotated, x [n][dim], codebooks [nsq][65536][ds] -> uint16 [n][nsq]"""
    nsq, rows, ds = codebooks.shape
    assert rows == 65536
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], nsq), np.uint16)
    with np.errstate(all="ignore"):
        for m in range(nsq):
            d = po.cross_dists(np.ascontiguousarray(codebooks[m]), np.ascontiguousarray(x[:, m * ds:(m + 1) * ds]), sum_mode)
            out[:, m] = po.select_k_neighbors(d, 1)[0][:, 0].astype(np.uint16)
    return out


def encode16(po, codebooks, vectors, coarse=None, rotation=None, sum_mode=1):
    """index_db::add_vectors' compute -> (assign int32 [n] or None, codes uint16 [n][nsq])"""
    v = np.ascontiguousarray(vectors, np.float32)
    a = None
    x = v
    if coarse is not None:
        a = ac.assign(po, v, coarse, 1, sum_mode)
        with np.errstate(all="ignore"):
            x = np.ascontiguousarray(v - np.asarray(coarse, np.float32)[a[:, 0]], np.float32)
    if rotation is not None:
        x = ac.rotate(x, rotation)
    return (None if a is None else a[:, 0].copy()), codes16(po, codebooks, x, sum_mode)
