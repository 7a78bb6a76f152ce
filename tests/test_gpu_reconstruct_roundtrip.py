"""GPU: the decoder against the encoders, through the engine and with no twin involved.  On the exactness
fixtures (tests/pq_decode_compose.py exact_fixture: small integers, every product and sum exact; tests/test_pq_decode_host.py holds
the encoders' CPU statements to it) index A is built from vectors made of centroid rows, every key is reconstructed in device memory,
the result is appended to an empty index B with the same quantizers, and every partition of B, read back, equals A's — IVF and flat at
4, 8 and 16 bits, with and without a rotation."""
import numpy as np
import pytest

import pq_decode_compose as pdc
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(16, 4, 32), (8, 8, 16), (2, 16, 8)]


def make(pyqadc, fx, bits, nsq):
    idx = pyqadc.Index(nsq) if bits == 4 else pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)
    idx.set_pq(fx["cb"])
    if fx["rotation"] is not None:
        idx.set_rotation(fx["rotation"])
    if fx["coarse"] is not None:
        idx.set_coarse(fx["coarse"])
    return idx


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("K", [0, 6], ids=["flat", "ivf"])
@pytest.mark.parametrize("nsq,bits,dim", SHAPES, ids=["%dx%d-dim%d" % s for s in SHAPES])
def test_reconstruct_then_add_gives_the_same_index(nsq, bits, dim, K, rotated):
    import pyqadc
    fx = pdc.exact_fixture(nsq, bits, dim, K, rotated)
    n = 500
    codes, assign = pdc.exact_rows(fx, n)
    x = pdc.restate(fx["cb"], codes, assign, fx["coarse"], fx["rotation"])  # vectors made of centroid rows: exact integers
    labels = np.random.default_rng(bits).permutation(100000)[:n].astype(np.uint32) if K else np.arange(n, dtype=np.uint32)
    a = make(pyqadc, fx, bits, nsq)
    a.add_vectors(x, labels=labels if K else None)
    if bits == 4:
        a.finalize(0.01)
    view = pyqadc.AdcIndex.view_of(a) if bits == 4 else a
    keys = torch.from_numpy(labels.view(np.int32)).cuda()
    rec, where = view.reconstruct_device(keys)
    assert (where.cpu().numpy() != -1).all()
    assert np.array_equal(rec.cpu().numpy().view(np.uint32), x.view(np.uint32))          # decode(encode(x)) == x
    b = make(pyqadc, fx, bits, nsq)
    b.add_vectors_device(rec, labels=keys if K else None)
    assert b.partition_count() == a.partition_count() == max(K, 1)
    for p in range(a.partition_count()):
        ca, la = a.read_partition(p)
        cb, lb = b.read_partition(p)
        assert np.array_equal(ca, cb), "partition %d: codes differ" % p
        assert (la is None and lb is None) or np.array_equal(la, lb), "partition %d: labels differ" % p
        want = pdc.unpack(codes, bits)[assign == p] if K else pdc.unpack(codes, bits)
        assert np.array_equal(pdc.unpack(ca, bits), want), "partition %d: not the codes the vectors were made from" % p
    if bits == 4:
        view.close()
    a.close()
    b.close()
