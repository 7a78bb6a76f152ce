"""GPU: reconstruction on an index — qadc_adc_index_reconstruct(_device) and _reconstruct_rows(_device) (include/qadc.h
"Reconstruction") — bit for bit against the CPU twin: the lookup's definition (the smallest (partition, row)
that holds a key) on the index read back, then host/pq_decode.hpp on the rows found.  Labelled IVF, flat, unlabelled multi-partition
and 16-bit indexes, views of 16 x 4 and 32 x 4 indexes with a key_base; repeats, labels held twice, missing keys, the full key span,
count 0, empty partitions, after a removal and a relocation, under a filter, by position, and behind a search."""
import ctypes as C

import numpy as np
import pytest

import pq_decode_compose as pdc
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def driver():
    return pdc.build_driver()


def expected(driver, tmp_path, parts, labels, key_base, keys, cb, coarse, rotation):
    """parts: the code rows of every partition -> (vectors, where) by the twin"""
    sizes = [len(p) for p in parts]
    where = pdc.where_numpy(sizes, labels, key_base, keys)
    assert np.array_equal(pdc.twin_where(driver, tmp_path, sizes, labels, key_base, keys), where)
    found = where != pdc.MISSING
    assign = np.where(found, (where >> np.uint64(32)).astype(np.int64), -1).astype(np.int32)
    rows = np.zeros((len(where),) + parts[0].shape[1:], parts[0].dtype)
    for i in np.flatnonzero(found):
        rows[i] = parts[assign[i]][int(where[i] & np.uint64(0xFFFFFFFF))]
    return pdc.twin(driver, tmp_path, cb, rows, assign, coarse, rotation), where


def read_back(idx):
    got = [idx.read_partition(p) for p in range(idx.partition_count())]
    return [g[0] for g in got], (None if got[0][1] is None else [g[1] for g in got])


def check_index(pyqadc, driver, tmp_path, idx, keys, cb, coarse, rotation, parts=None, labels=None, key_base=None, what=""):
    if parts is None:
        parts, labels = read_back(idx)
    keys = np.ascontiguousarray(keys, np.uint32)
    want, want_where = expected(driver, tmp_path, parts, labels, key_base if labels is None else None, keys, cb, coarse, rotation)
    got, where = idx.reconstruct(keys)
    assert np.array_equal(where, want_where), what
    pdc.same_floats(got, want, what + ": host form")
    t = torch.from_numpy(keys.view(np.int32)).cuda()
    dgot, dwhere = idx.reconstruct_device(t)
    assert np.array_equal(dwhere.cpu().numpy().view(np.uint64), want_where), what
    pdc.same_floats(dgot.cpu().numpy(), want, what + ": device form")
    return want, want_where


def quantizers(rng, nsq, bits, dim, K, rotated):
    c = pdc.random_case(rng, nsq, bits, dim, 1, K, rotated)
    return c["cb"], (c["coarse"] * 4 if K else None), c["rotation"]


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("nsq,bits,dim", [(8, 8, 24), (4, 16, 12)], ids=["8x8", "4x16"])
def test_labelled_ivf(pyqadc, driver, tmp_path, nsq, bits, dim, rotated):
    rng = np.random.default_rng(bits + rotated)
    K, n = 6, 2000
    cb, coarse, rot = quantizers(rng, nsq, bits, dim, K, rotated)
    coarse[4] = 1e6                                                         # partition 4 stays empty
    idx = pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)
    idx.set_pq(cb)
    idx.set_rotation(rot)
    idx.set_coarse(coarse)
    vec = (coarse[rng.integers(0, 4, n)] + rng.normal(size=(n, dim))).astype(np.float32)
    labels = rng.integers(100, 1500, n).astype(np.uint32)                   # held twice, inside a partition and across partitions
    labels[:4] = (0, 0xFFFFFFFF, 0xFFFFFFFE, 7)
    idx.add_vectors(vec, labels=labels)
    assert idx.partition_size(4) == 0
    keys = np.concatenate([labels[:300], labels[:300][::-1], [1, 2, 3, 99, 1500, 1501], labels[5:9]]).astype(np.uint32)   # repeats, missing
    want, where = check_index(pyqadc, driver, tmp_path, idx, keys, cb, coarse, rot, what="ivf")
    assert (where[600:606] == pdc.MISSING).all() and (want[600:606].view(np.uint32) == pdc.NAN_BITS).all()
    parts, labs = read_back(idx)
    twice = [k for k in np.unique(labels) if sum(int((l == k).sum()) for l in labs) > 1][:50]
    assert len(twice) > 10
    check_index(pyqadc, driver, tmp_path, idx, twice, cb, coarse, rot, what="held twice")
    # keys 0 and 0xFFFFFFFF together: the full span, a 512 MiB bitmap
    check_index(pyqadc, driver, tmp_path, idx, [0xFFFFFFFF, 0, 5, 0xFFFFFFFE], cb, coarse, rot, what="full span")
    # count = 0
    got, where = idx.reconstruct(np.zeros(0, np.uint32))
    assert got.shape == (0, dim) and where.shape == (0,)
    # a filter set on the index is ignored: a lookup, not a search
    f = pyqadc.AdcFilter(labels[:200], "exclude")
    idx.set_filter(f)
    check_index(pyqadc, driver, tmp_path, idx, keys, cb, coarse, rot, what="under a filter")
    idx.set_filter(None)
    f.close()
    # after remove_labels moved rows
    before = [idx.partition_size(p) for p in range(K)]
    assert idx.remove_labels(labels[10:400]) > 0
    want2, where2 = check_index(pyqadc, driver, tmp_path, idx, keys, cb, coarse, rot, what="after a removal")
    assert (where2[10:300] == pdc.MISSING).all() and [idx.partition_size(p) for p in range(K)] != before
    # after an add_vectors that relocated
    reloc = idx.relocations()
    more = (coarse[rng.integers(0, 4, 5000)] + rng.normal(size=(5000, dim))).astype(np.float32)
    idx.add_vectors(more, labels=np.arange(5000, 10000, dtype=np.uint32))
    assert idx.relocations() > reloc
    check_index(pyqadc, driver, tmp_path, idx, np.concatenate([keys, np.arange(5000, 5300, dtype=np.uint32)]), cb, coarse, rot,
                what="after a relocation")
    # by position: reconstruct_rows equals read_partition plus the stateless decode
    assert idx.reconstruct_rows(4).shape == (0, dim) and idx.reconstruct_rows(0, idx.partition_size(0), 0).shape == (0, dim)
    for p in (0, 3):
        size = idx.partition_size(p)
        for first, count in ((0, size), (size // 3, size - size // 3)):
            codes = idx.read_partition(p, first, count)[0]
            want_rows = pdc.twin(driver, tmp_path, cb, codes, np.full(count, p, np.int32), coarse, rot)
            pdc.same_floats(idx.reconstruct_rows(p, first, count), want_rows, "rows")
            pdc.same_floats(idx.reconstruct_rows_device(p, first, count).cpu().numpy(), want_rows, "rows, device")
    with pytest.raises(pyqadc.QadcError, match="outside partition"):
        idx.reconstruct_rows(0, 1, idx.partition_size(0))
    with pytest.raises(pyqadc.QadcError, match="does not exist"):
        idx.reconstruct_rows(K, 0, 0)
    # a coarse K that is not the partition count
    idx.set_coarse(coarse[:3])
    with pytest.raises(pyqadc.QadcError, match="partitions"):
        idx.reconstruct(keys)
    idx.close()


@path_independent
def test_refused_without_codebooks(pyqadc):
    idx = pyqadc.AdcIndex(8, 8)
    idx.add_partitions([np.zeros((10, 8), np.uint8)])
    out = np.zeros((1, 8), np.float32)
    key = np.zeros(1, np.uint32)
    assert pyqadc.lib().qadc_adc_index_reconstruct(idx._h, key.ctypes.data_as(C.POINTER(C.c_uint32)), 1, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                   None) == pyqadc.QADC_E_ARG
    assert b"set_pq" in pyqadc.lib().qadc_last_error()
    idx.close()


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
def test_flat_and_unlabelled_partitions(pyqadc, driver, tmp_path, rotated):
    rng = np.random.default_rng(3)
    nsq, dim = 4, 12
    cb, _, rot = quantizers(rng, nsq, 8, dim, 0, rotated)
    # flat: one unlabelled partition filled by add_vectors, key = position
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.set_pq(cb)
    idx.set_rotation(rot)
    idx.add_vectors(rng.normal(size=(700, dim)).astype(np.float32))
    keys = np.concatenate([rng.integers(0, 700, 200), [699, 700, 0xFFFFFFFF, 0]]).astype(np.uint32)
    parts, _ = read_back(idx)
    _, where = check_index(pyqadc, driver, tmp_path, idx, keys, cb, None, rot, parts=parts, labels=None, key_base=[0], what="flat")
    assert where[200] == 699 and where[201] == pdc.MISSING
    idx.close()
    # unlabelled partitions share positions: the lowest partition that has the row wins
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.set_pq(cb)
    idx.set_rotation(rot)
    sizes = [30, 0, 100, 65]
    parts = [rng.integers(0, 256, (n, nsq)).astype(np.uint8) for n in sizes]
    idx.add_partitions(parts)
    keys = np.array([0, 29, 30, 64, 65, 99, 100, 5, 5], np.uint32)
    _, where = check_index(pyqadc, driver, tmp_path, idx, keys, cb, None, rot, parts=parts, labels=None, key_base=[0] * 4, what="unlabelled")
    assert where.tolist() == [0, 29, (2 << 32) | 30, (2 << 32) | 64, (2 << 32) | 65, (2 << 32) | 99, int(pdc.MISSING), 5, 5]
    idx.close()


@path_independent
@pytest.mark.parametrize("labelled", [False, True], ids=["key_base", "labels"])
@pytest.mark.parametrize("M", [16, 32])
def test_view_of_a_4bit_index(pyqadc, driver, tmp_path, M, labelled):
    rng = np.random.default_rng(M)
    dim, K = 2 * M, 3
    cb, coarse, rot = quantizers(rng, M, 4, dim, K, True)
    sizes = [500, 0, 333]
    parts = [rng.integers(0, 256, (n, M // 2)).astype(np.uint8) for n in sizes]
    labels = [rng.integers(0, 600, n).astype(np.uint32) for n in sizes] if labelled else None
    base = [1000, 0, 1400]
    index = pyqadc.Index(M)
    index.add_partitions(parts, labels)
    if not labelled:
        for p, b in enumerate(base):
            index.set_key_base(p, b)
    index.finalize(0.01)
    index.set_pq(cb)
    index.set_rotation(rot)
    index.set_coarse(coarse)
    view = pyqadc.AdcIndex.view_of(index)
    keys = (np.concatenate([labels[0][:50], labels[2][:50], [600, 601]]) if labelled
            else np.array([1000, 1499, 1500, 1400, 1732, 1733, 999, 0, 1450, 1450])).astype(np.uint32)
    want, where = check_index(pyqadc, driver, tmp_path, view, keys, cb, coarse, rot, parts=parts, labels=labels, key_base=base, what="view")
    if not labelled:
        assert where.tolist()[:7] == [0, 499, (2 << 32) | 100, 400, (2 << 32) | 332, int(pdc.MISSING), int(pdc.MISSING)]
    pdc.same_floats(view.reconstruct_rows(2, 300, 33), pdc.twin(driver, tmp_path, cb, parts[2][300:], np.full(33, 2, np.int32), coarse, rot), "rows")
    view.close()
    got, got_where = index.reconstruct(keys)                                # the convenience: a view made, asked and destroyed
    pdc.same_floats(got, want, "Index.reconstruct")
    assert np.array_equal(got_where, where)
    index.close()


@path_independent
def test_search_reconstruct_equals_search_plus_reconstruct(pyqadc):
    rng = np.random.default_rng(12)
    nsq, dim, K, n, nq, R = 8, 32, 4, 3000, 7, 40
    cb, coarse, rot = quantizers(rng, nsq, 8, dim, K, True)
    idx = pyqadc.AdcIndex(nsq, 8)
    idx.set_pq(cb)
    idx.set_rotation(rot)
    idx.set_coarse(coarse)
    vec = (coarse[rng.integers(0, K, n)] + rng.normal(size=(n, dim))).astype(np.float32)
    idx.add_vectors(vec, labels=rng.permutation(50000)[:n].astype(np.uint32))
    small = (coarse[3] + rng.normal(size=(10, dim)) * 0.01).astype(np.float32)
    q = torch.from_numpy(np.concatenate([vec[:nq - 1], small[:1]])).cuda()
    keys, vals, sizes, vectors, where = idx.search_reconstruct(q, 1, R)
    k2, v2, s2 = idx.search_device(q, 1, R)
    assert torch.equal(keys, k2) and torch.equal(sizes, s2)
    sz = sizes.cpu().numpy()
    host, host_where = idx.reconstruct(keys.cpu().numpy().view(np.uint32).reshape(-1))
    host, host_where = host.reshape(nq, R, dim), host_where.reshape(nq, R)
    got, got_where = vectors.cpu().numpy(), where.cpu().numpy().view(np.uint64)
    for qi in range(nq):
        pdc.same_floats(got[qi, :sz[qi]], host[qi, :sz[qi]], "query %d" % qi)
        assert np.array_equal(got_where[qi, :sz[qi]], host_where[qi, :sz[qi]])
        assert (got[qi, sz[qi]:].view(np.uint32) == pdc.NAN_BITS).all() and (got_where[qi, sz[qi]:] == pdc.MISSING).all()
    assert (sz > 0).all() and vectors.shape == (nq, R, dim)
    # the nearest reconstruction of a stored vector is close to it
    assert np.linalg.norm(got[0, :sz[0]] - vec[0], axis=1).min() < np.linalg.norm(vec[0])
    idx.close()
