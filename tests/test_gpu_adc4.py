"""The float-ADC view of a 4-bit index (pyqadc.AdcIndex.view_of, qadc_adc_index_create_view in include/qadc.h): db_query's
scanner_simple over scan_4<M> on the partitions the 4-bit engine has resident.  Compared are the heap ARRAYS (keys, values
bit for bit, sizes) of kv_binheap<unsigned,float>(R) after each query; the expected arrays are composed in
tests/adc4_compose.py (the reference's own compiled scan at R = 1 where oracle/_ref is built)."""
import zlib

import numpy as np
import pytest

import pyqadc
from adc4_compose import assert_heap, expected, ivf_db, rand_tables, replay
from helpers import path_independent

pytestmark = pytest.mark.gpu

ZERO = np.zeros((1, 1), np.int32)


def flat_source(M, codes, keep=0.01):
    src = pyqadc.Index(M)
    src.add_partitions([codes])
    src.finalize(keep)
    return src


def rand_codes(rng, n, M):
    return rng.integers(0, 256, (n, M // 2), dtype=np.uint8)


@path_independent
@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000, 100000, 2000000])
def test_flat_unlabeled_matches_scan_4(po, M, n):
    rng = np.random.default_rng(M * 1000003 + n)
    codes = rand_codes(rng, n, M)
    tables = rand_tables(rng, 1, 1, M)
    src = flat_source(M, codes)
    view = pyqadc.AdcIndex.view_of(src)
    assert view.partition_count() == 1 and view.partition_size(0) == n and view.table_dim == M * 16
    for sum_mode in (1, 0):
        for R in (1, 7, 100, 1000):                        # (R > n included)
            got = view.query_scan(ZERO, tables, R, sum_mode=sum_mode)
            assert_heap(got, expected(po, M, [codes], None, tables[0], R, sum_mode), 0, "n=%d R=%d sum_mode=%d" % (n, R, sum_mode))
    view.close()
    src.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("kind", ["ties", "negative", "constant", "nonfinite"])
@pytest.mark.parametrize("sum_mode", [1, 0])
def test_special_tables(po, M, kind, sum_mode):
    rng = np.random.default_rng(zlib.crc32(("%d %s %d" % (M, kind, sum_mode)).encode()))
    n = 50000
    codes = rand_codes(rng, n, M)
    tables = rand_tables(rng, 1, 1, M, kind)
    src = flat_source(M, codes)
    view = pyqadc.AdcIndex.view_of(src)
    for R in (1, 7, 100, 1000):
        got = view.query_scan(ZERO, tables, R, sum_mode=sum_mode)
        assert_heap(got, expected(po, M, [codes], None, tables[0], R, sum_mode), 0, "%s R=%d" % (kind, R))
    view.close()
    src.close()


def ivf_source(M, parts, labels, keep=0.01):
    src = pyqadc.Index(M)
    src.add_partitions(parts, labels)
    src.finalize(keep)
    return src


@path_independent
@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("ma", [1, 8, 24])
def test_ivf_with_labels_empty_partitions_and_duplicate_probes(po, M, ma):
    rng = np.random.default_rng(100 * M + ma)
    parts, labels = ivf_db(rng, M)
    src = ivf_source(M, parts, labels)
    view = pyqadc.AdcIndex.view_of(src)
    assert view.partition_count() == 64 and view.partition_size(3) == len(parts[3])
    nq = 6
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    if ma > 1:
        assign[0, 1] = assign[0, 0]                        # a duplicate probe
        assign[1, :] = assign[1, 0]                        # every probe the same partition
    empty = [k for k in range(64) if len(parts[k]) == 0]
    assign[2, 0] = empty[0]                                # an empty partition first
    tables = rand_tables(rng, nq, ma, M)
    for sum_mode, Rs in ((1, (1, 100, 1000)), (0, (100,))):
        for R in Rs:
            got = view.query_scan(assign, tables, R, sum_mode=sum_mode)
            for q in range(nq):
                want = expected(po, M, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R, sum_mode)
                assert_heap(got, want, q, "ma=%d R=%d sum_mode=%d" % (ma, R, sum_mode))
    view.close()
    src.close()


@path_independent
@pytest.mark.parametrize("M,nq", [(16, 1), (32, 2), (16, 64), (32, 64)])
def test_batches_equal_their_per_query_results(po, M, nq):
    rng = np.random.default_rng(nq + M)
    ma, R = 4, 50
    parts, labels = ivf_db(rng, M, n=20000)
    src = ivf_source(M, parts, labels)
    view = pyqadc.AdcIndex.view_of(src)
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    tables = rand_tables(rng, nq, ma, M, "ties" if nq == 64 else "dist")
    got = view.query_scan(assign, tables, R)
    for q in range(nq):
        want = expected(po, M, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
        assert_heap(got, want, q, "batch of %d" % nq)
    view.close()
    src.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
def test_candidate_stream_replays_to_the_direct_arrays(po, M):
    rng = np.random.default_rng(33 + M)
    parts, labels = ivf_db(rng, M)
    src = ivf_source(M, parts, labels)
    view = pyqadc.AdcIndex.view_of(src)
    nq, ma, R = 5, 8, 64
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    tables = rand_tables(rng, nq, ma, M, "nonfinite")
    direct = view.query_scan(assign, tables, R)
    keys, vals, offsets = view.query_scan_candidates(assign, tables, R)
    assert offsets[0] == 0 and offsets[-1] == len(keys)
    for q in range(nq):
        a, b = int(offsets[q]), int(offsets[q + 1])
        assert not np.isnan(vals[a:b]).any()
        assert_heap(direct, replay(po, keys[a:b], vals[a:b], R), q, "stream replay")
        want = expected(po, M, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R)
        assert_heap(direct, want, q, "direct")
    need = int(offsets[-1])
    assert need > 0
    rc, _, _, off2 = view.query_scan_candidates_raw(assign, tables, R, 1, need - 1)
    assert rc == pyqadc.QADC_E_CAPACITY and int(off2[-1]) == need
    rc, k2, v2, off3 = view.query_scan_candidates_raw(assign, tables, R, 1, need)          # the retry with what was asked for
    assert rc == 0 and np.array_equal(off3, offsets) and np.array_equal(k2[:need], keys)
    assert np.array_equal(v2[:need].view(np.uint32), vals.view(np.uint32))
    with pytest.raises(pyqadc.QadcError):
        view.query_scan_candidates(assign, tables, R, capacity=need - 1)
    view.close()
    src.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
def test_both_finish_modes_give_the_same_arrays(po, M):
    """the device finish (order + replay on the GPU) over a grid of shapes: identical arrays, host_finishes() stays 0;
    R = 5000 exceeds the device replay's heap and is finished on the host, and counted"""
    rng = np.random.default_rng(M + 5)
    parts, labels = ivf_db(rng, M)
    src = ivf_source(M, parts, labels)
    host = pyqadc.AdcIndex.view_of(src)
    dev = pyqadc.AdcIndex.view_of(src)                     # two views of one index
    dev.set_finish(1)
    for nq, ma, R, kind in ((1, 1, 1, "dist"), (3, 8, 100, "ties"), (64, 24, 1000, "dist"), (5, 4, 4096, "nonfinite")):
        assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
        tables = rand_tables(rng, nq, ma, M, kind)
        for sum_mode in (1, 0):
            a = host.query_scan(assign, tables, R, sum_mode=sum_mode)
            b = dev.query_scan(assign, tables, R, sum_mode=sum_mode)
            assert np.array_equal(a[2], b[2])
            for q in range(nq):
                assert_heap(b, (a[0][q, :a[2][q]], a[1][q, :a[2][q]]), q, "device finish nq=%d R=%d" % (nq, R))
            q = nq - 1
            want = expected(po, M, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], R, sum_mode)
            assert_heap(b, want, q, "device finish against the composition")
    assert dev.host_finishes() == 0 and host.host_finishes() == 0
    assign = rng.integers(0, 64, (2, 8)).astype(np.int32)
    tables = rand_tables(rng, 2, 8, M)
    a = host.query_scan(assign, tables, 5000)
    b = dev.query_scan(assign, tables, 5000)
    for q in range(2):
        assert_heap(b, (a[0][q, :a[2][q]], a[1][q, :a[2][q]]), q, "R=5000")
        want = expected(po, M, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tables[q], 5000)
        assert_heap(b, want, q, "R=5000 against the composition")
    assert dev.host_finishes() == 2
    host.close()
    dev.close()
    src.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
@pytest.mark.parametrize("finish", [0, 1])
def test_forced_overflow_reruns_and_stays_exact(po, M, finish):
    """n = 65536 codes ascending in sub-quantizers 0-3 read as base-16 digits, entries -(d * 16^k), every other table zero:
    each sum is an exact integer whatever the grouping, candidates strictly decrease, so every code is a push and the
    candidate regions overflow"""
    n = 65536
    v = np.arange(n, dtype=np.uint32)
    codes = np.zeros((n, M // 2), np.uint8)
    codes[:, 0] = (v & 0xff).astype(np.uint8)              # sub-quantizers 0 (low nibble) and 1
    codes[:, 1] = ((v >> 8) & 0xff).astype(np.uint8)       # sub-quantizers 2 and 3
    tables = np.zeros((1, 1, M, 16), np.float32)
    for k in range(4):
        tables[0, 0, k, :] = -(np.arange(16, dtype=np.float32) * np.float32(16 ** k))
    tables = tables.reshape(1, 1, M * 16)
    src = flat_source(M, codes)
    view = pyqadc.AdcIndex.view_of(src)
    view.set_finish(finish)
    for sum_mode in (1, 0):
        cand = po.candidates_f32(M, codes, tables[0, 0], sum_mode)
        assert np.array_equal(cand, -v.astype(np.float32))
        before = view.reruns()
        got = view.query_scan(ZERO, tables, 10, sum_mode=sum_mode)
        assert view.reruns() > before
        assert_heap(got, expected(po, M, [codes], None, tables[0], 10, sum_mode), 0, "overflow sum_mode=%d" % sum_mode)
    keys, vals, offsets = view.query_scan_candidates(ZERO, tables, 10)
    assert int(offsets[-1]) == n and np.array_equal(keys, v)
    view.close()
    src.close()


@path_independent
@pytest.mark.parametrize("M", [16, 32])
def test_source_variants(po, M):
    """an interleaved import, a borrowed device partition, a key base, two keep values: the view reads what the index holds"""
    import torch
    rng = np.random.default_rng(77 + M)
    n, R = 30000, 100
    codes = rand_codes(rng, n, M)
    tables = rand_tables(rng, 1, 1, M)
    want = expected(po, M, [codes], None, tables[0], R)

    src = pyqadc.Index(M)                                  # the reference's block layout, de-interleaved on import
    src.add_partition_interleaved(po.interleave(codes), n)
    src.finalize(0.01)
    view = pyqadc.AdcIndex.view_of(src)
    assert_heap(view.query_scan(ZERO, tables, R), want, 0, "interleaved import")
    view.close()
    src.close()

    labels = rng.permutation(n).astype(np.uint32)          # borrowed: a torch tensor's memory, read where it lies
    dc = torch.zeros(codes.size + 64, dtype=torch.uint8, device="cuda")
    dc[:codes.size] = torch.from_numpy(codes.reshape(-1)).cuda()
    dl = torch.from_numpy(labels.astype(np.int64)).cuda().to(torch.int32)
    torch.cuda.synchronize()
    src = pyqadc.Index(M)
    src.add_partition_device(dc.data_ptr(), n, dl.data_ptr(), keepalive=(dc, dl))
    src.finalize(0.01)
    view = pyqadc.AdcIndex.view_of(src)
    for R2 in (1, R):
        assert_heap(view.query_scan(ZERO, tables, R2), expected(po, M, [codes], [labels], tables[0], R2), 0, "borrowed partition")
    view.close()
    src.close()

    src = pyqadc.Index(M)                                  # keys offset by the partition's key base
    src.add_partitions([codes])
    src.set_key_base(0, 123456)
    src.finalize(0.01)
    view = pyqadc.AdcIndex.view_of(src)
    for R2 in (1, R):
        got = view.query_scan(ZERO, tables, R2)
        assert_heap(got, expected(po, M, [codes], None, tables[0], R2, key_bases=[123456]), 0, "key base")
    wk, wv = want
    got = view.query_scan(ZERO, tables, R)
    assert np.array_equal(got[1][0].view(np.uint32), wv.view(np.uint32))
    view.close()
    src.close()

    for keep in (0.001, 0.5):                              # the pre-scan share is the 4-bit engine's business only
        src = flat_source(M, codes, keep)
        view = pyqadc.AdcIndex.view_of(src)
        assert_heap(view.query_scan(ZERO, tables, R), want, 0, "keep %g" % keep)
        view.close()
        src.close()


def _same_result(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("keys", "values", "sizes", "status"))


@path_independent
@pytest.mark.parametrize("M", [16, 32])
def test_the_source_index_is_undisturbed(po, M):
    rng = np.random.default_rng(9 + M)
    parts, labels = ivf_db(rng, M)
    src = ivf_source(M, parts, labels)
    nq, ma, R = 8, 6, 50
    assign = rng.integers(0, 64, (nq, ma)).astype(np.int32)
    t4 = rand_tables(rng, nq, ma, M)
    tv = rand_tables(rng, nq, ma, M)
    before = src.query_scan(assign, t4.copy(), R)
    view = pyqadc.AdcIndex.view_of(src)
    got = view.query_scan(assign, tv, R)
    during = src.query_scan(assign, t4.copy(), R)
    assert _same_result(before, during)
    # a view call between submit and collect of a 4-bit batch
    tables_in_flight = t4.copy()
    src.submit(0, assign, tables_in_flight, R)
    again = view.query_scan(assign, tv, R)
    batch = src.collect(0)
    assert _same_result(before, batch)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    q = 3
    assert_heap(got, expected(po, M, [parts[k] for k in assign[q]], [labels[k] for k in assign[q]], tv[q], R), q, "view")
    view.close()
    after = src.query_scan(assign, t4.copy(), R)
    assert _same_result(before, after)
    src.close()


@path_independent
def test_refusals():
    rng = np.random.default_rng(0)
    M = 16
    codes = rand_codes(rng, 1000, M)
    src = pyqadc.Index(M)
    src.add_partitions([codes])
    with pytest.raises(pyqadc.QadcError, match="not finalized"):
        pyqadc.AdcIndex.view_of(src)
    src.finalize(0.01)
    src.add_partitions([codes])                            # (adding un-finalizes)
    with pytest.raises(pyqadc.QadcError, match="not finalized"):
        pyqadc.AdcIndex.view_of(src)
    src.close()

    shard = pyqadc.Index(M)                                # the second half of a partition, with a starts replica
    shard.add_partition_shard(codes[512:], 512, 1000, starts=codes[:16])
    shard.finalize(0.01)
    with pytest.raises(pyqadc.QadcError, match="sharded"):
        pyqadc.AdcIndex.view_of(shard)
    shard.close()

    src = flat_source(M, codes)
    view = pyqadc.AdcIndex.view_of(src)
    with pytest.raises(pyqadc.QadcError, match="view"):
        view.add_partitions([rng.integers(0, 256, (10, M), dtype=np.uint8)])
    with pytest.raises(pyqadc.QadcError, match="view"):
        view.set_pq_raw(32, np.zeros((M, 256, 2), np.float32))
    with pytest.raises(pyqadc.QadcError, match="view"):
        view.set_rotation(np.eye(32, dtype=np.float32))
    with pytest.raises(pyqadc.QadcError, match="view"):
        view.set_coarse(np.zeros((4, 32), np.float32))
    with pytest.raises(ValueError):                        # tables [M][256]: the whole-byte engine's size
        view.query_scan(ZERO, np.zeros((1, 1, M * 256), np.float32), 10)
    tables = rand_tables(rng, 1, 1, M)
    for a in (1, -1):
        with pytest.raises(pyqadc.QadcError, match="partition"):
            view.query_scan(np.array([[a]], np.int32), tables, 10)
    with pytest.raises(pyqadc.QadcError, match="set_pq"):  # no quantizer on the source
        view.search(np.zeros((1, 32), np.float32), 1, 10)
    with pytest.raises(pyqadc.QadcError, match="1 live float-ADC view"):
        src.close()
    got = view.query_scan(ZERO, tables, 10)                # the refused close left everything in place
    assert got[2][0] == 10
    view.close()
    src.close()
    with pytest.raises(pyqadc.QadcError, match="Supported configurations are"):
        pyqadc.AdcIndex(16, 4)
