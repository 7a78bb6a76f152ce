"""GPU: the bucket copy (DESIGN.md sections 2 and 3.1) across lives of the 4-bit index, next to
tests/test_gpu_index_lifecycle.py::test_byte_plane_copy_after_remove_and_add, whose walk this follows: finalize builds the copy
from the codes as they are then, so after remove_labels and add_vectors it is rebuilt, and what the bucket form scans must be the
rows the model holds.  The bucket form is forced at lists of a few tiles (tests/test_gpu_bkt_scan.py: TINY, bkt_block = one
tile, bkt_max_pad lifted).  Every comparison is for equality: read_partition against the numpy model, the copy read back against
tests/bkt_model.py, query_scan's heaps and status against the CPU oracle (po.query_scan) on the model's rows."""
import numpy as np
import pytest

import bkt_model
import pyqadc
from helpers import float_tables, heaps_equal, rand_codes
from test_gpu_adc_remove import model_remove
from test_gpu_bkt_scan import ONE_QUERY_PER_PASS, TILE, TINY, best_code, check_profile, make_index
from test_gpu_index_add import Quantizers4

pytestmark = pytest.mark.gpu
M = 16
R = 100


def force_bkt(idx, block=TILE, nsp=5):
    """make_index's settings on an index that came from Quantizers4.index()."""
    for k, v in dict(ONE_QUERY_PER_PASS, **TINY).items():
        idx.set_option(k, v)
    idx.set_split(1, 1)
    idx.set_split6(1)
    idx.set_split5(1)
    idx.set_split_nib(1, 0, 9)
    idx.set_split_bkt(1, block, int(nsp == 6), int(nsp == 5), int(nsp == 4), 1e6)
    idx.set_option("profile", 1)


def keep_for(rows):
    """0.01 where that leaves R starts, else 0.5 (tests/index_model.py: index4_keep)"""
    return 0.01 if int(rows * 0.01) >= R else 0.5


def check_copies(idx, model, block=TILE):
    """every partition's copy against the model's codes; -> the slots of all of them"""
    slots = 0
    for p, (codes, _) in enumerate(model):
        copy = idx.bkt_copy(p)
        if len(codes) == 0:
            assert copy is None, p
            continue
        assert copy is not None, p
        bkt_model.check_copy(copy, codes, block)
        slots += sum(l[2] for l in bkt_model.block_layout(codes, block))
    return slots


def check_queries(po, idx, model, assign, tables, keep, what):
    """query_scan against po.query_scan on the model, status and heaps; -> (result, profile of the batch)"""
    idx.profile_reset()
    res = idx.query_scan(assign, tables.copy(), R)
    for i in range(len(assign)):
        want = po.query_scan(M, [c for c, _ in model], [l for _, l in model], keep, assign[i], tables[i].copy(), R)
        assert want["rc"] == res["status"][i], "%s: status of query %d" % (what, i)
        if want["rc"] == 0:
            assert heaps_equal(res["heaps"][i], (want["keys"], want["values"])), "%s: query %d" % (what, i)
    return res, idx.profile()


def test_bucket_copy_after_remove_and_add(po):
    q = Quantizers4(16, 16, K=1, n=50, seed=9)                                   # one coarse centroid: add_vectors on a labelled partition
    a, new_codes = q.encoded()
    assert not a.any()
    n = 3 * TILE + 101
    rng = np.random.default_rng(18)
    codes = rand_codes(rng, n, M)
    codes[:, 1] &= 3                                                             # 1024 keys: buckets of some 16 codes
    labels = rng.permutation(3 * n)[:n].astype(np.uint32)
    tables = float_tables(np.random.default_rng(5), 3, 1, M)
    assign = np.zeros((3, 1), np.int32)
    idx = q.index()
    try:
        force_bkt(idx)
        model = [(codes, labels)]

        def finalized(rows, what, keep=None):
            keep = keep_for(rows) if keep is None else keep
            idx.finalize(keep)
            assert len(model[0][0]) == rows and idx.partition_size(0) == rows, what
            got_codes, got_labels = idx.read_partition(0)
            assert np.array_equal(got_codes, model[0][0]), what
            assert rows == 0 or np.array_equal(got_labels, model[0][1]), what
            slots = check_copies(idx, model)
            res, pr = check_queries(po, idx, model, assign, tables, keep, what)
            assert pr["bkt_copy_slots"] == slots and pr["bkt_copy_failed"] == pr["bkt_copy_padded_out"] == 0, (what, pr)
            assert pr["bkt_copy_bytes"] == slots // TILE * (100352 + 196608), (what, pr)
            if rows:
                assert np.all(res["status"] == 0), what
                check_profile(pr, 5)                                             # every launch a bucket launch, no nibble-plane copy
                assert pr["bkt_codes"] == 3 * rows, (what, pr)
            else:
                assert idx.bkt_copy(0) is None and pr["bkt_copy_bytes"] == 0 and pr["bkt_launches"] == 0, (what, pr)
            return res, pr

        idx.add_partitions([codes], [labels])
        finalized(3 * TILE + 101, "add_partitions")
        removed = model[0][1][rng.permutation(n)[:100]]
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == 100
        finalized(3 * TILE + 1, "100 rows removed")
        idx.add_vectors(q.vectors, labels_offset=3 * n + 7)
        model = [(np.concatenate([model[0][0], new_codes]), np.concatenate([model[0][1], (np.arange(50) + 3 * n + 7).astype(np.uint32)]))]
        finalized(3 * TILE + 51, "50 rows appended")
        removed = np.concatenate([model[0][1][-30:], model[0][1][rng.permutation(3 * TILE)[:21]]])
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == 51
        first, pr1 = finalized(3 * TILE, "51 rows removed: three whole blocks")
        # a second finalize with another keep and no mutation in between: the copy is rebuilt, the same size
        again, pr2 = finalized(3 * TILE, "finalized again", keep=0.05)
        assert pr2["bkt_copy_bytes"] == pr1["bkt_copy_bytes"] and pr2["bkt_copy_slots"] == pr1["bkt_copy_slots"]
        removed = model[0][1][rng.permutation(3 * TILE)[:2 * TILE + 5000]]
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == 2 * TILE + 5000
        finalized(TILE - 5000, "one partial block")
        removed = model[0][1].copy()
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == TILE - 5000
        finalized(0, "no row left")
    finally:
        idx.close()


def refused_state(f, *args):
    with pytest.raises(pyqadc.QadcError, match="finalize") as e:
        f(*args)
    assert "qadc error %d:" % pyqadc.QADC_E_STATE in str(e.value)


@pytest.mark.parametrize("nib_copy", [False, True], ids=["no-nibble-copy", "nibble-copy"])
def test_bkt_state_rules_on_a_finalized_index(po, nib_copy):
    """Turning the form off or changing bkt_block on a finalized index is refused (the copy is finalize's).  The thresholds may
    change: with bkt_min_run above every run no launch reads the bucket copy, and none reads a copy that was never built: the
    launches take the nibble form where finalize built that copy (blocks of two tiles, the first two cuts miss them), the
    5-plane form where it did not (one partition, every long run on blocks)."""
    rng = np.random.default_rng(29)
    block = 2 * TILE if nib_copy else TILE
    n = 65536 + 3 * 2 * TILE + 37
    codes = rand_codes(rng, n, M)
    codes[:, 1] &= 1
    tables = float_tables(rng, 2, 1, M)
    codes[-1] = best_code(tables[0, 0])
    assign = np.zeros((2, 1), np.int32)
    model = [(codes, None)]
    want = [po.query_scan(M, [codes], None, 0.01, [0], tables[i].copy(), R) for i in range(2)]
    idx = make_index(pyqadc, [codes], 6, block=block)
    try:
        before = idx.query_scan(assign, tables.copy(), R)
        pr = idx.profile()
        check_profile(pr, 6, all_bkt=not nib_copy, nib_copy=nib_copy)
        assert (pr["nib_launches"] > 0) == nib_copy, pr
        refused_state(idx.set_split_bkt, 1, 2 * block, 1, 0, 0, 1e6)
        refused_state(idx.set_split_bkt, 0)
        refused_state(idx.set_split_bkt, 0, block, 1, 0, 0, 1e6)
        idx.set_split_bkt(1 << 40, 0, 1, 0, 0, 0.0)                              # accepted: a threshold
        idx.profile_reset()
        after = idx.query_scan(assign, tables.copy(), R)
        pa = idx.profile()
        assert pa["bkt_launches"] == pa["bkt_codes"] == pa["bkt_slots"] == pa["bkt_survivors"] == 0, pa
        assert pa["bkt_copy_bytes"] == pr["bkt_copy_bytes"] > 0 and (pa["nib_copy_bytes"] > 0) == nib_copy, pa
        assert pa["split_launches"] == pr["split_launches"] > 0 and pa["split_codes"] == pr["split_codes"], (pa, pr)
        other = "nib_launches" if nib_copy else "split5_launches"
        assert pa[other] == pa["split_launches"], pa
        idx.set_split_bkt(1, 0, 0, 1, 0, 0.0)                                    # and back, with 5 paid planes
        idx.profile_reset()
        back = idx.query_scan(assign, tables.copy(), R)
        pb = idx.profile()
        check_profile(pb, 5, all_bkt=not nib_copy, nib_copy=nib_copy)
        assert pb["bkt_launches"] == pr["bkt_launches"] == pb["bkt5_launches"] and pb["bkt_codes"] == pr["bkt_codes"], (pb, pr)
        for res in (before, after, back):
            assert np.all(res["status"] == 0)
            for i in range(2):
                assert heaps_equal(res["heaps"][i], (want[i]["keys"], want[i]["values"])), i
        assert np.count_nonzero(after["heaps"][0][0] == n - 1) == 1 + (16 - n % 16) % 16
        check_copies(idx, model, block)
    finally:
        idx.close()


def test_bucket_copies_of_two_partitions_through_a_life(po):
    """Two labelled partitions, probed in both orders: rows are appended to both, partition 0 is cut back to two whole blocks;
    finalize rebuilds both copies.  Order [0, 1] puts every cut on a block; in order [1, 0] partition 1's odd size moves
    partition 0's cuts off its blocks, and those runs take the nibble form (two partitions: finalize keeps that copy)."""
    q = Quantizers4(16, 16, K=2, n=60, seed=4)
    a, new_codes = q.encoded()
    added = [int((a == p).sum()) for p in range(2)]
    assert min(added) >= 5
    rng = np.random.default_rng(21)
    sizes = [2 * TILE + 60, 2 * TILE + 37]
    model = []
    for p, s in enumerate(sizes):
        c = rand_codes(rng, s, M)
        c[:, 1] &= 3
        model.append((c, (np.arange(s) * 2 + p).astype(np.uint32)))              # even labels in partition 0, odd ones in 1
    tables = float_tables(rng, 2, 2, M)
    assign = np.array([[0, 1], [1, 0]], np.int32)
    idx = q.index()
    try:
        force_bkt(idx, nsp=6)
        idx.add_partitions([c for c, _ in model], [l for _, l in model])
        idx.finalize(0.01)
        check_copies(idx, model)
        base = 1 << 20
        idx.add_vectors(q.vectors, labels_offset=base)
        new_labels = (np.arange(60) + base).astype(np.uint32)
        model = [(np.concatenate([c, new_codes[a == p]]), np.concatenate([l, new_labels[a == p]])) for p, (c, l) in enumerate(model)]
        removed = np.concatenate([new_labels[a == 0], model[0][1][rng.permutation(sizes[0])[:60]]])
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == added[0] + 60
        assert [len(c) for c, _ in model] == [2 * TILE, sizes[1] + added[1]]
        with pytest.raises(pyqadc.QadcError, match="finalize"):
            idx.query_scan(assign, tables.copy(), R)
        idx.finalize(0.01)
        for p in range(2):
            got_codes, got_labels = idx.read_partition(p)
            assert np.array_equal(got_codes, model[p][0]) and np.array_equal(got_labels, model[p][1]), p
        slots = check_copies(idx, model)
        res, pr = check_queries(po, idx, model, assign, tables, 0.01, "after the removal")
        assert np.all(res["status"] == 0)
        check_profile(pr, 6, all_bkt=False, nib_copy=True)
        assert pr["bkt_copy_slots"] == slots and pr["bkt6_launches"] == pr["bkt_launches"] and pr["nib_launches"] > 0, pr
    finally:
        idx.close()
