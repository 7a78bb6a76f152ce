"""add_vectors with the caller's label of every vector (qadc_adc_index_add_vectors_labelled, qadc_index_add_vectors_labelled and
their _device forms; add_vectors(labels=...) of pyqadc.AdcIndex and pyqadc.Index; DESIGN.md sections 11.5 and 11.6).

The definition is the test: the index after the labelled call is the index after the plain call with labels_offset 0, every
stored label i replaced by labels[i].  So a twin index takes the plain call beside every labelled one, through the same
sequence of adds, reserves and removals, and the partitions read back are compared for equality, codes as they are and the
twin's labels mapped through the label array.  Relocations are compared too: the labelled call plans as the plain one does.
The labels are random over 32 bits, with repeats, 0 and 0xFFFFFFFF among them, and with a cluster in a window of 4096 values:
a remove list or a filter drawn from the cluster needs a small bitmap (one over two random labels spans gigabits).
Every shape runs in the host form (numpy arrays) and in the device form (torch tensors, the labels as int32 bits)."""
import numpy as np
import pytest

import adc_filter_compose as afc
import pyqadc
from helpers import path_independent
from test_gpu_adc_add import TILE, Quantizers, assert_partitions, read_all
from test_gpu_index_add import Quantizers4

pytestmark = pytest.mark.gpu

# (engine, Quantizers arguments, OPQ)
CASES = [("adc", (8, 8, 64), False), ("adc", (16, 8, 32), True), ("adc", (2, 16, 16), False), ("idx", (16, 32), False), ("idx", (32, 64), False)]
IDS = ["adc8x8", "adc16x8opq", "adc2x16", "idx16x4", "idx32x4"]
ENGINES = [("adc", (8, 8, 64), False), ("idx", (16, 32), False)]                 # one shape per engine, for the lives
FORMS = ["host", "device"]
CLUSTER = 0x70000000                                                             # the window [CLUSTER, CLUSTER + 4096)


def make_quantizers(case, **kw):
    engine, shape, _ = case
    return Quantizers(*shape, **kw) if engine == "adc" else Quantizers4(*shape, **kw)


_shared = {}


def shared(case):
    if case not in _shared:
        _shared[case] = make_quantizers(case)
    return _shared[case]


def make_labels(n, seed):
    """uint32 [n]: random over 32 bits; a quarter in the cluster window (with repeats there); 0xFFFFFFFF, 0 and one repeat of a
    random label placed by hand"""
    rng = np.random.default_rng(900 + seed)
    lab = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    near = rng.choice(n, n // 4, replace=False)
    lab[near] = (CLUSTER + rng.integers(0, 4096, len(near))).astype(np.uint32)
    lab[0] = 0xFFFFFFFF
    if n >= 4:
        lab[n // 2] = 0
        lab[n - 1] = lab[1]
    return lab


def add(idx, form, vectors, labels=None, labels_offset=0, sum_mode=1):
    """add_vectors in the given form: labels None = the plain call"""
    if form == "host":
        idx.add_vectors(vectors, labels_offset=labels_offset, sum_mode=sum_mode, labels=labels)
        return
    import torch
    tv = torch.from_numpy(np.ascontiguousarray(vectors, np.float32)).to("cuda:0")
    tl = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels).view(np.int32)).to("cuda:0")
    idx.add_vectors_device(tv, labels_offset=labels_offset, sum_mode=sum_mode, labels=tl)


def mapped(parts, lab):
    """the twin's partitions with every label i replaced by lab[i]"""
    return [(c, lab[l]) for c, l in parts]


def assert_twin(got, twin, lab, what=""):
    assert_partitions(read_all(got), mapped(read_all(twin), lab), what)
    assert got.relocations() == twin.relocations(), "%s: %d relocations, the plain call made %d" % (what, got.relocations(), twin.relocations())


# ---- 1. the definition, every shape and form ---------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_partitions_equal_the_plain_call_with_mapped_labels(case, form):
    q, opq = shared(case), case[2]
    for n in (1, TILE - 1, TILE + 1):
        lab = make_labels(n, n)
        got, twin = q.index(opq), q.index(opq)
        try:
            add(got, form, q.vectors[:n], lab)
            add(twin, form, q.vectors[:n])
            assert_twin(got, twin, lab, "n %d" % n)
            stored = np.concatenate([l for _, l in read_all(got)])
            assert np.array_equal(np.sort(stored), np.sort(lab)), "n %d: the stored labels are not the caller's, each once" % n
            if n > 1:
                assert (stored == 0xFFFFFFFF).sum() == 1 and (stored == 0).sum() == 1 and (stored == lab[1]).sum() >= 2
        finally:
            got.close()
            twin.close()


@path_independent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", [("adc", (8, 8, 8), False), ("idx", (16, 16), False)], ids=["adc8x8", "idx16x4"])
def test_a_call_longer_than_one_pass(case, form):
    """262144 + 5 vectors: the second pass reads labels + 262144; a repeated label stands on either side of the pass edge"""
    chunk = pyqadc.QADC_ADC_ADD_CHUNK if case[0] == "adc" else pyqadc.QADC_INDEX_ADD_CHUNK
    n = chunk + 5
    q = make_quantizers(case, n=n, seed=6)
    lab = make_labels(n, 6)
    lab[chunk] = lab[chunk - 1]
    got, twin = q.index(), q.index()
    try:
        add(got, form, q.vectors, lab)
        add(twin, form, q.vectors)
        assert_twin(got, twin, lab)
        where = [p for p, (_, l) in enumerate(read_all(twin)) if (l == chunk + 4).any()]
        assert len(where) == 1 and read_all(got)[where[0]][1][-1] == lab[chunk + 4], "the last vector's label does not stand last in its partition"
    finally:
        got.close()
        twin.close()


# ---- 2. one life: growth, reserve, room freed by remove_labels ---------------------------------------------------------------

GROWTH = [1, 2, 5, 300, 1000]


@path_independent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", ENGINES, ids=["adc8x8", "idx16x4"])
def test_growth_reserve_and_freed_room(case, form):
    total, more = sum(GROWTH), 40
    q = make_quantizers(case, n=total, seed=3)
    lab = make_labels(total + more, 3)
    got, twin, res, res_twin = q.index(), q.index(), q.index(), q.index()
    try:
        at = 0
        for n in GROWTH:                                                         # calls that relocate
            add(got, form, q.vectors[at:at + n], lab[at:at + n])
            add(twin, form, q.vectors[at:at + n], labels_offset=at)
            at += n
            assert_twin(got, twin, lab, "after %d vectors" % at)
        assert got.relocations() > 0
        sizes = [got.partition_size(p) for p in range(q.K)]

        res.reserve(sizes)                                                       # calls after a reserve: none relocates
        res_twin.reserve(sizes)
        at = 0
        for n in GROWTH:
            add(res, form, q.vectors[at:at + n], lab[at:at + n])
            add(res_twin, form, q.vectors[at:at + n], labels_offset=at)
            at += n
        assert res.relocations() == 0
        assert_twin(res, res_twin, lab, "reserved")
        assert_partitions(read_all(res), read_all(got), "reserved against grown")

        S = np.unique(lab[:total][(lab[:total] >= CLUSTER) & (lab[:total] < CLUSTER + 4096)])[::2]   # a call into room that remove_labels freed
        hit = np.flatnonzero(np.isin(lab[:total], S)).astype(np.uint32)
        assert len(hit) > more and len(hit) > len(S), "the list frees too little room, or no label that repeats"
        assert res.remove_labels(S) == len(hit) == res_twin.remove_labels(hit)
        assert_twin(res, res_twin, lab, "after remove_labels")
        again = q.vectors[hit[:more]]                                            # (each lands where a removed row stood: the room is there)
        add(res, form, again, lab[total:])
        add(res_twin, form, again, labels_offset=total)
        assert_twin(res, res_twin, lab, "after the add into freed room")
        assert res.relocations() == 0
        assert sum(res.partition_size(p) for p in range(q.K)) == total - len(hit) + more
    finally:
        for idx in (got, twin, res, res_twin):
            idx.close()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", ENGINES, ids=["adc8x8", "idx16x4"])
def test_a_flat_index_refuses_labels(case, form):
    q = shared(case)
    lab = make_labels(10, 1)
    idx = q.index(coarse=False)
    try:
        with pytest.raises(pyqadc.QadcError, match="qadc error -4:"):            # QADC_E_STATE, also while the index is empty
            add(idx, form, q.vectors[:10], lab)
        assert idx.partition_count() == 0
        add(idx, form, q.vectors[:10])
        before = read_all(idx)
        relocations = idx.relocations()
        with pytest.raises(pyqadc.QadcError, match="qadc error -4:"):
            add(idx, form, q.vectors[:10], lab)
        assert_partitions(read_all(idx), before, "after the refused call")
        assert before[0][1] is None and idx.relocations() == relocations
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("case", ENGINES, ids=["adc8x8", "idx16x4"])
def test_an_unlabelled_index_refuses_labels(case):
    q = shared(case)
    a, codes = q.encoded()
    order = np.argsort(a[:100], kind="stable")
    bounds = np.searchsorted(a[:100][order], np.arange(q.K + 1))
    idx = q.index()
    try:
        idx.add_partitions([codes[:100][order[bounds[k]:bounds[k + 1]]] for k in range(q.K)])   # no labels: keys are positions
        before = read_all(idx)
        with pytest.raises(pyqadc.QadcError, match="qadc error -4:"):
            idx.add_vectors(q.vectors[:10], labels=make_labels(10, 2))
        assert_partitions(read_all(idx), before, "after the refused call")
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("case", ENGINES, ids=["adc8x8", "idx16x4"])
def test_the_front_end_checks_the_label_array(case):
    import torch
    q = shared(case)
    lab = make_labels(10, 1)
    v = q.vectors[:10]
    tv = torch.from_numpy(v).to("cuda:0")
    tl = torch.from_numpy(lab.view(np.int32)).to("cuda:0")
    idx = q.index()
    try:
        for bad in (lab[:9], lab.astype(np.int64), lab.astype(np.int32), lab.reshape(2, 5), list(lab)):
            with pytest.raises(ValueError):
                idx.add_vectors(v, labels=bad)
        with pytest.raises(ValueError):
            idx.add_vectors(v, labels_offset=1, labels=lab)
        for bad in (tl[:9], tl.to(torch.int64), tl.to(torch.float32), lab):
            with pytest.raises(ValueError):
                idx.add_vectors_device(tv, labels=bad)
        with pytest.raises(ValueError):
            idx.add_vectors_device(tv, labels_offset=1, labels=tl)
        assert idx.partition_count() == 0                                        # nothing reached the library
    finally:
        idx.close()


# ---- 4. queries, a filter and a removal over the random labels ---------------------------------------------------------------

def search_world(case, form):
    n = 3000
    q = make_quantizers(case, n=n, seed=4)
    lab = make_labels(n, 4)
    idx = q.index(case[2])
    add(idx, form, q.vectors[:2000], lab[:2000])
    add(idx, form, q.vectors[2000:], lab[2000:])
    in_cluster = lab[(lab >= CLUSTER) & (lab < CLUSTER + 4096)]
    return q, lab, idx, np.unique(in_cluster)[::3]


@path_independent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES[:3], ids=IDS[:3])
def test_adc_scans_equal_the_oracle_over_the_partitions_read_back(po, case, form):
    nq, ma, R = 3, 3, 100
    shape = case[1][:2]
    q, lab, idx, S = search_world(case, form)
    f = None
    try:
        rng = np.random.default_rng(45)
        assign = np.stack([rng.permutation(q.K)[:ma] for _ in range(nq)]).astype(np.int32)
        tables = afc.rand_tables(rng, shape, nq, ma)

        def check(S, what):
            parts = read_all(idx)
            got = idx.query_scan(assign, tables.copy(), R)
            for i in range(nq):
                pc, pl = [parts[k][0] for k in assign[i]], [parts[k][1] for k in assign[i]]
                want = afc.unfiltered(po, shape, pc, pl, tables[i], R) if S is None else afc.expected(po, shape, pc, pl, tables[i], R, S, "exclude")
                afc.assert_heap(got, want, i, what)

        check(None, "plain")
        f = pyqadc.AdcFilter(S, "exclude")
        idx.set_filter(f)
        check(S, "filtered")
        idx.set_filter(None)
        assert idx.remove_labels(S) == np.isin(lab, S).sum()
        check(None, "after remove_labels")
        assert not np.isin(np.concatenate([l for _, l in read_all(idx)]), S).any()
    finally:
        idx.close()
        if f is not None:
            f.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES[3:], ids=IDS[3:])
def test_index_scans_equal_the_oracle_over_the_partitions_read_back(po, case, form):
    """the 4-bit index's own int8 scan, and the float scan with a filter through its view"""
    nq, ma, R, keep = 3, 4, 100, 0.5
    M = case[1][0]
    q, lab, idx, S = search_world(case, form)
    view, f = None, None
    try:
        rng = np.random.default_rng(46)
        assign = np.stack([rng.permutation(q.K)[:ma] for _ in range(nq)]).astype(np.int32)
        tables = afc.rand_tables(rng, (M, 4), nq, ma)

        def check_int8(what):
            parts = read_all(idx)
            idx.finalize(keep)
            res = idx.query_scan(assign, tables.copy(), R)
            for i in range(nq):
                want = po.query_scan(M, [parts[k][0] for k in assign[i]], [parts[k][1] for k in assign[i]], keep, list(range(ma)), tables[i].copy(), R)
                assert want["rc"] == res["status"][i] == 0, "%s query %d" % (what, i)
                n = res["sizes"][i]
                assert np.array_equal(res["keys"][i, :n], want["keys"]) and np.array_equal(res["values"][i, :n], want["values"]), "%s query %d" % (what, i)
            return parts

        parts = check_int8("plain")
        view = pyqadc.AdcIndex.view_of(idx)
        f = pyqadc.AdcFilter(S, "exclude")
        view.set_filter(f)
        got = view.query_scan(assign, tables.copy(), R)
        for i in range(nq):
            pc, pl = [parts[k][0] for k in assign[i]], [parts[k][1] for k in assign[i]]
            afc.assert_heap(got, afc.expected(po, (M, 4), pc, pl, tables[i], R, S, "exclude"), i, "filtered view")
        view.set_filter(None)
        view.close()
        view = None
        assert idx.remove_labels(S) == np.isin(lab, S).sum()
        check_int8("after remove_labels")
    finally:
        if view is not None:
            view.close()
        idx.close()
        if f is not None:
            f.close()
