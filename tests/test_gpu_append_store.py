"""The seams of the shared append flow (quick-adc_amd/csrc/qadc_append.h over RowStore; DESIGN.md sections 11.5 and 11.6), on both
engines: the calls in which the float-ADC engine and the 4-bit index once ran code of their own and no other test looks — a call
of zero vectors into an index without partitions, and into a 4-bit index whose partitions are still allocations of their own;
reserve creating the partitions; a refused call between two good ones.  Tiny shapes (K = 8, at most 200 vectors): what is checked
is the host flow, the kernels have tests/test_gpu_adc_add.py and tests/test_gpu_index_add.py.

Every refusal here is an argument check that returns before the device is touched."""
import numpy as np
import pytest

import adc_filter_compose as fc
import pyqadc
from helpers import float_tables, heaps_equal, path_independent
from test_gpu_adc_add import Quantizers, append, assert_partitions, group, read_all
from test_gpu_index_add import Quantizers4, build_from_model

pytestmark = pytest.mark.gpu

K, N = 8, 200
ENGINES = ["adc", "idx"]                                                         # float ADC 8x8 at dim 64, the 4-bit index 16x4 at dim 16
_shared = {}


def quantizers(engine):
    if engine not in _shared:
        _shared[engine] = Quantizers(8, 8, 64, K=K, n=N, seed=12) if engine == "adc" else Quantizers4(16, 16, K=K, n=N, seed=12)
    return _shared[engine]


def none(q):
    return np.zeros((0, q.dim), np.float32)


def assert_empty(idx, parts):
    assert idx.partition_count() == parts and [idx.partition_size(p) for p in range(parts)] == [0] * parts


# ---- 1. zero vectors into an index without partitions -------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("engine", ENGINES)
def test_zero_vectors_into_a_fresh_index_create_the_partitions(engine):
    q = quantizers(engine)
    a, codes = q.encoded()
    idx = q.index()
    try:
        idx.add_vectors(none(q))
        assert_empty(idx, K)
        assert idx.relocations() == 0
        idx.add_vectors(q.vectors[:100])
        want = group(a[:100], codes[:100], K)
        assert_partitions(read_all(idx), want, "after 100 vectors")
        assert idx.relocations() == 1
        idx.add_vectors(none(q))                                                 # nothing to do
        idx.add_vectors_raw(None, 0, 5, 0)
        assert_partitions(read_all(idx), want, "after a second call of zero vectors")
        assert idx.relocations() == 1
    finally:
        idx.close()


# ---- 2. zero vectors into a 4-bit index whose partitions are allocations of their own -------------------------------------------

def test_zero_vectors_consolidate_a_built_index_and_change_no_row():
    q = quantizers("idx")
    a, codes = q.encoded()
    model = group(a[:150], codes[:150], K, 3)
    rng = np.random.default_rng(21)
    assign = np.stack([rng.permutation(K)[:4] for _ in range(3)]).astype(np.int32)
    tables = float_tables(rng, 3, 4, 16)
    idx = build_from_model(q, model)
    try:
        idx.finalize(0.5)
        before = idx.query_scan(assign, tables.copy(), 10)
        assert (before["status"] == 0).all()
        idx.add_vectors(none(q))
        assert_partitions(read_all(idx), model, "after the call")
        assert idx.relocations() == 0
        with pytest.raises(pyqadc.QadcError, match="finalize"):                  # the partitions moved into the store
            idx.query_scan(assign, tables.copy(), 10)
        idx.finalize(0.5)
        after = idx.query_scan(assign, tables.copy(), 10)
        for name in ("keys", "values", "sizes", "status"):
            assert np.array_equal(after[name], before[name]), name
    finally:
        idx.close()


# ---- 3. reserve creates the partitions ---------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("engine", ENGINES)
def test_reserve_creates_partitions_and_the_adds_behind_it_never_move(engine):
    q = quantizers(engine)
    a, codes = q.encoded()
    lab = np.random.default_rng(31).integers(0, 1 << 32, 80, dtype=np.uint64).astype(np.uint32)
    lab[5] = lab[6] = 0xFFFFFFFF
    idx = q.index()
    try:
        idx.reserve([10, 0, 10])                                                 # on an index without partitions
        assert_empty(idx, 3)
        idx.reserve([N] * K)                                                     # ... and on one that has fewer
        assert_empty(idx, K)
        assert idx.relocations() == 0
        idx.add_vectors(q.vectors[:80], labels=lab)
        want = [(c, lab[l]) for c, l in group(a[:80], codes[:80], K)]
        assert_partitions(read_all(idx), want, "after the labelled add")
        idx.add_vectors(q.vectors[80:150], labels_offset=80)
        want = append(want, group(a[80:150], codes[80:150], K, 80))
        assert_partitions(read_all(idx), want, "after the plain add")
        assert idx.relocations() == 0
    finally:
        idx.close()


# ---- 4. a refused call in the middle of a life ---------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", ENGINES)
def test_a_refused_call_between_two_adds_changes_nothing(po, engine):
    q = quantizers(engine)
    a, codes = q.encoded()
    nine = np.concatenate([q.coarse, q.coarse[:1] + 100]).astype(np.float32)
    idx = q.index()
    try:
        idx.add_vectors(q.vectors[:100])
        assert idx.relocations() == 1
        model = group(a[:100], codes[:100], K)
        with pytest.raises(pyqadc.QadcError, match="sum_mode is 0") as e:
            idx.add_vectors(q.vectors[100:150], labels_offset=100, sum_mode=2)
        assert "qadc error %d:" % pyqadc.QADC_E_ARG in str(e.value)
        idx.set_coarse(nine)
        with pytest.raises(pyqadc.QadcError, match="the coarse quantizer has 9 centroids and the index 8 partitions") as e:
            idx.add_vectors(q.vectors[100:150], labels_offset=100)
        assert "qadc error %d:" % pyqadc.QADC_E_ARG in str(e.value)
        idx.set_coarse(q.coarse)
        assert_partitions(read_all(idx), model, "after the refusals")
        assert idx.relocations() == 1
        idx.add_vectors(q.vectors[100:150], labels_offset=100)
        model = append(model, group(a[100:150], codes[100:150], K, 100))
        assert_partitions(read_all(idx), model, "after the second add")
        rng = np.random.default_rng(41)
        if engine == "adc":
            queries = (q.coarse[rng.integers(0, K, 3)] + rng.normal(size=(3, q.dim))).astype(np.float32)
            assign, tables = idx.search_tables(queries, 4)
            got = idx.search(queries, 4, 10)
            assert np.array_equal(got[3], assign)
            for i in range(3):
                want = fc.unfiltered(po, (8, 8), [model[k][0] for k in assign[i]], [model[k][1] for k in assign[i]], tables[i], 10)
                fc.assert_heap(got[:3], want, i, "search after the second add")
        else:
            assign = np.stack([rng.permutation(K)[:4] for _ in range(3)]).astype(np.int32)
            tables = float_tables(rng, 3, 4, 16)
            idx.finalize(0.5)
            res = idx.query_scan(assign, tables.copy(), 10)
            for i in range(3):
                want = po.query_scan(16, [c for c, _ in model], [l for _, l in model], 0.5, assign[i], tables[i].copy(), 10)
                assert want["rc"] == res["status"][i] == 0, i
                assert heaps_equal(res["heaps"][i], (want["keys"], want["values"])), i
    finally:
        idx.close()
