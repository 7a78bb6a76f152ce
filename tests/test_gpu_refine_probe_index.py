"""GPU: the probed exact search reads its index as it is at the call (qadc_refine_knn_probed): an owned 8-bit
index with labels and without (key = position in the partition), a 16-bit index, a view of a 16x4 4-bit index with labels and with
key bases; dense and keyed stores, a keyed one with free rows and after overwrites; the candidates follow remove_labels and
add_vectors(labels=) on the index; a filter on the index, on the call, on both, and an empty ALLOW.  The partitions the twin is given
are read back from the index itself (read_partition), so every result is the twin's, bit for bit."""
import numpy as np
import pytest

import refine_probe_cases as pc
from helpers import path_independent

pytestmark = pytest.mark.gpu
K = len(pc.SIZES)
N = sum(pc.SIZES)
DIM = 16


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return pc.build_driver()


def store_case(rng, keyed, dtype="f32", lo=0):
    """a store of the keys lo .. lo + N; keyed: put in two halves, a third of the keys removed, some put back with other vectors
    (free rows reused, rows overwritten)"""
    vec = rng.normal(size=(N, DIM)).astype(np.float32)
    keys = np.arange(lo, lo + N, dtype=np.uint32)
    kw = dict(zip(("vmin", "step"), pc.sq_params(vec))) if dtype == "sq8" else {}
    if not keyed:
        return pc.case(False, DIM, dtype, [pc.add(lo, vec)], [], [], **kw)
    ops = [pc.put(keys[:600], vec[:600]), pc.remove(keys[100:400:3]), pc.put(keys[600:], vec[600:]), pc.put(keys[90:130], vec[500:540] + np.float32(1)),
           pc.remove(keys[1000:1010])]
    return pc.case(True, DIM, dtype, ops, [], [], **kw)


def calls_of(rng, nq=9):
    q = rng.normal(size=(nq, DIM)).astype(np.float32)
    return [pc.call(q, pc.probes(rng, nq, ma, K), R) for ma in (1, 2, K) for R in (10, 400)]


def check_on(pyqadc, twin, tmp_path, c, idx, parts=None, what=""):
    """the case's calls on the store the case describes and on `idx`, whose partitions the twin reads as `parts` (default: read back)"""
    c = dict(c, parts=pc.parts_of(idx) if parts is None else parts)
    (want,) = pc.run_twin(twin, tmp_path, [c])
    st = pc.make_store(pyqadc, c)
    try:
        pc.assert_same(pc.run_calls(pyqadc, st, idx, c["calls"]), want, what + " host form")
        pc.assert_same(pc.run_calls(pyqadc, st, idx, c["calls"], device=True), want, what + " device form")
    finally:
        st.close()
    return want


def labelled_parts(rng, lo=0):
    return pc.split_labels(rng.permutation(np.arange(lo, lo + N, dtype=np.uint32)))


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_an_owned_8_bit_index_labelled_and_unlabelled(pyqadc, twin, tmp_path, dtype, keyed):
    rng = np.random.default_rng(3 + keyed)
    c = dict(store_case(rng, keyed, dtype), calls=calls_of(rng))
    idx = pc.make_index(pyqadc, labelled_parts(rng))
    try:
        want = check_on(pyqadc, twin, tmp_path, c, idx, what="labelled")
        assert (want[5]["missing"] > 0) == keyed
    finally:
        idx.close()
    idx = pc.make_index(pyqadc, [pc.part(None, 0, n) for n in pc.SIZES])     # key = position: the partitions' keys overlap
    try:
        want = check_on(pyqadc, twin, tmp_path, c, idx, what="unlabelled")
        assert max(int(w["keys"][w["keys"] != pc.NO_KEY].max()) for w in want) < 700
    finally:
        idx.close()


@path_independent
def test_a_16_bit_index(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(5)
    parts = labelled_parts(rng)
    idx = pyqadc.AdcIndex.create16(2)
    try:
        idx.add_partitions([rng.integers(0, 65536, (p[2], 2)).astype(np.uint16) for p in parts], [p[0] for p in parts])
        check_on(pyqadc, twin, tmp_path, dict(store_case(rng, False), calls=calls_of(rng)), idx, what="16-bit")
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("labelled", [True, False], ids=["labels", "key-bases"])
def test_a_view_of_a_4_bit_index(pyqadc, twin, tmp_path, labelled):
    rng = np.random.default_rng(6)
    parts = labelled_parts(rng) if labelled else [pc.part(None, base, n) for base, n in zip((0, 5, 100, 40, 364), pc.SIZES)]
    src = pyqadc.Index(16)
    src.add_partitions([rng.integers(0, 256, (p[2], 8), dtype=np.uint8) for p in parts], [p[0] for p in parts] if labelled else None)
    for p, part in enumerate(parts):
        if not labelled:
            src.set_key_base(p, part[1])
    src.finalize(0.01)
    view = pyqadc.AdcIndex.view_of(src)
    try:
        check_on(pyqadc, twin, tmp_path, dict(store_case(rng, False), calls=calls_of(rng)), view, parts=parts, what="view")
    finally:
        view.close()
        src.close()


@path_independent
def test_the_candidates_follow_the_index(pyqadc, twin, tmp_path):
    """remove_labels takes rows out of the partitions and add_vectors(labels=) appends rows to them: the next call sees both"""
    rng = np.random.default_rng(7)
    c = dict(store_case(rng, False), calls=calls_of(rng))
    parts = labelled_parts(rng)
    idx = pc.make_index(pyqadc, parts)
    try:
        idx.set_pq(rng.normal(size=(8, 256, DIM // 8)).astype(np.float32))
        idx.set_coarse(rng.normal(size=(K, DIM)).astype(np.float32))
        before = check_on(pyqadc, twin, tmp_path, c, idx, what="before")
        gone = np.concatenate([parts[4][0][::2], parts[2][0][:10]])
        assert idx.remove_labels(gone) == len(gone)
        after = check_on(pyqadc, twin, tmp_path, c, idx, what="after remove_labels")
        assert not np.isin(after[5]["keys"], gone).any() and np.isin(before[5]["keys"], gone).any()
        back = gone[:200]
        idx.add_vectors(rng.normal(size=(len(back), DIM)).astype(np.float32), labels=back)
        assert sum(idx.partition_size(p) for p in range(K)) == N - len(gone) + len(back)
        again = check_on(pyqadc, twin, tmp_path, c, idx, what="after add_vectors")
        assert np.isin(again[5]["keys"], back).any()
    finally:
        idx.close()


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_a_filter_on_the_index_on_the_call_and_on_both(pyqadc, twin, tmp_path, keyed):
    rng = np.random.default_rng(9)
    parts = labelled_parts(rng)
    q = rng.normal(size=(9, DIM)).astype(np.float32)
    a = pc.probes(rng, 9, 3, K)
    some, other = rng.choice(N, 500, replace=False).astype(np.uint32), rng.choice(N, 500, replace=False).astype(np.uint32)
    filters = (None, ("exclude", some), ("allow", some), ("allow", []), ("exclude", []))
    for on_index in filters:
        c = dict(store_case(rng, keyed), parts=parts, index_filter=pc._filter(on_index),
                 calls=[pc.call(q, a, 50, f) for f in (None, ("exclude", other), ("allow", other), ("allow", []))])
        (want,) = pc.run_twin(twin, tmp_path, [c])
        pc.assert_same(pc.run_gpu(pyqadc, c), want, "index filter %s" % (on_index and on_index[0],))
        assert want[3]["sizes"].max() == 0 and want[3]["missing"] == 0
        if on_index is not None and on_index[0] == "allow" and len(on_index[1]):
            assert np.isin(want[1]["keys"][want[1]["keys"] != pc.NO_KEY], np.setdiff1d(some, other)).all()


@path_independent
def test_what_the_call_refuses(pyqadc):
    rng = np.random.default_rng(2)
    c = store_case(rng, False)
    st, idx = pc.make_store(pyqadc, c), pc.make_index(pyqadc, labelled_parts(rng))
    q, a = np.zeros((2, DIM), np.float32), np.zeros((2, 1), np.int32)
    try:
        for bad in (lambda: st.knn_probed_raw(None, 2, q, 1, a, 5), lambda: st.knn_probed_raw(idx, 2, q, 0, a, 5),
                    lambda: st.knn_probed_raw(idx, 2, q, K + 1, np.zeros((2, K + 1), np.int32), 5), lambda: st.knn_probed_raw(idx, 2, q, 1, a, 0),
                    lambda: st.knn_probed_raw(idx, 2, q, 1, a, 1025), lambda: st.knn_probed_raw(idx, 2, q, 1, None, 5),
                    lambda: st.knn_probed_raw(idx, 2, None, 1, a, 5), lambda: st.knn_probed_raw(idx, 2, q, 1, a, 5, outputs=False),
                    lambda: st.knn_probed_raw(idx, -1, q, 1, a, 5), lambda: st.knn_probed(idx, q, [[K], [0]], 5)):
            with pytest.raises(pyqadc.QadcError):
                bad()
        k, d, s, m = st.knn_probed_raw(idx, 0, None, 1, None, 5)
        assert k.shape == (0, 5) and m == 0
    finally:
        idx.close()
        st.close()
