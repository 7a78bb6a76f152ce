"""GPU: keys that reach a query through several rows, keys the store does not hold and probe lists that repeat (qadc_refine_knn_probed;
DESIGN.md section 11.22), against the host twin.  A label may stand in two probed partitions and twice inside one; counted twice among
the first R of a buffer it would displace the true R-th word, so the selects drop equal words before they count — with chunks of 64
rows the copies meet in one buffer, in two groups and in two launches.  And with every partition probed and the store's keys as labels
the call is Refine.knn, bits and all."""
import numpy as np
import pytest

import refine_knn_cases as kc
import refine_probe_cases as pc
from helpers import path_independent

pytestmark = pytest.mark.gpu
K = len(pc.SIZES)


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return pc.build_driver()


def dup_case(rng, dim, dtype, keyed):
    """the store holds the keys 0 .. 1063; the index's labels are those keys, row by row, but: the key of partition 3's row 7 also
    stands at partition 4's row 9 (two partitions: two groups), at partition 4's rows 20 and 41 (one chunk of 64: one buffer) and at
    partition 4's row 600 (another launch at chunks of 64); query 0 is that key's vector, so the copies are the nearest words"""
    n = sum(pc.SIZES)
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    labels = np.arange(n, dtype=np.uint32)
    key = labels[64 + 7]
    for row in (9, 20, 41, 600):
        labels[364 + row] = key
    labels[364 + 100:364 + 110] = np.arange(7000, 7010)                      # labels the store does not hold
    labels[64 + 50] = 0xFFFFFFFF
    q = rng.normal(size=(4, dim)).astype(np.float32)
    q[0] = vec[key]
    everything = np.tile(np.arange(K, dtype=np.int32), (4, 1))
    calls = []
    for R in (1, 2, 3, 5, 64, 1024):                                          # R = 2 .. 5: the copies would fill the first R by themselves
        calls += [pc.call(q, [[3, 4]] * 4, R), pc.call(q, [[4, 3]] * 4, R), pc.call(q, [[4, 4]] * 4, R), pc.call(q, everything, R)]
    calls.append(pc.call(q, [[3, 4, 3, 4, 2]] * 4, 3))                        # repeats: a partition counts once
    ops = [pc.put(np.arange(n, dtype=np.uint32), vec)] if keyed else [pc.add(0, vec)]
    return pc.case(keyed, dim, dtype, ops, pc.split_labels(labels), calls), int(key)


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_key_reached_through_several_rows_is_kept_once(pyqadc, twin, tmp_path, dtype, keyed):
    rng = np.random.default_rng(21 + keyed)
    c, key = dup_case(rng, 64, dtype, keyed)
    (want,) = pc.run_twin(twin, tmp_path, [c])
    # the twin keeps the key once and fills the first R with distinct keys; every entry it misses is counted
    for w in want:
        for row, size in zip(w["keys"], w["sizes"]):
            assert len(set(row[:size].tolist())) == size
    assert want[4]["keys"][0, 0] == key and want[4]["sizes"][0] == 2 and want[0]["missing"] == 4 * 11 and want[2]["missing"] == 4 * 10
    for plan in (None, (64, 0), (64, 1), (1, 0)):
        pc.assert_same(pc.run_gpu(pyqadc, c, plan=plan), want, "plan %s" % (plan,))
    pc.assert_same(pc.run_gpu(pyqadc, c, plan=(64, 0), device=True), want, "device form")


@path_independent
def test_the_device_form_skips_a_probe_that_is_no_partition_and_the_host_form_refuses_it(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(4)
    q = rng.normal(size=(5, 32)).astype(np.float32)
    a = np.array([[3, 3], [-1, 4], [K, 2], [2 ** 31 - 1, -2 ** 31], [4, 2]], np.int32)
    c = pc.dense_case(rng, 32, "f32", lambda vec, labels: [pc.call(q, a, 10)])
    (want,) = pc.run_twin(twin, tmp_path, [c])
    assert want[0]["sizes"].tolist() == [10, 10, 10, 0, 10]
    pc.assert_same(pc.run_gpu(pyqadc, c, device=True), want, "device form")
    with pytest.raises(pyqadc.QadcError):
        pc.run_gpu(pyqadc, c)
    c["calls"] = [pc.call(q[:1], a[:1], 10), pc.call(q[4:], a[4:], 10)]
    pc.assert_same(pc.run_gpu(pyqadc, c), pc.run_twin(twin, tmp_path, [c])[0], "host form, a repeat")


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_every_partition_probed_with_the_stores_keys_as_labels_is_knn(pyqadc, dtype):
    rng = np.random.default_rng(13)
    dim, n = 128, sum(pc.SIZES)
    q = rng.normal(size=(33, dim)).astype(np.float32)
    everything = np.tile(np.arange(K, dtype=np.int32), (33, 1))
    flt = None
    c = pc.dense_case(rng, dim, dtype, lambda vec, labels: [], lo=40)
    st, idx = pc.make_store(pyqadc, c), pc.make_index(pyqadc, c["parts"])
    try:
        flt = pyqadc.AdcFilter(np.arange(40, 40 + n, 3, dtype=np.uint32), "allow", device=st.device)
        for f in (None, flt):
            for R in (1, 100, 1024):
                k, d, s, missing = st.knn_probed(idx, q, everything, R, filter=f)
                wk, wd, ws = st.knn(q, R, filter=f)
                assert missing == 0 and kc.same(dict(keys=k, dist=d, sizes=s), dict(keys=wk, dist=wd, sizes=ws)) is None
    finally:
        idx.close()
        st.close()
        if flt is not None:
            flt.close()
