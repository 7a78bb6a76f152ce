"""GPU: the exhaustive search over a KEYED refine store (DESIGN.md sections 11.14 and 11.16) against the host twin
(refine::knn over refine::keyed_store): the kernel walks the rows allocated so far, reads a row's key from row_key and skips the free
rows, so the lives here leave free rows between live ones, reuse them, relocate the rows and empty the store.  A life is a script
in the style of tests/refine_keyed_cases.py (tests/refine_knn_cases.py); every comparison is for equality of bits."""
import numpy as np
import pytest

import refine_knn_cases as kc
from helpers import path_independent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return kc.build_driver()


@path_independent
@pytest.mark.parametrize("plan", [(0, 0), (64, 3)], ids=["default", "chunks-of-64"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_life_with_free_rows_between_live_ones(pyqadc, twin, tmp_path, dtype, plan):
    rng = np.random.default_rng(61)
    dim, n = 65, 900
    labels = rng.choice(2 ** 32 - 1, n, replace=False).astype(np.uint32)
    labels[:4] = (0, 0xFFFFFFFE, 0xFFFFFFFD, 0x80000000)                                       # keys near 0xFFFFFFFE
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    q = rng.normal(size=(7, dim)).astype(np.float32)
    q[0] = vec[1]
    ops = [kc.knn(q, 5),                                                                       # empty
           kc.put(labels[:600], vec[:600]), kc.knn(q, 10), kc.knn(q, 600),
           kc.remove(labels[1:500:2]), kc.knn(q, 10), kc.knn(q, 351),                          # every second row free
           kc.put(labels[100:200], vec[300:400]), kc.knn(q, 10),                               # overwrites, and free rows taken back
           kc.put(labels[600:], vec[600:]), kc.knn(q, 1000),                                   # new keys: the rest of the free rows, then new rows
           kc.remove(labels), kc.knn(q, 4),                                                    # remove everything
           kc.put(labels[:3], vec[:3]), kc.knn(q, 4)]
    c = kc.case(True, dim, dtype, ops)
    (want,) = kc.run_twin(twin, tmp_path, [c])
    st = kc.make_store(pyqadc, c)
    kc.assert_same(kc.run_store(pyqadc, c, plan=plan, st=st), want)
    info = st.keyed_info()
    st.close()
    assert info["live"] == 3 and info["rows_free"] > 0
    assert want[0]["sizes"].tolist() == [0] * 7 and want[-2]["sizes"].tolist() == [0] * 7 and want[-1]["sizes"].tolist() == [3] * 7
    assert want[2]["sizes"].tolist() == [600] * 7 and want[4]["sizes"].tolist() == [350] * 7
    assert want[1]["keys"][0, 0] == 0xFFFFFFFE


@path_independent
def test_after_a_relocation(pyqadc, twin, tmp_path):
    rng = np.random.default_rng(62)
    dim = 16
    labels = rng.permutation(100000)[:9000].astype(np.uint32)
    vec = rng.normal(size=(9000, dim)).astype(np.float32)
    q = rng.normal(size=(33, dim)).astype(np.float32)
    ops = [kc.put(labels[:100], vec[:100]), kc.knn(q, 20), kc.remove(labels[:100:3]), kc.put(labels[100:], vec[100:]), kc.knn(q, 20),
           kc.knn(q[:2], 1024)]
    c = kc.case(True, dim, "f32", ops)
    (want,) = kc.run_twin(twin, tmp_path, [c])
    st = kc.make_store(pyqadc, c)
    kc.assert_same(kc.run_store(pyqadc, c, st=st), want)
    assert st.relocations() >= 1 and st.keyed_info()["rows_allocated"] > kc.CHUNK              # the rows moved; more than one group
    st.close()
