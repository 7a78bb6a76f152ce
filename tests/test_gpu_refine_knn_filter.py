"""GPU: the exhaustive search under a key filter (qadc_refine_knn with a qadc_adc_filter; DESIGN.md sections 11.10 and 11.16): ALLOW
and EXCLUDE sets built from host and from device memory, spans inside, across and outside the store's key range, against the host
twin (refine::knn with refine::filter) and against the unfiltered search of a store built without the dropped rows.  Equality of
bits throughout."""
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


def key_sets(rng, lo, rows):
    keys = np.arange(lo, lo + rows, dtype=np.int64)
    return dict(inside=rng.choice(keys, rows // 3, replace=False),
                across=np.concatenate([np.arange(max(0, lo - 5), lo + 7), np.arange(lo + rows - 7, lo + rows + 5)]),
                outside=np.array([max(0, lo - 40), max(0, lo - 1), lo + rows, lo + rows + 33]),
                edges=np.array([lo, lo + rows - 1]),
                word=np.arange(lo + 32 - lo % 32, lo + 64 - lo % 32),
                empty=np.zeros(0, np.int64),
                all=keys)


@path_independent
@pytest.mark.parametrize("device_filter", [False, True], ids=["host-set", "device-set"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_filters_on_a_dense_store(pyqadc, twin, tmp_path, dtype, device_filter):
    rng = np.random.default_rng(71)
    dim, rows, lo = 65, 700, 1000
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    vec[300:310] = vec[5]
    q = rng.normal(size=(6, dim)).astype(np.float32)
    q[0] = vec[5]
    sets = key_sets(rng, lo, rows)
    ops = [kc.add(lo, vec)] + [kc.knn(q, R, (mode, s)) for mode in ("exclude", "allow") for s in sets.values() for R in (8, rows)]
    c = kc.case(False, dim, dtype, ops)
    (want,) = kc.run_twin(twin, tmp_path, [c])
    kc.assert_same(kc.run_store(pyqadc, c, device_filter=device_filter), want)
    kc.assert_same(kc.run_store(pyqadc, c, device_filter=device_filter, plan=(64, 4)), want, "chunks of 64 rows")
    size = {(op[3][0], name, op[2]): int(w["sizes"][0]) for op, w, name in
            zip(ops[1:], want, [n for _ in range(2) for n in sets for _ in range(2)])}
    assert size[("allow", "empty", rows)] == 0 and size[("exclude", "all", rows)] == 0 and size[("exclude", "empty", rows)] == rows
    assert size[("allow", "edges", rows)] == 2 and size[("exclude", "outside", rows)] == rows and size[("allow", "across", rows)] == 14


@path_independent
@pytest.mark.parametrize("mode", ["exclude", "allow"])
def test_a_filtered_search_is_the_search_of_a_store_without_the_dropped_rows(pyqadc, mode):
    rng = np.random.default_rng(72)
    dim, n = 128, 9000
    labels = rng.permutation(50000)[:n].astype(np.uint32)
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    q = rng.normal(size=(33, dim)).astype(np.float32)
    listed = rng.random(n) < 0.4
    extra = np.arange(50000, 50010, dtype=np.uint32)                                           # listed keys the store does not hold
    keep = listed if mode == "allow" else ~listed
    full, reduced = pyqadc.Refine(dim, "f32", keyed=True), pyqadc.Refine(dim, "f32", keyed=True)
    full.put(vec, labels)
    reduced.put(vec[keep], labels[keep])
    f = pyqadc.AdcFilter(np.concatenate([labels[listed], extra]), mode)
    for R in (1, 100, 1024):
        gk, gd, gs = full.knn(q, R, filter=f)
        wk, wd, ws = reduced.knn(q, R)
        assert kc.same(dict(keys=gk, dist=gd, sizes=gs), dict(keys=wk, dist=wd, sizes=ws)) is None, R
    f.close()                                                                                  # no use is counted on the filter
    full.close()
    reduced.close()
