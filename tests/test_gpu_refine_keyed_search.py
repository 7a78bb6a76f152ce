"""GPU: one life of an index and a keyed refine store under the caller's own labels (DESIGN.md sections 11.5, 11.6 and 11.14), on
the small world of tests/test_gpu_refine_search.py: 20 000 clustered 32-d vectors, K = 16.

  1. labelled add with a random injective label map        (AdcIndex 8x8; Index 16x4, searched itself and through its view)
  2. put of the same labels into a keyed store
  3. search_refined / search_refined_device
  4. remove_labels on the index and remove on the store, for a third of the labels
  5. search again
  6. labelled add of half of those labels with new vectors, and their put
  7. search again — and once more after a removal from the store alone

After every search the refined result equals the twin's rerank (refine::keyed_store, tests/cpp/refine_keyed_host.cpp) of the keys
that same search returned.  missing is 0 whenever the index and the store hold the same labels, and the twin's count after the
removal from the store alone."""
import numpy as np
import pytest

import refine_cases as rc
import refine_keyed_cases as kc
from helpers import path_independent
from test_gpu_refine_search import DIM, N, NQ, World, as_result

pytestmark = pytest.mark.gpu

MA, R = 4, 100


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return kc.build_driver()


@pytest.fixture(scope="module")
def world(pyqadc):
    w = World(pyqadc)
    yield w
    w.close()


class Adc:
    """the 8x8 float-ADC index: the refined search in its host and device form"""
    r_in = 400

    def __init__(self, world):
        self.world = world
        self.idx = world.pyqadc.AdcIndex(8, 8)
        self.idx.set_pq(world.cb8)
        self.idx.set_coarse(world.coarse)

    def searches(self, store):
        """-> [(the twin's rerank operation on what a search returned, the refined result)]"""
        import torch
        q = self.world.queries
        keys, vals, _, _ = self.idx.search(q, MA, self.r_in)
        op = kc.rerank(q, keys, R, values=vals)
        return [(op, as_result(*self.idx.search_refined(q, MA, R, self.r_in, store))),
                (op, as_result(*self.idx.search_refined_device(torch.from_numpy(q).cuda(), MA, R, self.r_in, store)))]


class Index4:
    """the 16x4 index: its own search (counts, no values), and the float scan of a view of it"""
    r_in = 1000

    def __init__(self, world):
        self.world = world
        self.idx = world.pyqadc.Index(16)
        self.idx.set_pq(world.cb4)
        self.idx.set_coarse(world.coarse)

    def searches(self, store):
        import torch
        q = self.world.queries
        self.idx.finalize(1.0)
        found = self.idx.search(q, MA, self.r_in)
        assert (found["status"] == 0).all() and (found["sizes"] == self.r_in).all()
        out = [(kc.rerank(q, found["keys"], R, counts=found["sizes"]), as_result(*self.idx.search_refined(q, MA, R, self.r_in, store)))]
        view = self.world.pyqadc.AdcIndex.view_of(self.idx)
        try:
            keys, vals, _, _ = view.search(q, MA, 400)
            op = kc.rerank(q, keys, R, values=vals)
            out.append((op, as_result(*view.search_refined(q, MA, R, 400, store))))
            out.append((op, as_result(*view.search_refined_device(torch.from_numpy(q).cuda(), MA, R, 400, store))))
        finally:
            view.close()                                                         # (the index takes no add or removal while a view lives)
        return out


def live_one_life(world, twin, tmp_path, engine, dtype):
    rng = np.random.default_rng(51)
    labels = np.unique(rng.integers(0, 0xFFFFFFFF, 2 * N, dtype=np.uint64).astype(np.uint32))
    labels = rng.permutation(labels)[:N]                                         # an injective map, sparse over all 32 bits
    store = world.pyqadc.Refine(DIM, dtype, keyed=True)
    script = []

    def check(what, missing=0):
        pairs = engine.searches(store)
        want = kc.run_twin(twin, tmp_path, DIM, dtype, script + [op for op, _ in pairs])[len(script):]
        for i, ((_, got), w) in enumerate(zip(pairs, want)):
            assert rc.same(got, w) is None, "%s, search %d: %s differs from the twin" % (what, i, rc.same(got, w))
            assert (w["missing"] == 0) == (missing == 0), "%s, search %d: %d keys missing" % (what, i, w["missing"])
            assert missing or (w["sizes"] == R).all()
        return want

    def both(vectors, lab):
        engine.idx.add_vectors(vectors, labels=lab)
        store.put(vectors, lab)
        script.append(kc.put(lab, vectors))

    try:
        both(world.vectors, labels)                                              # 1, 2
        check("after the build")                                                 # 3
        third = labels[rng.permutation(N)[:N // 3]]
        assert engine.idx.remove_labels(third) == len(third) == store.remove(third)   # 4
        script.append(kc.remove(third))
        want = check("after the removal")                                        # 5
        assert not np.isin(want[0]["keys"], third).any()
        back = third[:len(third) // 2]                                           # 6: half of them again, with new vectors
        moved = (world.vectors[rng.integers(0, N, len(back))] + 0.1 * rng.normal(size=(len(back), DIM))).astype(np.float32)
        both(moved, back)
        want = check("after the second add")                                     # 7
        assert np.isin(want[0]["keys"], back).any(), "no re-added vector among the results: the case is vacuous"
        info = store.keyed_info()
        assert info["live"] == N - len(third) + len(back) and info["rows_allocated"] == N and info["rows_free"] == len(third) - len(back)
        gone = want[0]["keys"][:, :3].reshape(-1)                                # from the store alone: the best three of every query
        assert store.remove(gone) == len(np.unique(gone))
        script.append(kc.remove(gone))
        want = check("after a removal from the store alone", missing=1)
        assert all(w["missing"] >= NQ * 3 for w in want[:1]) and not np.isin(want[0]["keys"], gone).any()
    finally:
        store.close()
        engine.idx.close()


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_an_adc_index_and_a_keyed_store_under_the_callers_labels(world, twin, tmp_path, dtype):
    live_one_life(world, twin, tmp_path, Adc(world), dtype)


def test_a_4bit_index_and_a_keyed_store_under_the_callers_labels(world, twin, tmp_path, scan_path):
    live_one_life(world, twin, tmp_path, Index4(world), "f32")
