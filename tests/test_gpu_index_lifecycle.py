"""Whole lives of the 4-bit index (pyqadc.Index; DESIGN.md sections 11.6 and 11.7): the sequences of tests/index_model.py —
add_vectors, reserve and remove_labels in the orders that leave one call's state to the next: an append into an arena region that
still holds old rows behind the span a removal zeroed, the move of add_partitions' own allocations into the arena with their full
sizes and after a removal shortened them, finalize and the byte-plane copy after a removal and an append.

Every comparison is for equality.  After every mutating call read_partition and read_codes equal the numpy model and a query is
refused until finalize.  At every check step the index is finalized (keep 0.5 and 0.01 in turn, 0.5 where the starts at 0.01 would
not fill a heap of 100: index_model.index4_keep) and query_scan equals the CPU oracle's scanner_4 (po.query_scan) on the model's
partitions, every query answered with status 0 wherever the index holds rows — tests/test_index_model_host.py shows on a CPU, with
the same probes, tables and keep values, that the rows each removal took were in those heaps.  A float-ADC view of the index is
searched under an exclude and an allow filter against adc_filter_compose.expected.  The start sizes alone have no oracle: they are compared with those of a fresh
index built from the model.  The long walks run once; the query checks of a short walk run under every scan path."""
import numpy as np
import pytest

import adc_filter_compose as fc
import index_model as im
import pyqadc
from helpers import float_tables, heaps_equal, path_independent, rand_codes
from test_gpu_adc_remove import check, model_remove
from test_gpu_index_add import SPLIT_TILE, Quantizers4, build_from_model

pytestmark = pytest.mark.gpu

NQ, MA = im.NQ, im.MA
# the calls that leave a finalized index finalized: a removal that hits nothing and, as test_gpu_index_add.py's
# test_a_move_of_the_partitions_asks_for_finalize_again has it, a reserve that has nothing to do
STAYS_FINALIZED = ("remove_nothing", "reserve_less")
UNCHANGED = ("refill_in_place", "remove", "remove_device", "empty_partition", "empty_index", "remove_nothing", "remove_found", "reserve_less")


class IndexWalk:
    """one 4-bit index, its model and the steps of its sequence"""

    def __init__(self, po, case, kind):
        import torch
        shape, start, seed = case
        M, _, dim = shape
        self.po, self.M = po, M
        q = self.q = im.quantizers(shape)
        assign, codes = q.encoded()                                              # pyqadc.ivf_encode, the stateless encoder
        assert np.array_equal(assign, im.host_assign(po, shape))                 # what the CPU test generated its sequences from
        self.steps = im.steps(seed, im.Profile(kind, assign, start, shape))
        self.model = im.Model(assign, codes)
        self.assign, self.tables = im.index4_inputs(shape, seed)
        self.queries = im.queries(q)
        self.tq = torch.from_numpy(self.queries).to("cuda:0")
        self.tv = torch.from_numpy(q.vectors).to("cuda:0")
        self.idx = q.index()
        self.finalized, self.last, self.keep = False, None, im.KEEPS[0]
        self.checks = self.answered = self.held_rows = self.views = self.refusals = 0
        self.found = None

    def close(self):
        self.idx.close()

    def query(self, R=100):
        return self.idx.query_scan(self.assign, self.tables.copy(), R)

    def walk(self):
        for at, st in enumerate(self.steps):
            self.what = "step %d (%s)" % (at, st["op"])
            self.run(st)
        # every query of every check on an index that held rows was answered, and its heap compared
        assert self.checks >= 3 and self.held_rows >= 3 and self.answered == 2 * NQ * self.held_rows
        assert self.views == 1 and self.found is not None

    def run(self, st):
        import torch
        op, idx, model, what = st["op"], self.idx, self.model, self.what
        if op == "check":
            self.check(st.get("view", False))
            return
        assert op in im.MUTATIONS, op
        moved = idx.relocations()
        if op == "start_partitions":
            parts = model.start(st["rows"], st["labels_offset"])
            idx.add_partitions([c for c, _ in parts], [l for _, l in parts])
        elif op in ("add", "refill_in_place", "overflow"):
            idx.add_vectors(self.q.vectors[st["rows"]], labels_offset=st["labels_offset"])
        elif op == "add_device":
            idx.add_vectors_device(self.tv[torch.from_numpy(st["rows"]).to("cuda:0")].contiguous(), labels_offset=st["labels_offset"])
        elif op in ("remove", "empty_partition", "empty_index"):
            assert idx.remove_labels(st["labels"]) == st["gone"], what
        elif op == "remove_device":
            t = torch.from_numpy(st["labels"].view(np.int32).copy()).to("cuda:0")
            assert idx.remove_labels_device(t) == st["gone"], what
        elif op == "remove_nothing":
            assert idx.remove_labels(st["labels"]) == 0 and idx.remove_labels([]) == 0, what
        elif op == "remove_found":
            self.keep = im.index4_keep(model.sizes(), self.assign, self.checks)  # the next check's, if the rows stayed
            self.finalize()
            before = self.oracle(100)
            allowed = im.found_filter(model.labels())
            view = pyqadc.AdcIndex.view_of(idx)                                  # a view again, after the mutations since the last one
            f = pyqadc.AdcFilter(allowed, "allow")
            try:
                view.set_filter(f)
                keys, _, sizes = view.search_device(self.tq, MA, 100)            # "remove what this search returned"
                assert int(sizes.min().item()) == 100
            finally:
                view.close()
                f.close()
            flat = keys.reshape(-1)
            self.found = flat.cpu().numpy().view(np.uint32)
            assert np.isin(self.found, allowed).all(), what
            # some of them are in the heaps of the check queries: the next check would notice a row that stayed
            assert all(w["rc"] == 0 for w in before) and np.isin(np.concatenate([w["keys"] for w in before]), self.found).any(), what
            gone = model.remove(self.found)
            assert gone >= 100                                                   # a heap holds distinct rows
            assert idx.remove_labels_device(flat) == gone, what
        elif op in ("reserve_more", "reserve_less"):
            idx.reserve(st["capacities"])
        gone = im.apply(model, st)
        assert gone is None or gone == st["gone"], what
        self.read_back()
        if op in UNCHANGED or st.get("fits") is True:
            assert idx.relocations() == moved, what
        if op == "overflow" or st.get("fits") == "moves":
            assert idx.relocations() > moved, what
        if op in STAYS_FINALIZED and self.finalized:
            after = self.query()                                                 # no second finalize, and the answers it gave before
            for name in ("keys", "values", "sizes", "status"):
                assert np.array_equal(after[name], self.last[name]), "%s: %s changed" % (what, name)
        else:
            self.finalized = False
            with pytest.raises(pyqadc.QadcError, match="finalize") as e:
                self.query()
            assert "qadc error %d:" % pyqadc.QADC_E_STATE in str(e.value), what
            self.refusals += 1

    def read_back(self):
        parts = self.model.parts
        check(self.idx, parts, self.what)
        for p, (codes, _) in enumerate(parts):
            if len(codes):
                assert np.array_equal(self.idx.read_codes(p, 0, len(codes)), codes), "%s: read_codes of partition %d" % (self.what, p)

    def finalize(self):
        self.idx.finalize(self.keep)
        self.finalized = True

    def oracle(self, R):
        """scanner_4::query_scan of every check query on the model, at the keep the index is finalized with"""
        codes, labels = [c for c, _ in self.model.parts], [l for _, l in self.model.parts]
        return [self.po.query_scan(self.M, codes, labels, self.keep, self.assign[i], self.tables[i].copy(), R) for i in range(NQ)]

    def check(self, with_view):
        idx, model, what = self.idx, self.model, self.what
        self.keep = im.index4_keep(model.sizes(), self.assign, self.checks)
        self.finalize()
        for R in (1, 100):
            res = self.query(R)
            for i, want in enumerate(self.oracle(R)):
                assert want["rc"] == res["status"][i], "%s: status of query %d, R=%d" % (what, i, R)
                assert want["rc"] == 0 or sum(model.sizes()) == 0, "%s: query %d is not answered, R=%d" % (what, i, R)
                if want["rc"] == 0:
                    assert heaps_equal(res["heaps"][i], (want["keys"], want["values"])), "%s: query %d, R=%d" % (what, i, R)
                    self.answered += 1
                    if self.found is not None:
                        assert not np.isin(res["heaps"][i][0], self.found).any(), "%s: a removed key is in a heap" % what
        self.last = res
        self.held_rows += sum(model.sizes()) > 0
        fresh = build_from_model(self.q, model.parts)                            # the start sizes have no oracle
        try:
            fresh.finalize(self.keep)
            assert [idx.start_size(p) for p in range(im.K)] == [fresh.start_size(p) for p in range(im.K)], what
        finally:
            fresh.close()
        if with_view:
            self.view()
        self.checks += 1

    def view(self):
        """a float-ADC view of the finalized index under an exclude and an allow filter; while it lives, mutations are refused"""
        po, idx, model, what = self.po, self.idx, self.model, self.what
        held = model.labels()
        rng = np.random.default_rng(len(held))
        S = rng.permutation(held)[:len(held) * 3 // 10]
        view = pyqadc.AdcIndex.view_of(idx)
        try:
            assign, tables = view.search_tables(self.queries, MA)
            for mode in ("exclude", "allow"):
                f = pyqadc.AdcFilter(S, mode)
                try:
                    view.set_filter(f)
                    got = view.search(self.queries, MA, 100)
                    assert np.array_equal(got[3], assign)
                    for i in range(NQ):
                        want = fc.expected(po, (self.M, 4), [model.parts[k][0] for k in assign[i]], [model.parts[k][1] for k in assign[i]],
                                           tables[i], 100, S, mode)
                        fc.assert_heap(got[:3], want, i, "%s: the view, %s" % (what, mode))
                finally:
                    view.set_filter(None)
                    f.close()
            for call, args in ((idx.remove_labels, (held[:5],)), (idx.add_vectors, (self.q.vectors[:5], 4000000)), (idx.reserve, ([70000] * im.K,))):
                with pytest.raises(pyqadc.QadcError, match="view"):
                    call(*args)
            self.read_back()
        finally:
            view.close()
        self.views += 1


@path_independent
@pytest.mark.parametrize("case", im.INDEX4_CASES, ids=im.case_id)
def test_a_whole_life_equals_the_model(po, case):
    """the mutation walk: every state of the long sequence, read back; the queries of its check steps take the library's default path"""
    walk = IndexWalk(po, case, "index4")
    try:
        walk.walk()
        assert walk.checks >= 10 and walk.refusals >= 10
    finally:
        walk.close()


@pytest.mark.parametrize("case", im.INDEX4_SHORT_CASES, ids=im.case_id)
def test_queries_along_a_short_life_equal_the_oracle(po, case):
    """the query walk: a few steps, under every scan path"""
    walk = IndexWalk(po, case, "index4_short")
    try:
        walk.walk()
    finally:
        walk.close()


def test_byte_plane_copy_after_remove_and_add(po):
    """test_gpu_index_remove.test_split_scan_after_remove's setup, lived on: the byte-plane copy that finalize builds follows the rows
    through a removal, an append into the room it freed and another removal, down to exactly one tile"""
    R, keep = 100, 0.01
    q = Quantizers4(16, 16, K=1, n=50, seed=9)                                   # one coarse centroid: add_vectors on a labelled partition
    a, new_codes = q.encoded()
    assert not a.any()
    n = SPLIT_TILE + 101
    rng = np.random.default_rng(18)
    codes = rand_codes(rng, n, 16)
    labels = rng.permutation(3 * n)[:n].astype(np.uint32)
    tables = float_tables(np.random.default_rng(5), 3, 1, 16)
    idx = q.index()
    try:
        for k, v in dict(share_variant=0, mq=0, front_run_max=0, wgq=0).items():   # one query per pass: the launches that read the copy
            idx.set_option(k, v)
        idx.set_split(1, 1)
        model = [(codes, labels)]

        def finalized(rows, what):
            idx.finalize(keep)
            assert len(model[0][0]) == rows and idx.partition_size(0) == rows, what
            assert idx.profile()["split_copy_bytes"] == -(-rows // SPLIT_TILE) * 7 * SPLIT_TILE, what   # 7 planes of whole tiles
            got_codes, got_labels = idx.read_partition(0)
            assert np.array_equal(got_codes, model[0][0]) and np.array_equal(got_labels, model[0][1]), what
            res = idx.query_scan(np.zeros((3, 1), np.int32), tables.copy(), R)
            for i in range(3):
                want = po.query_scan(16, [model[0][0]], [model[0][1]], keep, [0], tables[i].copy(), R)
                assert want["rc"] == res["status"][i] == 0, what
                assert heaps_equal(res["heaps"][i], (want["keys"], want["values"])), "%s: query %d" % (what, i)

        idx.add_partitions([codes], [labels])
        finalized(SPLIT_TILE + 101, "add_partitions")
        removed = model[0][1][rng.permutation(n)[:100]]
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == 100
        finalized(SPLIT_TILE + 1, "100 rows removed")
        idx.add_vectors(q.vectors, labels_offset=3 * n + 7)
        model = [(np.concatenate([model[0][0], new_codes]), np.concatenate([model[0][1], (np.arange(50) + 3 * n + 7).astype(np.uint32)]))]
        finalized(SPLIT_TILE + 51, "50 rows appended")
        removed = np.concatenate([model[0][1][-30:], model[0][1][rng.permutation(SPLIT_TILE)[:21]]])
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == 51
        finalized(SPLIT_TILE, "51 rows removed: one whole tile")
    finally:
        idx.close()
