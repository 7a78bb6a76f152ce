"""Whole lives of a float-ADC index (pyqadc.AdcIndex; DESIGN.md sections 11.5, 11.7 and 11.10): the sequences of
tests/index_model.py — add_vectors, reserve, remove_labels, add_partitions, filters and finishes in the orders that leave one call's
state to the next: capacities above sizes, stale rows behind the new end, a label buffer reserved before the index had labels, an
emptied partition or index that is filled again, partitions that pass kRemoveTile and kAddTile in both directions.

Every comparison is for equality.  After every mutating call the partitions read back (read_partition) equal the numpy model, and
the calls' return values and relocations() are what the model says.  At every check step search and query_scan return the heap
arrays of the CPU oracle on the model's partitions (adc_filter_compose.expected / unfiltered) — never those of another index of
this library.  tests/test_index_model_host.py shows on a CPU that the sequences reach the states they are built for and that no
check is vacuous."""
import numpy as np
import pytest

import adc_filter_compose as fc
import index_model as im
import pyqadc
from helpers import path_independent
from test_gpu_adc_filter import replayed
from test_gpu_adc_remove import check

pytestmark = pytest.mark.gpu

NQ, MA = im.NQ, im.MA
UNCHANGED = ("refill_in_place", "remove", "remove_device", "empty_partition", "empty_index", "remove_nothing", "remove_found", "reserve_less")


class FilterBank:
    """the AdcFilter objects of a walk by the order of their set_filter steps; two walks that share a bank share the objects: their
    steps ask for the same key sets (index_model.with_keys_of)"""

    def __init__(self):
        self.made = {}

    def get(self, ordinal, mode, keys):
        if ordinal not in self.made:
            f = pyqadc.AdcFilter(keys, mode)
            self.made[ordinal] = (f, mode, keys, f.info())
        f, made_mode, made_keys, info = self.made[ordinal]
        assert made_mode == mode and np.array_equal(made_keys, keys)
        return f, made_keys, info

    def close(self):
        for f, _, _, _ in self.made.values():
            f.close()
        self.made = {}


class AdcWalk:
    """one index, its model and the steps of its sequence"""

    def __init__(self, po, shape, seed, bank):
        import torch
        self.po, self.shape, self.bank = po, shape, bank
        nsq, bits, dim = shape
        self.opq = shape in im.ADC_OPQ
        q = self.q = im.quantizers(shape)
        assign, codes = q.encoded(self.opq)                                      # the stateless encoders, on the GPU
        assert np.array_equal(assign, im.host_assign(po, shape))                 # what the CPU test generated its sequences from
        self.steps = im.steps(seed, im.Profile("adc", assign, "fresh", shape))
        self.model = im.Model(assign, codes)
        self.queries = im.queries(q)
        self.tq = torch.from_numpy(self.queries).to("cuda:0")
        self.tv = torch.from_numpy(q.vectors).to("cuda:0")
        self.idx = q.index(self.opq)
        self.filter, self.keys, self.mode, self.info, self.ordinal = None, None, None, None, 0
        self.found = None
        self.finish = 0
        self.deep = self.checks = 0
        self.at = 0

    def close(self):
        self.idx.close()

    def done(self):
        return self.at == len(self.steps)

    def step(self):
        st = self.steps[self.at]
        self.what = "step %d (%s) of %dx%d" % (self.at, st["op"], self.shape[0], self.shape[1])
        self.at += 1
        self.run(st)

    def run(self, st):
        import torch
        op, idx, model, what = st["op"], self.idx, self.model, self.what
        moved = idx.relocations()
        if op == "check":
            self.check(st.get("deep", False))
            return
        if op == "set_finish":
            idx.set_finish(st["mode"])
            self.finish = st["mode"]
            return
        if op == "set_filter":
            self.mode = st["mode"]
            if self.mode is None:
                self.filter = self.keys = self.info = None
            else:
                self.filter, self.keys, self.info = self.bank.get(self.ordinal, st["mode"], st["keys"])
                self.ordinal += 1
            idx.set_filter(self.filter)
            return
        assert op in im.MUTATIONS, op
        if op in ("add", "refill_in_place", "overflow"):
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
            keys, _, sizes = idx.search_device(self.tq, MA, 100)                 # "remove what this search returned"
            assert int(sizes.min().item()) == 100
            flat = keys.reshape(-1)
            self.found = flat.cpu().numpy().view(np.uint32)
            gone = model.remove(self.found)
            assert gone >= 100                                                   # a heap holds distinct rows
            assert idx.remove_labels_device(flat) == gone, what
        elif op in ("reserve_more", "reserve_less"):
            idx.reserve(st["capacities"])
        elif op == "add_partitions":
            codes, labels = im.extra_partition(self.shape, st["seed"], st["labels"])
            idx.add_partitions([codes], [labels])
            idx.set_coarse(im.coarse_of(self.q, im.K + 1))                       # the new partition's centroid: no pool vector is nearest to it
        gone = im.apply(model, st, self.shape)
        assert gone is None or gone == st["gone"], what
        check(idx, model.parts, what)
        if op in UNCHANGED or st.get("fits") is True:
            assert idx.relocations() == moved, what
        if op == "overflow" or st.get("fits") == "moves":
            assert idx.relocations() > moved, what
        if self.filter is not None:                                              # the filter stays set, and as it is
            assert self.filter.info() == self.info, what

    def heaps(self, assign, tables, R):
        po, model, shape = self.po, self.model, self.shape[:2]
        out = []
        for i in range(NQ):
            parts, labels = [model.parts[k][0] for k in assign[i]], [model.parts[k][1] for k in assign[i]]
            if self.mode is None:
                out.append(fc.unfiltered(po, shape, parts, labels, tables[i], R))
            else:
                out.append(fc.expected(po, shape, parts, labels, tables[i], R, self.keys, self.mode))
        return out

    def check(self, deep):
        idx, what = self.idx, self.what
        assign, tables = idx.search_tables(self.queries, MA)
        for R in (1, 100):
            want = self.heaps(assign, tables, R)
            got = idx.search(self.queries, MA, R)
            scan = idx.query_scan(assign, tables, R)
            assert np.array_equal(got[3], assign), what
            for i in range(NQ):
                fc.assert_heap(got[:3], want[i], i, "%s: search R=%d" % (what, R))
                fc.assert_heap(scan, want[i], i, "%s: query_scan R=%d" % (what, R))
                if self.found is not None:
                    assert not np.isin(got[0][i, :got[2][i]], self.found).any(), "%s: a removed key is in a heap" % what
            if deep and R == 100:
                idx.set_finish(0)                                                # (the candidate stream is the host finish's input)
                dk, dv, ds = idx.search_device(self.tq, MA, R)
                dev = (dk.cpu().numpy().view(np.uint32), dv.cpu().numpy(), ds.cpu().numpy())
                keys, vals, offsets = idx.query_scan_candidates(assign, tables, R)
                stream = replayed(self.po, keys, vals, offsets, NQ, R)
                for i in range(NQ):
                    fc.assert_heap(dev, want[i], i, "%s: search_device" % what)
                    fc.assert_heap(stream, want[i], i, "%s: the replayed stream" % what)
                idx.set_finish(self.finish)
                self.deep += 1
        self.checks += 1


def finished(walk):
    assert walk.done() and walk.deep == 1 and walk.found is not None and walk.checks >= 10


@path_independent
@pytest.mark.parametrize("case", im.ADC_CASES, ids=im.case_id)
def test_a_whole_life_equals_the_model_and_the_oracle(po, case):
    shape, seed = case
    bank = FilterBank()
    walk = AdcWalk(po, shape, seed, bank)
    try:
        while not walk.done():
            walk.step()
        finished(walk)
    finally:
        walk.close()
        bank.close()


@path_independent
def test_two_indexes_in_alternation(po):
    """an 8x8 and a 2x16 index live their sequences step by step in turn, in one thread, and share every AdcFilter: the pinned staging,
    the streams and whatever else the process holds once serve both"""
    bank = FilterBank()
    walks = [AdcWalk(po, (8, 8, 64), 1, bank), AdcWalk(po, (2, 16, 16), 1, bank)]
    # (tests/test_index_model_host.py: the second walk's checks are not vacuous under the first one's key sets either)
    walks[1].steps = im.with_keys_of(walks[1].steps, walks[0].steps)
    try:
        while not all(w.done() for w in walks):
            for w in walks:
                if not w.done():
                    w.step()
        for w in walks:
            finished(w)
    finally:
        for w in walks:
            w.close()
        bank.close()
