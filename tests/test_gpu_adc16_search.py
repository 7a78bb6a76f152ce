"""The float-ADC engine on 16-bit codes fed with query vectors (AdcIndex.create16: search, search_tables, search_device): coarse
assignment, residual, OPQ rotation and the tables [nsq][65536] of every (query, probe) run on the GPU.  Assign and tables are
compared bit for bit with the composition of the oracle's functions (tests/adc_compose.py's steps with 65536-row codebooks), the
heaps with tests/adc16_compose.py on those tables."""
import numpy as np
import pytest

import adc16_compose as a16
import adc_compose as ac
import pyqadc
from adc16_compose import assert_heap, tables_direct, tables_expansion
from helpers import path_independent

pytestmark = pytest.mark.gpu

DIM = 16           # nsq 2: sub-vectors of 8 (the table kernel's register path); nsq 8: of 2 (its any-size path)
NQ, MA = 5, 3


class Case:
    """One database (flat: one partition; IVF: K = 8 labelled partitions of skewed sizes, one empty), its quantizers, its GPU index"""

    def __init__(self, nsq, ivf, opq):
        rng = np.random.default_rng(16000 + 100 * nsq + 10 * ivf + opq)
        self.nsq, self.K = nsq, 8 if ivf else 0
        self.codebooks = rng.standard_normal((nsq, 65536, DIM // nsq), dtype=np.float32)
        self.rotation = ac.random_rotation(rng, DIM) if opq else None
        if ivf:
            self.coarse = (rng.normal(size=(8, DIM)) * 2).astype(np.float32)
            sizes = [7000, 0, 3100, 1, 5000, 17, 2500, 1382]
            perm = rng.permutation(sum(sizes)).astype(np.uint32)
            self.parts = [rng.integers(0, 65536, (s, nsq)).astype(np.uint16) for s in sizes]
            self.labels = list(np.split(perm, np.cumsum(sizes)[:-1]))
        else:
            self.coarse = None
            self.parts, self.labels = [rng.integers(0, 65536, (9001, nsq)).astype(np.uint16)], None
        self.idx = pyqadc.AdcIndex.create16(nsq)
        self.idx.add_partitions(self.parts, self.labels)
        self.idx.set_pq(self.codebooks)
        self.idx.set_rotation(self.rotation)
        self.idx.set_coarse(self.coarse)
        self.queries = rng.normal(size=(NQ, DIM)).astype(np.float32)
        if ivf:
            self.queries += self.coarse[rng.integers(0, 8, NQ)]
        self.composed = {}

    def compose(self, po, table_form, sum_mode=1):
        """-> (assign [NQ][MA], tables [NQ][MA][nsq*65536]), computed once per (form actually used, sum mode)"""
        expansion = ac.expansion_used(table_form, MA)
        if (expansion, sum_mode) not in self.composed:
            a = ac.assign(po, self.queries, self.coarse, MA, sum_mode)
            res = ac.residuals(self.queries, self.coarse, a, self.rotation).reshape(NQ * MA, DIM)
            f = tables_expansion if expansion else tables_direct
            self.composed[expansion, sum_mode] = (a, f(po, self.codebooks, res, sum_mode).reshape(NQ, MA, -1))
        return self.composed[expansion, sum_mode]

    def heap(self, po, a, tables, q, R, sum_mode=1):
        labels = None if self.labels is None else [self.labels[k] for k in a[q]]
        return a16.heap(po, self.nsq, [self.parts[k] for k in a[q]], labels, tables[q], R, sum_mode)


@pytest.fixture(scope="module", params=[(nsq, ivf, opq) for nsq in (2, 8) for ivf in (0, 1) for opq in (0, 1)],
                ids=lambda p: "%dx16-%s-%s" % (p[0], "ivf" if p[1] else "flat", "opq" if p[2] else "pq"))
def case(request):
    c = Case(*request.param)
    yield c
    c.idx.close()


@path_independent
@pytest.mark.parametrize("table_form,sum_mode", [(0, 1), (1, 1), (2, 1), (0, 0), (1, 0)])
def test_tables_equal_the_composition(po, case, table_form, sum_mode):
    want_a, want_t = case.compose(po, table_form, sum_mode)
    got_a, got_t = case.idx.search_tables(case.queries, MA, table_form, sum_mode)
    assert np.array_equal(got_a, want_a), "assign differs"
    diff = got_t.view(np.uint32) != want_t.view(np.uint32)
    assert not diff.any(), "%d table entries differ, first at %s" % (int(diff.sum()), np.argwhere(diff)[0])


@path_independent
@pytest.mark.parametrize("table_form,sum_mode", [(0, 1), (1, 1), (2, 1), (1, 0)])
def test_search_heaps_equal_the_composition(po, case, table_form, sum_mode):
    want_a, want_t = case.compose(po, table_form, sum_mode)
    for R in (1, 100, 1000):
        keys, vals, sizes, a = case.idx.search(case.queries, MA, R, table_form, sum_mode)
        assert np.array_equal(a, want_a)
        for q in range(NQ):
            assert_heap((keys, vals, sizes), case.heap(po, want_a, want_t, q, R, sum_mode), q, "form %d R %d" % (table_form, R))


@path_independent
def test_search_device_and_the_table_budget(po, case):
    torch = pytest.importorskip("torch")
    R = 100
    want_a, want_t = case.compose(po, 2)
    dq = torch.from_numpy(case.queries).cuda()
    per_query = MA * case.nsq * 65536 * 4
    try:
        for per in (0, 1, 2):                                      # 0: the default budget, the whole batch in one pass
            case.idx.set_table_budget(per * per_query)
            out = case.idx.search_device(dq, MA, R)
            got = (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy())
            host = case.idx.search(case.queries, MA, R)[:3]
            for q in range(NQ):
                want = case.heap(po, want_a, want_t, q, R)
                assert_heap(got, want, q, "device, %d queries per pass" % per)
                assert_heap(host, want, q, "host, %d queries per pass" % per)
        assert case.idx.host_finishes() == 0
    finally:
        case.idx.set_table_budget(0)
