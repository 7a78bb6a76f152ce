"""The model and the sequences of the lifecycle tests (tests/index_model.py), on a CPU: for every (seed, profile) that
tests/test_gpu_adc_lifecycle.py and tests/test_gpu_index_lifecycle.py walk,
  * the coverage conditions hold — the states a sequence is built to reach are reached;
  * the generator is deterministic;
  * the model's steps give what a brute-force recomputation gives: the surviving (vector, label) pairs in insertion order, grouped
    stably by assignment;
  * no check that follows a removal or a filter change is vacuous: the removed or dropped rows intersect the R = 100 heaps the
    oracle gives on the model as it stood before the step, so a row that stayed behind, or a filter that was not applied, would
    change a heap.  The heaps come from adc_filter_compose.unfiltered / expected on random tables for a fixed query set, the probes
    from the oracle's coarse assignment of index_model.queries;
  * the 4-bit walks once more under the probes, tables and keep values their GPU test queries with (index_model.index4_inputs,
    index4_keep), through the oracle's scanner_4 (po.query_scan): every query of every check on an index that holds rows is
    answered (rc 0: the pre-scanned starts fill a heap of 100, so the GPU test has heaps to compare), and the removed rows were in
    those heaps;
  * the second walk of test_two_indexes_in_alternation under the first walk's key sets, which it shares."""
import numpy as np
import pytest

import adc_compose as ac
import adc_filter_compose as fc
import index_model as im

R = 100
CASES = [("adc",) + c for c in im.ADC_CASES] + [("index4",) + c for c in im.INDEX4_CASES] + [("index4_short",) + c for c in im.INDEX4_SHORT_CASES]


def case_id(c):
    return c[0] + "-" + im.case_id(c[1:])


def profile_of(po, case):
    kind, shape = case[0], case[1]
    start, seed = ("fresh", case[2]) if kind == "adc" else case[2:]
    nsq, bits, dim = shape
    assign, codes = im.host_pool(po, shape, kind == "adc" and shape in im.ADC_OPQ)
    return im.Profile(kind, assign, start, shape), seed, assign, codes


_sequences = {}


def sequence(po, case):
    if case not in _sequences:
        pf, seed, assign, codes = profile_of(po, case)
        _sequences[case] = (pf, im.steps(seed, pf), assign, codes)
    return _sequences[case]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_coverage_conditions_hold(po, case):
    pf, seq, _, _ = sequence(po, case)
    got = im.coverage(seq, pf)
    for name in im.required(pf):
        assert got[name], name
    assert seq[-1]["op"] == "check" and seq[-2]["op"] == "remove_found"
    assert all(st["op"] in im.MUTATIONS + ("check", "set_filter", "set_finish") for st in seq)
    offsets = [st["labels_offset"] for st in seq if "labels_offset" in st]
    assert len(set(offsets)) == len(offsets), "a labels_offset is used twice"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_generator_is_deterministic(po, case):
    pf, seq, _, _ = sequence(po, case)
    again = im.steps(profile_of(po, case)[1], pf)
    assert im.same_steps(seq, again)
    assert not im.same_steps(seq, im.steps(profile_of(po, case)[1] + 17, pf)), "the seed does not reach the sequence"


def probes_and_tables(po, case, partitions):
    """assign [NQ][MA] of the fixed queries on the coarse centroids the index has with that many partitions, and random tables"""
    shape = case[1]
    q = im.quantizers(shape)
    assign = ac.assign(po, im.queries(q), im.coarse_of(q, partitions), im.MA)
    tables = fc.rand_tables(np.random.default_rng(99), (shape[0], shape[1]), im.NQ, im.MA)
    return assign, tables


def heap_keys(po, case, model, mode=None, keys=None):
    """the keys of the R = 100 heaps of every query on the model, under the filter"""
    shape = (case[1][0], case[1][1])
    assign, tables = probes_and_tables(po, case, len(model.parts))
    out = []
    for i in range(im.NQ):
        parts, labels = [model.parts[k][0] for k in assign[i]], [model.parts[k][1] for k in assign[i]]
        if mode is None:
            out.append(fc.unfiltered(po, shape, parts, labels, tables[i], R)[0])
        else:
            out.append(fc.expected(po, shape, parts, labels, tables[i], R, keys, mode)[0])
    return np.concatenate(out)


def float_heaps(po, case):
    return lambda model, mode, keys, ordinal: heap_keys(po, case, model, mode, keys)


def scanner4_heaps(po, case):
    """the keys of the R = 100 heaps of po.query_scan under the GPU test's own probes, tables and keep; every query is answered"""
    shape, _, seed = case[1:]
    assign, tables = im.index4_inputs(shape, seed)

    def heaps(model, mode, keys, ordinal):
        assert mode is None
        if sum(model.sizes()) == 0:
            return np.zeros(0, np.uint32)
        keep = im.index4_keep(model.sizes(), assign, ordinal)
        used.add(keep)
        out = []
        for i in range(im.NQ):
            want = po.query_scan(shape[0], [c for c, _ in model.parts], [l for _, l in model.parts], keep, assign[i], tables[i].copy(), R)
            assert want["rc"] == 0 and len(want["keys"]) == R, "query %d of check %d is not answered at keep %g" % (i, ordinal, keep)
            out.append(want["keys"])
        return np.concatenate(out)

    used = set()
    heaps.used = used
    return heaps


def walk(po, case, seq, heaps):
    """the model through the sequence; at every check, what the removals and filter changes since the last one took from the heaps
    (heaps(model, mode, keys, number of the next check) -> keys) must be more than nothing.  -> (model, the keys of remove_found)"""
    pf, _, assign, codes = sequence(po, case)
    shape = case[1]
    model = im.Model(assign, codes)
    mode, keys = None, None
    pending = []                                                                 # what the next check has to notice
    found = None
    checks = noticed = 0
    for st in seq:
        op = st["op"]
        if op in ("remove", "remove_device", "empty_partition", "empty_index"):
            hit = np.isin(heaps(model, mode, keys, checks), st["labels"]).sum()
            assert im.apply(model, st, shape) == st["gone"]
            pending.append((op, hit))
        elif op == "remove_found":
            found = heap_keys(po, case, model, mode, keys)                       # (a float-ADC search: the view's, on a 4-bit index)
            pending.append((op, np.isin(heaps(model, mode, keys, checks), found).sum()))
            assert model.remove(found) >= R
        elif op == "set_filter":
            plain = heaps(model, None, None, checks)
            if st["mode"] is not None:
                pending.append(("set_filter " + st["mode"], fc.dropped(plain, st["keys"], st["mode"]).sum()))
            elif mode is not None:                                               # the rows that come back
                pending.append(("set_filter None", fc.dropped(plain, keys, mode).sum()))
            mode, keys = st["mode"], st["keys"]
        elif op == "check":
            if sum(model.sizes()):
                heaps(model, mode, keys, checks)                                 # (the 4-bit form asserts that every query is answered)
            for what, hit in pending:
                assert hit > 0, "check %d, after %s, is vacuous: no removed or dropped row was in a heap" % (checks, what)
            noticed += len(pending) > 0
            pending = []
            checks += 1
        else:
            im.apply(model, st, shape)
    assert not pending and noticed >= (2 if pf.short else 5)
    return model, found


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_model_equals_a_brute_force_recomputation_and_no_check_is_vacuous(po, case):
    pf, seq, assign, codes = sequence(po, case)
    model, found = walk(po, case, seq, float_heaps(po, case))
    want = im.brute_force(seq, assign, codes, found, case[1])
    assert len(want) == len(model.parts)
    for (gc, gl), (wc, wl) in zip(model.parts, want):
        assert gc.dtype == wc.dtype and np.array_equal(gc, wc) and np.array_equal(gl, wl)
    if not pf.short:
        assert max(model.sizes()[:im.K]) > im.REMOVE_TILE - R * im.NQ


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "adc"], ids=case_id)
def test_no_check_of_a_4_bit_walk_is_vacuous_under_its_own_probes_tables_and_keep(po, case):
    pf, seq, _, _ = sequence(po, case)
    heaps = scanner4_heaps(po, case)
    walk(po, case, seq, heaps)
    assert pf.short or heaps.used == set(im.KEEPS), "a keep value is never used"


def test_the_second_walk_of_the_alternation_under_the_keys_of_the_first(po):
    """test_two_indexes_in_alternation: the 2x16 index takes the AdcFilter objects, so the key sets, of the 8x8 index"""
    first, second = ("adc", (8, 8, 64), 1), ("adc", (2, 16, 16), 1)
    seq = im.with_keys_of(sequence(po, second)[1], sequence(po, first)[1])
    assert not im.same_steps(seq, sequence(po, second)[1])
    walk(po, second, seq, float_heaps(po, second))
