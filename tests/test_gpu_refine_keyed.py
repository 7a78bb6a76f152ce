"""GPU: the keyed refine store (pyqadc.Refine(keyed=True) over qadc_refine_create_keyed, _put, _remove, _rerank; DESIGN.md section
11.14) against its host twin (refine::keyed_store of quick-adc_amd/host/refine.hpp through tests/cpp/refine_keyed_host.cpp).  A
life of a store is a script of put, remove and rerank (tests/refine_keyed_cases.py); every operation's result — keys held, keys
removed, the re-ranked keys, the distances' bit patterns, sizes, the missing count — is compared for equality.  There is no
tolerance anywhere: the hash table's layout may not show in a result.

The scripts aim at what only the device structure can get wrong: probe chains longer than a wave that all start in one slot or
wrap around the table's end, dead slots inside a chain, claims of one slot by a whole workgroup and across workgroups and passes,
rows that come back from the free list, and rebuilds and relocations in the middle of a life."""
import numpy as np
import pytest

import refine_cases as rc
import refine_keyed_cases as kc
from helpers import path_independent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def twin():
    return kc.build_driver()


def fmix32(k):
    k = np.asarray(k, np.uint64)
    m = np.uint64(0xFFFFFFFF)
    k = k ^ (k >> np.uint64(16))
    k = (k * np.uint64(0x85EBCA6B)) & m
    k = k ^ (k >> np.uint64(13))
    k = (k * np.uint64(0xC2B2AE35)) & m
    return k ^ (k >> np.uint64(16))


def keys_with_home(pyqadc, bits, home, n, start=0):
    """the first n keys from `start` on whose home slot in a table of 2^bits slots is `home`: found with numpy, then confirmed
    with the library's own hash"""
    found = []
    while len(found) < n:
        k = np.arange(start, start + (1 << 22), dtype=np.uint64)
        found += k[(fmix32(k) >> np.uint64(32 - bits)) == home].tolist()
        start += 1 << 22
    found = np.array(found[:n], np.uint32)
    assert all(pyqadc.refine_keyed_slot(int(k), bits) == home for k in found)
    return found


def bits_of(st):
    slots = st.keyed_info()["table_slots"]
    assert slots & (slots - 1) == 0
    return slots.bit_length() - 1


def distinct(rng, n, bits=32):
    """n different keys below 2^bits (never the filler key 0xFFFFFFFF), in a random order"""
    k = np.unique(rng.integers(0, min(1 << bits, 0xFFFFFFFF), 2 * n + 16, dtype=np.uint64).astype(np.uint32))
    assert len(k) >= n
    return rng.permutation(k)[:n]


class Life:
    """a store and the script it has run so far: step(ops) runs more operations on the store, the whole script on the twin, and
    compares the new operations' results"""

    def __init__(self, pyqadc, twin, tmp_path, dim, dtype, device=False):
        self.pyqadc, self.twin, self.tmp_path, self.dim, self.dtype, self.device = pyqadc, twin, tmp_path, dim, dtype, device
        self.st = pyqadc.Refine(dim, dtype, keyed=True)
        self.script = []

    def step(self, ops):
        got = kc.run_store(self.pyqadc, self.st, ops, self.device)
        self.script += ops
        kc.assert_same(got, kc.run_twin(self.twin, self.tmp_path, self.dim, self.dtype, self.script)[-len(ops):], "step ending at operation %d" % len(self.script))
        return got


def run(pyqadc, twin, tmp_path, dim, dtype, script, device=False, st=None):
    """the script on a store (a new one unless given) and on the twin, compared; -> the store"""
    st = pyqadc.Refine(dim, dtype, keyed=True) if st is None else st
    got = kc.run_store(pyqadc, st, script, device)
    kc.assert_same(got, kc.run_twin(twin, tmp_path, dim, dtype, script), "device forms" if device else "host forms")
    return st


# ---- probe chains ------------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("how", ["one_call", "many_calls"])
def test_probe_chains_longer_than_a_wave(pyqadc, twin, tmp_path, how):
    dim = 8
    rng = np.random.default_rng(41)
    st = pyqadc.Refine(dim, "f32", keyed=True)
    st.reserve(4096)                                                             # the table keeps its size through the test
    bits = bits_of(st)
    assert bits == 13
    slots = 1 << bits
    group = keys_with_home(pyqadc, bits, 1234, 320)                              # one home slot: a chain of 300, and 20 that stay absent
    wrap = keys_with_home(pyqadc, bits, slots - 1, 320, start=1 << 30)           # a chain that starts in the last slot and wraps
    near = np.concatenate([keys_with_home(pyqadc, bits, h, 3, start=1 << 29) for h in (1233, 1235, 1300, 1533, 0, 5, 299)])   # inside the chains' slots
    live = np.concatenate([group[:300], wrap[:300], near[::3]])
    absent = np.concatenate([group[300:], wrap[300:], near[1::3]])
    v = lambda n: rng.normal(size=(n, dim)).astype(np.float32)
    look = lambda: kc.all_keys_rerank(rng, dim, live, absent)
    order = rng.permutation(len(live))
    if how == "one_call":                                                        # the claims of a chain contend
        script = [kc.put(live[order], v(len(live)))]
    else:
        script = [kc.put(live[order[i:i + 7]], v(len(order[i:i + 7]))) for i in range(0, len(live), 7)]
    script += look()
    gone = np.concatenate([group[:300:2], wrap[:300:2]])                         # every other key of each chain: dead slots inside them
    script += [kc.remove(gone)] + look()
    script += [kc.put(near[1::3], v(len(near[1::3])))] + look()                  # new keys probe past the dead slots
    script += [kc.put(gone[::-1], v(len(gone)))] + look()                        # the removed keys again, with new vectors: their slots revive
    run(pyqadc, twin, tmp_path, dim, "f32", script, st=st)
    info = st.keyed_info()
    assert info["table_slots"] == slots and st.relocations() == 0 and info["live"] == len(live) + len(near[1::3])
    assert info["table_used"] == info["live"] and info["rows_free"] == 0         # every dead slot was revived, every freed row reused
    st.close()


# ---- duplicates in one put ---------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_last_of_equal_keys_in_one_put_wins(pyqadc, twin, tmp_path, dtype):
    dim = 4
    rng = np.random.default_rng(42)
    v = lambda n: rng.normal(size=(n, dim)).astype(np.float32)
    once = np.full(1000, 77, np.uint32)                                          # one key 1000 times: four workgroups on one slot
    labels = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    labels[labels == 0xFFFFFFFF] = 1
    labels[255] = labels[256] = 4242                                             # across a workgroup boundary (256 inputs each)
    labels[10] = labels[700] = 4243                                              # ... and far apart
    labels[63] = labels[64] = 4244                                               # across a wave boundary
    every = np.unique(np.concatenate([once, labels]))
    script = [kc.put(once, v(1000))] + kc.all_keys_rerank(rng, dim, every) + [kc.put(labels, v(1000))] + kc.all_keys_rerank(rng, dim, every)
    script += [kc.put(np.concatenate([labels[:300], once[:300]]), v(600))] + kc.all_keys_rerank(rng, dim, every)   # overwrites, again with repeats
    st = run(pyqadc, twin, tmp_path, dim, dtype, script)
    assert st.keyed_info()["live"] == len(every)
    st.close()


@path_independent
def test_equal_keys_on_either_side_of_a_pass(pyqadc, twin, tmp_path):
    """dim 4096 has the smallest pass, 4096 inputs (host/refine_keyed_plan.hpp): the key of the first pass's last input comes again
    as the second pass's first, and one of its early keys as the call's last"""
    dim, n = 4096, 4096 + 4
    rng = np.random.default_rng(43)
    labels = distinct(rng, n)
    labels[4096] = labels[4095]
    labels[n - 1] = labels[5]
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    script = [kc.put(labels, vec)] + kc.all_keys_rerank(rng, dim, labels, extra=[3], nq=1)
    want = kc.run_twin(twin, tmp_path, dim, "f16", script)
    for device in (False, True):
        st = pyqadc.Refine(dim, "f16", keyed=True)
        kc.assert_same(kc.run_store(pyqadc, st, script, device), want, "device forms" if device else "host forms")
        assert st.keyed_info()["live"] == n - 2
        st.close()


# ---- rows: overwrite allocates nothing, free rows come back, reserve ----------------------------------------------------------

@path_independent
def test_an_overwrite_allocates_nothing_and_free_rows_come_back(pyqadc, twin, tmp_path):
    dim = 24
    rng = np.random.default_rng(44)
    v = lambda n: rng.normal(size=(n, dim)).astype(np.float32)
    keys = distinct(rng, 3000)
    first, other = keys[:2000], keys[2000:]
    look = lambda: kc.all_keys_rerank(rng, dim, keys)
    life = Life(pyqadc, twin, tmp_path, dim, "f32")
    st = life.st
    life.step([kc.put(first, v(2000))])
    before, moved = st.keyed_info(), st.relocations()
    assert before["live"] == before["rows_allocated"] == 2000 and before["rows_free"] == 0 and st.info()["rows"] == 2000 and st.info()["lo"] == 0
    life.step([kc.put(first, v(2000)), kc.put(rng.permutation(first)[:1500], v(1500))] + look())   # keys that are all held
    assert st.keyed_info() == before and st.relocations() == moved               # nothing is allocated, nothing moves, no slot is claimed
    m = 700                                                                      # m keys leave, m other keys come: the freed rows serve them
    (gone,) = life.step([kc.remove(first[:m])])
    life.step(look())
    mid = st.keyed_info()
    assert gone["removed"] == m and mid["live"] == 2000 - m and mid["rows_free"] == m and mid["rows_allocated"] == 2000 and mid["table_used"] == 2000
    life.step([kc.put(other[:m], v(m))] + look())
    after = st.keyed_info()
    assert after["rows_allocated"] == 2000 and after["rows_free"] == 0 and after["live"] == 2000 and st.relocations() == moved
    st.close()


@path_independent
def test_reserve_makes_room_in_the_rows_and_in_the_table(pyqadc, twin, tmp_path):
    dim, n = 8, 5000
    rng = np.random.default_rng(45)
    keys = distinct(rng, n)
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    st = pyqadc.Refine(dim, "f16", keyed=True)
    st.reserve(n)
    before = st.keyed_info()
    assert before["table_slots"] >= 2 * n and before["live"] == 0
    script = [kc.put(keys[a:b], vec[a:b]) for a, b in ((0, 1), (1, 1000), (1000, 4999), (4999, 5000))] + kc.all_keys_rerank(rng, dim, keys, extra=[0xFFFFFFFF])
    run(pyqadc, twin, tmp_path, dim, "f16", script, st=st)
    after = st.keyed_info()
    assert st.relocations() == 0 and after["table_slots"] == before["table_slots"] and after["bytes"] == before["bytes"] and after["live"] == n
    st.close()


# ---- growth and rebuild ------------------------------------------------------------------------------------------------------

@path_independent
def test_a_store_grown_from_nothing_through_rebuilds_and_relocations(pyqadc, twin, tmp_path):
    dim = 16
    rng = np.random.default_rng(46)
    pool = distinct(rng, 6000) | np.uint32(1)                                    # odd keys: the even ones below stay absent
    pool = pool[np.sort(np.unique(pool, return_index=True)[1])]
    pool = pool[pool != 0xFFFFFFFF]
    st = pyqadc.Refine(dim, "f32", keyed=True)
    script, ever, held, at = [], np.zeros(0, np.uint32), set(), 0
    for step in range(36):
        n = int(rng.integers(1, 260))
        new = pool[at:at + n]
        at += n
        again = rng.choice(ever, min(len(ever), n // 3), replace=False) if len(ever) else np.zeros(0, np.uint32)   # overwrites and re-puts among them
        labels = rng.permutation(np.concatenate([new, again]))
        script.append(kc.put(labels, rng.normal(size=(len(labels), dim)).astype(np.float32)))
        ever = np.unique(np.concatenate([ever, labels]))
        held |= set(labels.tolist())
        script += kc.all_keys_rerank(rng, dim, ever, extra=[0, 2, 4], nq=1)
        if step % 3 == 1:                                                        # removes in between: dead slots are there when a rebuild comes
            gone = rng.choice(ever, len(ever) // 4, replace=False)
            script.append(kc.remove(np.concatenate([gone, gone[:5], np.array([6, 8], np.uint32)])))
            held -= set(gone.tolist())
            script += kc.all_keys_rerank(rng, dim, ever, extra=[0, 2, 4], nq=1)
    want = kc.run_twin(twin, tmp_path, dim, "f32", script)
    rebuilds, dropped, last = 0, 0, st.keyed_info()
    for i, op in enumerate(script):                                              # operation by operation, the store's state looked at in between
        (got,) = kc.run_store(pyqadc, st, [op])
        diff = kc.differs(got, want[i])
        assert diff is None, "operation %d (%s): %s" % (i, op[0], diff)
        info = st.keyed_info()
        assert info["table_used"] * 2 <= info["table_slots"] and info["live"] <= info["table_used"], info
        assert info["live"] + info["rows_free"] == info["rows_allocated"], info
        if op[0] == "put" and (info["table_slots"] != last["table_slots"] or info["table_used"] < last["table_used"]):
            rebuilds += 1
            dropped += last["table_used"] - last["live"]
            assert info["table_used"] == info["live"], "dead slots survived a rebuild: %s" % (info,)
        last = info
    assert rebuilds >= 3 and dropped > 0 and st.relocations() >= 3, (rebuilds, dropped, st.relocations())
    assert last["live"] == len(held)
    st.close()


# ---- edge keys ---------------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_edge_keys_and_the_refused_filler_key(pyqadc, twin, tmp_path, device):
    dim = 5
    rng = np.random.default_rng(47)
    v = lambda n: rng.normal(size=(n, dim)).astype(np.float32)
    every = np.array([0, 1, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF, 1 << 31], np.uint32)
    probe = kc.all_keys_rerank(rng, dim, every)                                  # one list of operations, run three times
    life = Life(pyqadc, twin, tmp_path, dim, "f32", device)
    st = life.st
    life.step(probe + [kc.put(np.array([0, 0xFFFFFFFE, 1 << 31], np.uint32), v(3))])
    first = life.step(probe)
    before = st.keyed_info()
    got = life.step([kc.put(np.array([9, 0xFFFFFFFF, 0], np.uint32), v(3)), kc.put(np.array([0xFFFFFFFF], np.uint32), v(1))] + probe)
    assert [g["ok"] for g in got[:2]] == [0, 0]                                  # refused, in the host and in the device form
    assert st.keyed_info() == before                                             # ... with the store exactly as it was
    kc.assert_same(got[2:], first)
    assert got[2]["sizes"].tolist() == [3, 3] and got[2]["missing"] == 6
    (gone,) = life.step([kc.remove(np.array([0xFFFFFFFF, 0, 0], np.uint32))])
    assert gone["removed"] == 1 and st.keyed_info()["live"] == 2
    life.step(probe)
    st.close()


# ---- the rerank kernel's edges through the keyed lookup ------------------------------------------------------------------------

# (r_in, nq, dim, rows): the sort sizes' edges, one workgroup per query and many, the shortest and the longest rows
EDGES = [(1, 257, 65, 300), (65, 257, 1, 1000), (513, 3, 65, 700), (513, 257, 1, 700), (8192, 3, 65, 20000), (8192, 1, 4096, 1024)]


@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("r_in,nq,dim,rows", EDGES, ids=["rin%d-nq%d-dim%d" % e[:3] for e in EDGES])
def test_rerank_kernel_edges_through_the_keyed_lookup(pyqadc, twin, tmp_path, r_in, nq, dim, rows, dtype):
    rng = np.random.default_rng(r_in * 1000 + nq + dim)
    drawn = np.unique(rng.integers(0, 0xFFFFFFFF, 2 * rows + 64, dtype=np.uint64).astype(np.uint32))   # sparse over all 32 bits
    drawn = rng.permutation(drawn)
    labels, absent = drawn[:rows], drawn[rows:]
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    keys = labels[rng.integers(0, rows, (nq, r_in))]
    if rows >= r_in:
        keys[0::2] = labels[rng.random((len(keys[0::2]), rows)).argsort(1)[:, :r_in]]      # even queries: distinct keys
    miss = rng.random((nq, r_in)) < 0.1                                                    # a tenth of the candidates: keys not held
    keys[miss] = absent[rng.integers(0, len(absent), int(miss.sum()))]
    values = rng.random((nq, r_in)).astype(np.float32)
    values[rng.random((nq, r_in)) < 0.05] = rc.FLT_MAX
    counts = rng.integers(0, r_in + 1, nq).astype(np.int32)
    counts[0::3] = r_in
    script = [kc.put(labels, vec)]
    script += [kc.rerank(q, keys, R) for R in (max(r_in // 2, 1), r_in, r_in + 5)]
    script += [kc.rerank(q, keys, r_in, counts=counts, values=values)]
    st = pyqadc.Refine(dim, dtype, keyed=True)
    got = kc.run_store(pyqadc, st, script)
    want = kc.run_twin(twin, tmp_path, dim, dtype, script)
    kc.assert_same(got, want, "r_in %d nq %d dim %d %s" % (r_in, nq, dim, dtype))
    assert want[2]["missing"] == int(miss.sum()) > 0 or r_in == 1
    st.close()


# ---- device forms and mode errors --------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_device_forms_equal_the_host_forms(pyqadc, twin, tmp_path, dtype):
    dim = 33
    rng = np.random.default_rng(48)
    v = lambda n: rng.normal(size=(n, dim)).astype(np.float32)
    keys = distinct(rng, 2500)
    keys = keys[keys > 2]
    look = lambda: kc.all_keys_rerank(rng, dim, keys, extra=[1, 2])
    script = [kc.put(keys[:1500], v(1500))] + look() + [kc.remove(np.concatenate([keys[:400], keys[:7], keys[2000:2010]]))] + look()
    script += [kc.put(np.concatenate([keys[1000:], keys[200:300]]), v(1600))] + look()
    r_in = 40
    cand = keys[rng.integers(0, len(keys), (6, r_in))]
    values = rng.random((6, r_in)).astype(np.float32)
    values[:, ::7] = rc.FLT_MAX
    script += [kc.rerank(v(6), cand, 10, counts=np.array([0, 1, 39, 40, 17, 40], np.int32), values=values)]
    host = pyqadc.Refine(dim, dtype, keyed=True)
    dev = pyqadc.Refine(dim, dtype, keyed=True)
    a, b = kc.run_store(pyqadc, host, script), kc.run_store(pyqadc, dev, script, device=True)
    kc.assert_same(b, a, "device forms against host forms")
    kc.assert_same(a, kc.run_twin(twin, tmp_path, dim, dtype, script))
    assert host.keyed_info() == dev.keyed_info()
    host.close()
    dev.close()


@path_independent
def test_the_two_kinds_of_store_do_not_mix(pyqadc):
    import torch
    dim = 4
    v = np.ones((3, dim), np.float32)
    lab = np.array([1, 2, 3], np.uint32)
    tv, tl = torch.from_numpy(v).cuda(), torch.from_numpy(lab.view(np.int32)).cuda()
    dense, keyed = pyqadc.Refine(dim), pyqadc.Refine(dim, keyed=True)
    state = "qadc error -4:"                                                     # QADC_E_STATE
    for call in (lambda: dense.put(v, lab), lambda: dense.put_device(tv, tl), lambda: dense.remove(lab), lambda: dense.remove_device(tl),
                 dense.keyed_info, lambda: keyed.add(v, 0), lambda: keyed.add_device(tv, 0)):
        with pytest.raises(pyqadc.QadcError, match=state):
            call()
    assert dense.info()["rows"] == 0 and keyed.keyed_info()["live"] == 0
    dense.add(v, 10)                                                             # both still work as their kind
    keyed.put(v, lab)
    assert dense.info()["rows"] == 3 and dense.info()["lo"] == 10 and keyed.info()["rows"] == 3 and keyed.info()["lo"] == 0
    assert keyed.rerank(v[:1], lab.reshape(1, 3), 3)[2].tolist() == [3] and dense.rerank(v[:1], np.array([[10, 11, 1]], np.uint32), 3)[3] == 1
    dense.close()
    keyed.close()
