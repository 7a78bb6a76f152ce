"""GPU: the memory behaviour of the refine store's device entry points at the C-ABI, on guard-band arenas
(tests/guard_arena.py): qadc_refine_add_device, _rerank_device, _put_device and _remove_device through raw ctypes calls, stores of
floats and halves, dense and keyed.

W  every byte outside the declared outputs is unchanged (add, put and remove write no caller buffer at all);
R  the results under the two guard poisons are bit-identical and equal the host form on the same data; for the calls that change the
   store, "results" are info / keyed_info and a rerank over every key afterwards;
F  every [nq][R] slot and every d_out_sizes[q] is written: rerank's 0xFFFFFFFF / +inf fillers behind out_sizes[q] are asserted
   under the 0x5A output poison as well as the 0xFF one (which is itself the filler key);
A  every buffer at 4 bytes and nothing coarser, and at 256.

Under P2 the label guards cycle through keys the store holds and the list does not, the count guards hold r_in and the float guards
zeros: one stray read removes, overwrites or admits a row."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = [4, 256]
STORES = [(d, k) for d in ("f32", "f16") for k in (False, True)]
STORE_IDS = ["%s-%s" % (d, "keyed" if k else "dense") for d, k in STORES]
FLT_MAX = np.float32(3.4028234663852886e38)
NO_KEY = 0xFFFFFFFF


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def quiet(labels):
    """the labels none of whose bytes is 0xFF: what a P2 guard may cycle through"""
    labels = np.ascontiguousarray(labels, np.uint32)
    return labels[~(labels[:, None].view(np.uint8) == 0xFF).any(1)]


def state(st, queries, keys):
    """what a store answers: its info and one rerank of `keys` (host form)"""
    k, d, s, m = st.rerank(queries, keys, keys.shape[1])
    out = dict(keys=k, dist=d, sizes=s, missing=np.int64(m), rows=np.int64(st.info()["rows"]))
    if st.keyed:
        ki = st.keyed_info()
        out.update(live=np.int64(ki["live"]), rows_free=np.int64(ki["rows_free"]))
    return out


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_add_device(pyqadc, dtype, align):
    rng = np.random.default_rng(31)
    dim, n, lo = 65, 301, 50
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    queries = rng.normal(size=(2, dim)).astype(np.float32)
    keys = np.tile(np.arange(lo - 2, lo + n + 2, dtype=np.uint32), (2, 1))   # every row, and two missing keys on each side
    ref = pyqadc.Refine(dim, dtype)
    ref.add(vec[:100], lo)
    ref.add(vec[100:])
    want = state(ref, queries, keys)
    ref.close()

    def call(a):
        first = a.place(vec[:100], align, "in", name="d_vectors")
        rest = a.place(vec[100:], align, "in", name="d_vectors (second add)")
        st = pyqadc.Refine(dim, dtype)
        a.snapshot()
        for v, key in ((first, lo), (rest, lo + 100)):                       # the second add relocates the rows of the first
            rc = pyqadc.lib().qadc_refine_add_device(st._h, a.ptr(v), v.shape[0], key)
            assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([])
        got = state(st, queries, keys)
        st.close()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=1 << 20)
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)
    assert want["missing"] == 8 and (want["sizes"] == n).all()


RERANK = [(65, 3, 65, 300), (513, 1, 1, 700)]                                # (r_in, nq, dim, rows)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "counts-values"])
@pytest.mark.parametrize("r_in,nq,dim,rows", RERANK, ids=["rin%d-nq%d-dim%d" % r[:3] for r in RERANK])
@pytest.mark.parametrize("dtype,keyed", STORES, ids=STORE_IDS)
def test_rerank_device(pyqadc, dtype, keyed, r_in, nq, dim, rows, extras, align):
    rng = np.random.default_rng(r_in + 7 * keyed)
    R = r_in + 5
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    labels = (rng.permutation(4 * rows)[:rows].astype(np.uint32) + 16) if keyed else np.arange(rows, dtype=np.uint32) + 16
    st = pyqadc.Refine(dim, dtype, keyed=keyed)
    if keyed:
        st.put(vec, labels)
    else:
        st.add(vec, 16)
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    keys = labels[rng.integers(0, rows, (nq, r_in))]
    keys[0, :3] = (3, NO_KEY, labels[0])                                     # two missing keys; duplicates come with the draw
    counts = values = None
    if extras:
        counts = np.array([r_in, 10, 0][:nq], np.int32) if nq > 1 else np.array([r_in - 3], np.int32)
        values = rng.random((nq, r_in)).astype(np.float32)
        values[0, 5:9] = FLT_MAX                                             # skipped
    held = quiet(labels)

    def call(a):
        q = a.place(queries, align, "in", name="d_queries")
        k = a.place(keys, align, "in", guard=held, name="d_keys")
        c = a.place(counts, align, "in", guard=np.array([r_in], np.int32), name="d_counts") if extras else None
        v = a.place(values, align, "in", name="d_values") if extras else None
        ok = a.place(np.empty((nq, R), np.uint32), align, "out", name="d_out_keys")
        od = a.place(np.empty((nq, R), np.float32), align, "out", name="d_out_dist")
        osz = a.place(np.empty(nq, np.int32), align, "out", name="d_out_sizes")
        missing = C.c_uint64(77)
        a.snapshot()
        rc = pyqadc.lib().qadc_refine_rerank_device(st._h, nq, a.ptr(q), r_in, a.ptr(k), a.ptr(c) if extras else None, a.ptr(v) if extras else None,
                                                    R, a.ptr(ok), a.ptr(od), a.ptr(osz), C.byref(missing))
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([ok, od, osz])
        got = dict(keys=a.host(ok), dist=a.host(od), sizes=a.host(osz), missing=np.int64(missing.value))
        for qi in range(nq):                                                 # F, under this poison: the fillers behind out_sizes[q]
            size = int(got["sizes"][qi])
            assert 0 <= size <= r_in and (got["keys"][qi, size:] == NO_KEY).all() and np.isposinf(got["dist"][qi, size:]).all()
            assert (got["keys"][qi, :size] != NO_KEY).all() and (got["keys"][qi, :size] != 0x5A5A5A5A).all()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    hk, hd, hs, hm = st.rerank(queries, keys, R, counts=counts, values=values)
    host = dict(keys=hk, dist=hd, sizes=hs, missing=np.int64(hm))
    assert ga.same(got, host) is None, "%s differs from the host form" % ga.same(got, host)
    t = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(dt)).cuda()
    wk, wd, ws, wm = st.rerank_device(t(queries, np.float32), t(keys, np.int32), R, counts=t(counts, np.int32), values=t(values, np.float32))
    wrapper = dict(keys=wk.cpu().numpy().view(np.uint32), dist=wd.cpu().numpy(), sizes=ws.cpu().numpy(), missing=np.int64(wm))
    assert ga.same(got, wrapper) is None, "%s differs from the wrapper's call" % ga.same(got, wrapper)
    assert host["missing"] >= 2 and host["sizes"][0] > 1
    st.close()


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_put_device_and_remove_device(pyqadc, dtype, align):
    """a keyed store's life through the device forms: a fill, a put of new keys and overwrites whose last entry repeats an earlier key
    (the last occurrence wins), a removal whose last entry repeats an earlier one (counted once)"""
    rng = np.random.default_rng(47)
    dim = 65
    pool = rng.permutation(3000)[:400].astype(np.uint32) + 16
    fill, fresh = pool[:200], pool[200:300]
    v_fill = rng.normal(size=(200, dim)).astype(np.float32)
    put_labels = np.concatenate([fresh, fill[:50], fresh[7:8]])             # 100 new, 50 overwrites, a duplicate at the last position
    v_put = rng.normal(size=(len(put_labels), dim)).astype(np.float32)
    rm_labels = np.concatenate([fill[40:90], fresh[:10], pool[300:305], fill[45:46]])   # held, held, never held, a duplicate last
    queries = rng.normal(size=(2, dim)).astype(np.float32)
    keys = np.tile(pool, (2, 1))
    bystanders = quiet(fill[100:])                                           # held, and in neither list: what P2's label guards hold
    assert len(bystanders) > 50

    ref = pyqadc.Refine(dim, dtype, keyed=True)
    ref.put(v_fill, fill)
    ref.put(v_put, put_labels)
    want_put = state(ref, queries, keys)
    assert ref.remove(rm_labels) == 60
    want = state(ref, queries, keys)
    ref.close()
    assert want_put["live"] == 300 and want["live"] == 240 and want["rows_free"] == 60

    def call(a):
        L = pyqadc.lib()
        st = pyqadc.Refine(dim, dtype, keyed=True)
        st.put(v_fill, fill)
        pv = a.place(v_put, align, "in", name="d_vectors")
        pl = a.place(put_labels, align, "in", guard=bystanders, name="d_labels (put)")
        rl = a.place(rm_labels, align, "in", guard=bystanders, name="d_labels (remove)")
        a.snapshot()
        assert L.qadc_refine_put_device(st._h, a.ptr(pv), a.ptr(pl), len(put_labels)) == 0, L.qadc_last_error()
        a.check_untouched([])
        got = {"put " + k: v for k, v in state(st, queries, keys).items()}
        removed = C.c_uint64(0)
        assert L.qadc_refine_remove_device(st._h, a.ptr(rl), len(rm_labels), C.byref(removed)) == 0, L.qadc_last_error()
        a.check_untouched([])
        got.update(state(st, queries, keys), removed=np.int64(removed.value))
        st.close()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=1 << 20)
    assert got["removed"] == 60
    assert ga.same(got, want) is None, "%s differs from the host form after the removal" % ga.same(got, want)
    assert ga.same({k[4:]: v for k, v in got.items() if k.startswith("put ")}, want_put) is None, "the put differs from the host form"


@path_independent
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_refine_device_calls_refuse_pointers_below_the_stated_alignment(pyqadc, keyed):
    """each device pointer in turn two bytes off its 4: QADC_E_ARG before any HIP call, no byte written, the store as before"""
    rng = np.random.default_rng(53)
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    dim, rows, nq, r_in, R = 8, 100, 2, 20, 25
    vec = rng.normal(size=(rows, dim)).astype(np.float32)
    labels = np.arange(rows, dtype=np.uint32) + 16
    st = pyqadc.Refine(dim, "f32", keyed=keyed)
    if keyed:
        st.put(vec, labels)
    else:
        st.add(vec, 16)
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    keys = labels[rng.integers(0, rows, (nq, r_in))]
    before = state(st, queries, keys)
    a = ga.Arena(ga.P2, backend="torch", capacity=2 << 20)
    ins = [a.place(queries, 4, "in", name="d_queries"), a.place(keys, 4, "in", guard=labels, name="d_keys"),
           a.place(np.full(nq, r_in, np.int32), 4, "in", name="d_counts"), a.place(np.zeros((nq, r_in), np.float32), 4, "in", name="d_values")]
    outs = [a.place(np.empty((nq, R), np.uint32), 4, "out", name="d_out_keys"), a.place(np.empty((nq, R), np.float32), 4, "out", name="d_out_dist"),
            a.place(np.empty(nq, np.int32), 4, "out", name="d_out_sizes")]
    more = a.place(vec[:10], 4, "in", name="d_vectors")
    more_labels = a.place(labels[:10] + 1000, 4, "in", name="d_labels")
    missing = C.c_uint64(0)
    a.snapshot()
    for bad in range(7):
        p = [a.ptr(v) + (2 if i == bad else 0) for i, v in enumerate(ins + outs)]
        assert L.qadc_refine_rerank_device(st._h, nq, p[0], r_in, p[1], p[2], p[3], R, p[4], p[5], p[6], C.byref(missing)) == E, bad
        assert b"must be 4-byte aligned" in L.qadc_last_error()
    if keyed:
        assert L.qadc_refine_put_device(st._h, a.ptr(more) + 2, a.ptr(more_labels), 10) == E
        assert L.qadc_refine_put_device(st._h, a.ptr(more), a.ptr(more_labels) + 2, 10) == E
        assert L.qadc_refine_remove_device(st._h, a.ptr(more_labels) + 2, 10, None) == E
    else:
        assert L.qadc_refine_add_device(st._h, a.ptr(more) + 2, 10, 16 + rows) == E
    a.check_untouched([])
    assert ga.same(state(st, queries, keys), before) is None
    p = [a.ptr(v) for v in ins + outs]
    assert L.qadc_refine_rerank_device(st._h, nq, p[0], r_in, p[1], p[2], p[3], R, p[4], p[5], p[6], C.byref(missing)) == 0
    a.check_untouched(outs)
    assert np.array_equal(a.host(outs[0])[:, :r_in], before["keys"])
    st.close()
