"""GPU: the memory behaviour of the database-side device entry points at the C-ABI, on guard-band arenas
(tests/guard_arena.py): qadc_adc_index_add_vectors_device / _labelled_device and qadc_index_add_vectors_device / _labelled_device
(8x8, 2x16, 16x4, 32x4; flat and IVF with K = 3), qadc_adc_index_remove_labels_device, qadc_index_remove_labels_device,
qadc_adc_filter_create_device (lists of 1, 255 and 257 keys) and qadc_pq_encode / qadc_pq_encode_mode (16x4, 32x4, both forms).

W  no byte of the arena but d_codes changes; R  the index after the call — read_partition of every partition and one search — is the
same under both guard poisons and equals the host form's; F  every byte of d_codes [n][M/2] is written, and the byte right behind
it is not; A  d_vectors of the float-ADC add at 16 bytes, every other pointer at its element's size (d_codes at 1), and all at 256.

Under P2 the label guards cycle through labels the index holds and the list does not: one stray read removes or filters a row more."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = ["min", 256]
N, K, DS = 1001, 3, 8
SHAPES = ["8x8", "2x16", "16x4", "32x4"]
VEC_ALIGN = {"8x8": 16, "2x16": 16, "16x4": 4, "32x4": 4}    # include/qadc.h: the float-ADC add takes d_vectors at 16 bytes


def al(align, minimum):
    return minimum if align == "min" else align


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


class Data:
    """the quantizers and vectors of one shape, drawn once per module"""

    def __init__(self, shape):
        rng = np.random.default_rng(sum(map(ord, shape)))
        self.shape, self.nsq, self.bits = shape, int(shape.split("x")[0]), int(shape.split("x")[1])
        self.dim = self.nsq * DS
        self.codebooks = rng.normal(size=(self.nsq, 1 << self.bits, DS)).astype(np.float32)
        self.coarse = rng.normal(size=(K, self.dim)).astype(np.float32)
        self.first = rng.normal(size=(100, self.dim)).astype(np.float32)     # what the index holds before the call
        self.first_labels = (rng.permutation(5000)[:100] + 70000).astype(np.uint32)
        self.vectors = rng.normal(size=(N, self.dim)).astype(np.float32)
        self.labels = (rng.permutation(60000)[:N] + 300).astype(np.uint32)
        self.labels[-1] = self.labels[5]                                     # a repeat, at the last position
        self.queries = rng.normal(size=(3, self.dim)).astype(np.float32)

    def index(self, pyqadc, ivf):
        if self.bits == 4:
            idx = pyqadc.Index(self.nsq)
        else:
            idx = pyqadc.AdcIndex.create16(self.nsq) if self.bits == 16 else pyqadc.AdcIndex(self.nsq, 8)
        idx.set_pq(self.codebooks)
        if ivf:
            idx.set_coarse(self.coarse)
        return idx

    def state(self, idx, ivf):
        """read_partition of every partition and one search"""
        out = {}
        for p in range(idx.partition_count()):
            codes, labels = idx.read_partition(p)
            out["codes %d" % p] = codes
            if labels is not None:
                out["labels %d" % p] = labels
        ma = 2 if ivf else 1
        if self.bits == 4:
            idx.finalize(0.5)
            found = idx.search(self.queries, ma, 50)
            out.update(keys=found["keys"], values=found["values"], sizes=found["sizes"])
        else:
            keys, vals, sizes, _ = idx.search(self.queries, ma, 50)
            out.update(keys=keys, values=vals, sizes=sizes)
        return out


@pytest.fixture(scope="module")
def data():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Data(shape)
        return made[shape]
    return get


def quiet(labels):
    labels = np.ascontiguousarray(labels, np.uint32)
    return labels[~(labels[:, None].view(np.uint8) == 0xFF).any(1)]


ADD_KINDS = ["flat", "ivf", "ivf-labelled"]


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("kind", ADD_KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_add_vectors_device(pyqadc, data, shape, kind, align):
    d, ivf, labelled = data(shape), kind != "flat", kind == "ivf-labelled"
    prefix = "qadc_index_" if d.bits == 4 else "qadc_adc_index_"
    L = pyqadc.lib()

    def filled():
        idx = d.index(pyqadc, ivf)
        if labelled:
            idx.add_vectors(d.first, labels=d.first_labels)
        else:
            idx.add_vectors(d.first, labels_offset=0)
        return idx

    ref = filled()
    if labelled:
        ref.add_vectors(d.vectors, labels=d.labels)
    else:
        ref.add_vectors(d.vectors, labels_offset=100)
    want = d.state(ref, ivf)
    ref.close()
    assert sum(len(want["codes %d" % p]) for p in range(K if ivf else 1)) == N + 100

    def call(a):
        idx = filled()
        v = a.place(d.vectors, al(align, VEC_ALIGN[shape]), "in", name="d_vectors")
        a_labels = a.place(d.labels, al(align, 4), "in", guard=quiet(d.first_labels), name="d_labels") if labelled else None
        a.snapshot()
        if labelled:
            rc = getattr(L, prefix + "add_vectors_labelled_device")(idx._h, a.ptr(v), a.ptr(a_labels), N, 1)
        else:
            rc = getattr(L, prefix + "add_vectors_device")(idx._h, a.ptr(v), N, 100, 1)
        assert rc == 0, L.qadc_last_error()
        a.check_untouched([])
        got = d.state(idx, ivf)
        idx.close()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=d.vectors.nbytes + (1 << 20))
    assert set(got) == set(want) and ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
@pytest.mark.parametrize("shape", ["8x8", "16x4"])
def test_add_vectors_labelled_device_over_the_pass_edge(pyqadc, shape):
    """262144 + 5 vectors at the smallest dim of the shape: the second pass reads d_vectors and d_labels from an offset, and its five
    rows end right in front of the guard bands"""
    nsq, bits = (int(x) for x in shape.split("x"))
    rng = np.random.default_rng(nsq)
    n, dim = pyqadc.QADC_ADC_ADD_CHUNK + 5, nsq
    assert pyqadc.QADC_INDEX_ADD_CHUNK == pyqadc.QADC_ADC_ADD_CHUNK
    codebooks = rng.normal(size=(nsq, 1 << bits, 1)).astype(np.float32)
    coarse = rng.normal(size=(K, dim)).astype(np.float32)
    vectors = rng.normal(size=(n, dim)).astype(np.float32)
    labels = rng.permutation(n).astype(np.uint32) + 70000
    first, first_labels = vectors[:64] + np.float32(0.5), np.arange(300, 364, dtype=np.uint32)
    queries = vectors[1000:1003] + np.float32(0.01)
    prefix = "qadc_index_" if bits == 4 else "qadc_adc_index_"

    def filled():
        idx = pyqadc.Index(nsq) if bits == 4 else pyqadc.AdcIndex(nsq, 8)
        idx.set_pq(codebooks)
        idx.set_coarse(coarse)
        idx.add_vectors(first, labels=first_labels)
        return idx

    def state(idx):
        out = {}
        for p in range(K):
            out["codes %d" % p], out["labels %d" % p] = idx.read_partition(p)
        if bits == 4:
            idx.finalize(0.01)
            found = idx.search(queries, 2, 50)
            out.update(keys=found["keys"], values=found["values"], sizes=found["sizes"])
        else:
            out.update(zip(("keys", "values", "sizes"), idx.search(queries, 2, 50)[:3]))
        return out

    ref = filled()
    ref.add_vectors(vectors, labels=labels)
    want = state(ref)
    ref.close()

    def call(a):
        idx = filled()
        v = a.place(vectors, VEC_ALIGN[shape], "in", name="d_vectors")
        lab = a.place(labels, 4, "in", guard=first_labels, name="d_labels")
        a.snapshot()
        rc = getattr(pyqadc.lib(), prefix + "add_vectors_labelled_device")(idx._h, a.ptr(v), a.ptr(lab), n, 1)
        assert rc == 0, pyqadc.lib().qadc_last_error()
        a.check_untouched([])
        got = state(idx)
        idx.close()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=vectors.nbytes + labels.nbytes + (1 << 20))
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


LISTS = [1, 255, 257]


def removal_setup(pyqadc, d, count):
    """an IVF index with N labelled rows; the list: `count` labels it holds (the last repeats the first where there is room), and
    the bystanders: labels it holds that are not in the list"""
    idx = d.index(pyqadc, True)
    labels = d.labels.copy()
    labels[-1] = 299                                                         # (all distinct here)
    idx.add_vectors(d.vectors, labels=labels)
    rm = labels[7:7 + count].copy()
    if count > 1:
        rm[-1] = rm[0]
    return idx, labels, rm, quiet(labels[400:])


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("count", LISTS)
@pytest.mark.parametrize("shape", ["8x8", "16x4"])
def test_remove_labels_device(pyqadc, data, shape, count, align):
    d = data(shape)
    L = pyqadc.lib()
    call_c = L.qadc_index_remove_labels_device if d.bits == 4 else L.qadc_adc_index_remove_labels_device
    ref, labels, rm, bystanders = removal_setup(pyqadc, d, count)
    gone = ref.remove_labels(rm)
    want = dict(d.state(ref, True), removed=np.int64(gone))
    ref.close()
    assert gone == len(set(rm.tolist())) == max(count - 1, 1)

    def call(a):
        idx = removal_setup(pyqadc, d, count)[0]
        lst = a.place(rm, al(align, 4), "in", guard=bystanders, name="d_labels")
        removed = C.c_uint64(0)
        a.snapshot()
        assert call_c(idx._h, a.ptr(lst), count, C.byref(removed)) == 0, L.qadc_last_error()
        a.check_untouched([])
        got = dict(d.state(idx, True), removed=np.int64(removed.value))
        idx.close()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=1 << 20)
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("mode", ["exclude", "allow"])
@pytest.mark.parametrize("count", LISTS)
def test_filter_create_device(pyqadc, data, count, mode, align):
    d = data("8x8")
    L = pyqadc.lib()
    idx, labels, keys, bystanders = removal_setup(pyqadc, d, count)

    def answers(f):
        found = idx.search(d.queries, 2, 50, filters=[f, None, f])
        return dict(info=np.array([f.info()[k] for k in ("lo", "hi", "bitmap_bytes")], np.int64), keys=found[0], values=found[1], sizes=found[2])

    ref = pyqadc.AdcFilter(keys, mode)
    want = answers(ref)
    ref.close()

    def call(a):
        lst = a.place(keys, al(align, 4), "in", guard=bystanders, name="d_keys")
        a.snapshot()
        f = pyqadc.AdcFilter.__new__(pyqadc.AdcFilter)
        f._create(lambda h: L.qadc_adc_filter_create_device(h, pyqadc.AdcFilter._mode(mode), a.ptr(lst), count, 0), 0)
        a.check_untouched([])
        got = answers(f)
        f.close()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=1 << 20)
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)
    idx.close()


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("form", [0, 1], ids=["direct", "expansion"])
@pytest.mark.parametrize("shape", ["16x4", "32x4"])
def test_pq_encode(pyqadc, data, shape, form, align):
    """d_codes is byte-granular: at the smallest alignment it starts at an odd address, and the guard byte right behind
    d_codes [n][M/2] is the first thing a one-byte overrun would hit"""
    d = data(shape)
    L = pyqadc.lib()
    want = pyqadc.pq_encode(d.codebooks, d.vectors, encode_form=form)
    cb = d.codebooks.ctypes.data_as(C.POINTER(C.c_float))

    def call(a):
        v = a.place(d.vectors, al(align, 4), "in", name="d_vectors")
        codes = a.place(np.empty((N, d.nsq // 2), np.uint8), al(align, 1), "out", name="d_codes")
        a.snapshot()
        if form == 1:
            rc = L.qadc_pq_encode(d.nsq, d.dim, cb, C.c_void_p(a.ptr(v)), N, C.c_void_p(a.ptr(codes)), 0)
        else:
            rc = L.qadc_pq_encode_mode(d.nsq, d.dim, cb, C.c_void_p(a.ptr(v)), N, C.c_void_p(a.ptr(codes)), 0, 1, 0)
        assert rc == 0, L.qadc_last_error()
        a.check_untouched([codes])
        return dict(codes=a.host(codes))

    got = ga.under_both_poisons(call, backend="torch", capacity=d.vectors.nbytes + (1 << 20))
    assert np.array_equal(got["codes"], want)


@path_independent
def test_build_calls_refuse_pointers_below_the_stated_alignment(pyqadc, data):
    """every pointer in turn below its stated alignment: QADC_E_ARG before any HIP call, the arena unchanged, the index as before"""
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    a = ga.Arena(ga.P2, backend="torch", capacity=2 << 20)
    d8, d4 = data("8x8"), data("16x4")
    v8 = a.place(d8.vectors[:50], 4, "in", name="d_vectors (8x8) at 4 bytes")
    v8_8 = a.place(d8.vectors[:50], 8, "in", name="d_vectors (8x8) at 8 bytes")
    v8_ok = a.place(d8.vectors[:50], 16, "in", name="d_vectors (8x8)")
    v4 = a.place(d4.vectors[:50], 4, "in", name="d_vectors (16x4)")
    lab = a.place(d8.labels[:50], 4, "in", name="d_labels")
    codes = a.place(np.empty((50, 8), np.uint8), 1, "out", name="d_codes")
    removed = C.c_uint64(0)
    for d, vec_low in ((d8, (a.ptr(v8), a.ptr(v8_8), a.ptr(v8_ok) + 2)), (d4, (a.ptr(v4) + 2,))):
        prefix = "qadc_index_" if d.bits == 4 else "qadc_adc_index_"
        idx = d.index(pyqadc, True)
        idx.add_vectors(d.first, labels=d.first_labels)
        before = d.state(idx, True)
        good = a.ptr(v4) if d.bits == 4 else a.ptr(v8_ok)
        a.snapshot()
        for p in vec_low:
            assert getattr(L, prefix + "add_vectors_device")(idx._h, p, 50, 0, 1) == E and b"d_vectors must be" in L.qadc_last_error()
            assert getattr(L, prefix + "add_vectors_labelled_device")(idx._h, p, a.ptr(lab), 50, 1) == E
        assert getattr(L, prefix + "add_vectors_labelled_device")(idx._h, good, a.ptr(lab) + 2, 50, 1) == E and b"d_labels must be" in L.qadc_last_error()
        assert getattr(L, prefix + "remove_labels_device")(idx._h, a.ptr(lab) + 2, 50, C.byref(removed)) == E
        a.check_untouched([])
        assert ga.same(d.state(idx, True), before) is None
        idx.close()
    h = C.c_void_p(7)
    a.snapshot()
    assert L.qadc_adc_filter_create_device(C.byref(h), 0, a.ptr(lab) + 2, 50, 0) == E and not h.value and b"d_keys must be" in L.qadc_last_error()
    cb = d4.codebooks.ctypes.data_as(C.POINTER(C.c_float))
    assert L.qadc_pq_encode(16, d4.dim, cb, C.c_void_p(a.ptr(v4) + 2), 50, C.c_void_p(a.ptr(codes)), 0) == E
    a.check_untouched([])
    assert L.qadc_pq_encode(16, d4.dim, cb, C.c_void_p(a.ptr(v4)), 50, C.c_void_p(a.ptr(codes)), 0) == 0
    a.check_untouched([codes])
    assert np.array_equal(a.host(codes), pyqadc.pq_encode(d4.codebooks, d4.vectors[:50]))
