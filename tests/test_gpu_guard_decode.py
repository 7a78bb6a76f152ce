"""GPU: the memory behaviour of the decoder's device entry points at the C-ABI, on guard-band arenas
(tests/guard_arena.py): qadc_pq_decode_device, qadc_adc_index_reconstruct_device and qadc_adc_index_reconstruct_rows_device through
raw ctypes calls.

W  every byte outside d_out, d_err_out and d_where_out is unchanged;
R  the results under the two guard poisons are bit-identical and equal the host form on the same data;
F  every declared slot is written — the missing rows' 0x7FC00000 fill and their where entries are asserted under the 0x5A output
   poison as well as the 0xFF one;
A  every buffer at 4 bytes and nothing coarser (the gather then stores float by float), and at 256 (16-byte stores).

Under P2 the key guards cycle through keys the index holds and the list does not, the assign guards through valid partitions and the
float guards hold zeros: one stray read changes a row."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
import pq_decode_compose as pdc
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = [4, 256]


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


F32P = C.POINTER(C.c_float)
SHAPES = [(16, 4, 32, False), (16, 4, 16, True), (8, 8, 24, False), (8, 8, 21 * 8, True), (2, 16, 6, False), (2, 16, 6, True)]


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("nsq,bits,dim,rotated", SHAPES, ids=["%dx%d-dim%d-%s" % (s[0], s[1], s[2], "rotated" if s[3] else "plain") for s in SHAPES])
def test_pq_decode_device(pyqadc, nsq, bits, dim, rotated, align):
    rng = np.random.default_rng(dim + align)
    n, K = 301, 4
    c = pdc.random_case(rng, nsq, bits, dim, n, K, rotated)
    c["assign"][[7, 300]] = (-1, K)                                         # missing rows: their fill is an output like any other
    codes = np.ascontiguousarray(c["codes"], "<u2" if bits == 16 else np.uint8)
    code_bytes = codes.view(np.uint8).reshape(n, -1)
    want = pyqadc.pq_decode(c["cb"], c["codes"], assign=c["assign"], coarse=c["coarse"], rotation=c["rotation"], vectors=c["vectors"])
    L = pyqadc.lib()

    def call(a):
        d_assign = a.place(c["assign"], align, "in", guard=np.array([1, 2, 3], np.int32), name="d_assign")
        d_codes = a.place(code_bytes, min(align, 256), "in", name="d_codes")
        d_vec = a.place(c["vectors"], align, "in", name="d_vectors")
        d_out = a.place(np.empty((n, dim), np.float32), align, "out", name="d_out")
        d_err = a.place(np.empty(n, np.float32), align, "out", name="d_err_out")
        a.snapshot()
        rc = L.qadc_pq_decode_device(nsq, bits, dim, c["cb"].ctypes.data_as(F32P), None if not rotated else c["rotation"].ctypes.data_as(F32P), K,
                                     c["coarse"].ctypes.data_as(F32P), a.ptr(d_assign), a.ptr(d_codes), n, a.ptr(d_vec), a.ptr(d_out),
                                     a.ptr(d_err), 0)
        assert rc == 0, L.qadc_last_error()
        a.check_untouched([d_out, d_err])
        got = dict(out=a.host(d_out), err=a.host(d_err))
        assert (got["out"][[7, 300]].view(np.uint32) == pdc.NAN_BITS).all() and (got["err"][[7, 300]].view(np.uint32) == pdc.NAN_BITS).all()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    assert ga.same(got, dict(out=want[0], err=want[1])) is None, "%s differs from the host form" % ga.same(got, dict(out=want[0], err=want[1]))


def ivf_index(pyqadc, rng, nsq, bits, dim, rotated, n=1500, K=5):
    c = pdc.random_case(rng, nsq, bits, dim, 1, K, rotated)
    idx = pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)
    idx.set_pq(c["cb"])
    idx.set_rotation(c["rotation"])
    idx.set_coarse(c["coarse"] * 4)
    vec = (c["coarse"][rng.integers(0, K, n)] * 4 + rng.normal(size=(n, dim))).astype(np.float32)
    labels = (rng.permutation(30000)[:n] + 16).astype(np.uint32)
    idx.add_vectors(vec, labels=labels)
    return idx, labels


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("nsq,bits,dim,rotated", [(8, 8, 24, False), (8, 8, 24, True), (2, 16, 6, False)], ids=["8x8-plain", "8x8-rotated", "2x16-plain"])
def test_reconstruct_device_and_rows_device(pyqadc, nsq, bits, dim, rotated, align):
    rng = np.random.default_rng(dim + bits + align)
    idx, labels = ivf_index(pyqadc, rng, nsq, bits, dim, rotated)
    held = labels[~(labels[:, None].view(np.uint8) == 0xFF).any(1)]
    keys = np.concatenate([held[:200], [3, 5, 40000], held[:7]]).astype(np.uint32)    # three missing keys, repeats
    others = held[400:]                                                     # held, and not in the list: what P2's key guards cycle through
    want, want_where = idx.reconstruct(keys)
    part = 2
    size = idx.partition_size(part)
    first, count = size // 4, size - size // 4
    want_rows = idx.reconstruct_rows(part, first, count)
    L = pyqadc.lib()

    def call(a):
        d_keys = a.place(keys, align, "in", guard=others, name="d_keys")
        d_out = a.place(np.empty((len(keys), dim), np.float32), align, "out", name="d_out")
        d_where = a.place(np.empty((len(keys), 2), np.uint32), align, "out", name="d_where_out")   # uint64 [count], as its 32-bit words
        d_rows = a.place(np.empty((count, dim), np.float32), align, "out", name="d_out (rows)")
        a.snapshot()
        assert L.qadc_adc_index_reconstruct_device(idx._h, a.ptr(d_keys), len(keys), a.ptr(d_out), a.ptr(d_where)) == 0, L.qadc_last_error()
        a.check_untouched([d_out, d_where])
        got = dict(out=a.host(d_out), where=a.host(d_where).view(np.uint64).reshape(-1))
        assert (got["where"][200:203] == pdc.MISSING).all() and (got["out"][200:203].view(np.uint32) == pdc.NAN_BITS).all()   # F
        assert (got["where"][:200] != pdc.MISSING).all()
        assert L.qadc_adc_index_reconstruct_rows_device(idx._h, part, first, count, a.ptr(d_rows)) == 0, L.qadc_last_error()
        a.check_untouched([d_out, d_where, d_rows])
        got["rows"] = a.host(d_rows)
        # where_out is optional: without it nothing but d_out changes
        a.snapshot()
        assert L.qadc_adc_index_reconstruct_device(idx._h, a.ptr(d_keys), len(keys), a.ptr(d_out), None) == 0, L.qadc_last_error()
        a.check_untouched([d_out])
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=2 << 20)
    host = dict(out=want, where=want_where, rows=want_rows)
    assert ga.same(got, host) is None, "%s differs from the host form" % ga.same(got, host)
    idx.close()


@path_independent
def test_decode_device_calls_refuse_pointers_below_the_stated_alignment(pyqadc):
    """each device pointer in turn two bytes off its 4: QADC_E_ARG before any HIP call, no byte written"""
    rng = np.random.default_rng(5)
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    idx, labels = ivf_index(pyqadc, rng, 8, 8, 24, False, n=200)
    c = pdc.random_case(rng, 8, 8, 24, 50, 3, False)
    a = ga.Arena(ga.P2, backend="torch", capacity=2 << 20)
    ins = [a.place(c["assign"], 4, "in", name="d_assign"), a.place(c["vectors"], 4, "in", name="d_vectors"), a.place(labels[:50], 4, "in", name="d_keys")]
    outs = [a.place(np.empty((50, 24), np.float32), 4, "out", name="d_out"), a.place(np.empty(50, np.float32), 4, "out", name="d_err_out"),
            a.place(np.empty((50, 2), np.uint32), 4, "out", name="d_where_out")]
    d_codes = a.place(c["codes"], 1, "in", name="d_codes")
    a.snapshot()
    cb, co = c["cb"].ctypes.data_as(F32P), c["coarse"].ctypes.data_as(F32P)
    for bad, name in ((0, b"d_assign"), (1, b"d_vectors"), (3, b"d_out"), (4, b"d_err_out")):
        p = [a.ptr(v) + (2 if i == bad else 0) for i, v in enumerate(ins + outs)]
        assert L.qadc_pq_decode_device(8, 8, 24, cb, None, 3, co, p[0], a.ptr(d_codes), 50, p[1], p[3], p[4], 0) == E
        assert name + b" must be 4-byte aligned" in L.qadc_last_error()
    for bad, name in ((2, b"d_keys"), (3, b"d_out"), (5, b"d_where_out")):
        p = [a.ptr(v) + (2 if i == bad else 0) for i, v in enumerate(ins + outs)]
        assert L.qadc_adc_index_reconstruct_device(idx._h, p[2], 50, p[3], p[5]) == E
        assert name + b" must be 4-byte aligned" in L.qadc_last_error()
    assert L.qadc_adc_index_reconstruct_rows_device(idx._h, 0, 0, 1, a.ptr(outs[0]) + 2) == E
    a.check_untouched([])
    p = [a.ptr(v) for v in ins + outs]
    assert L.qadc_pq_decode_device(8, 8, 24, cb, None, 3, co, p[0], a.ptr(d_codes), 50, p[1], p[3], p[4], 0) == 0    # codes at an odd address
    a.check_untouched(outs[:2])
    idx.close()
