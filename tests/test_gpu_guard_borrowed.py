"""GPU: a borrowed partition (qadc_index_add_partition_device) on a guard-band arena (tests/guard_arena.py; DESIGN.md section
6.1), under the three scan paths: its codes and labels are read in place by every query, so the guard bands begin at the end of the
documented readable extent — size * M/2 rounded up to 16 bytes — and the padding bytes inside that extent take both poisons too.

W  no byte of the arena changes; R  the heaps of qadc_query_scan are the same under both poisons and equal those of an index that
owns a copy of the partition; A  d_codes at 16 bytes and nothing coarser, d_labels at 4, and both at 256."""
import ctypes as C

import numpy as np
import pytest

import guard_arena as ga
from helpers import float_tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = (301, 4099)                                          # 301 * 8 bytes is no multiple of 16; 4099 rows: more than one workgroup


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def heaps(idx, tables, nq, R):
    got = idx.query_scan(np.zeros((nq, 1), np.int32), tables.copy(), R)      # (tables are mutated in place)
    assert (got["status"] == 0).all()
    return dict(keys=got["keys"], values=got["values"], sizes=got["sizes"])


@pytest.mark.parametrize("align", ["min", 256])
@pytest.mark.parametrize("labelled", [False, True], ids=["positions", "labels"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("M", [16, 32])
def test_a_borrowed_partition_is_read_inside_its_extent_only(pyqadc, scan_path, M, size, labelled, align):
    rng = np.random.default_rng(M + size)
    cs, nq, R = M // 2, 3, 100
    codes = rng.integers(0, 256, (size, cs), dtype=np.uint8)
    labels = (rng.permutation(3 * size)[:size] + 16).astype(np.uint32) if labelled else None
    tables = float_tables(rng, nq, 1, M)
    extent = -(-size * cs // 16) * 16
    quiet = None if labels is None else labels[~(labels[:, None].view(np.uint8) == 0xFF).any(1)][:50]   # (no 0xFF byte: P2's guard labels)
    assert M == 32 or size * cs % 16 == 8

    own = pyqadc.Index(M)
    own.add_partitions([codes], None if labels is None else [labels])
    own.finalize(0.5)
    want = heaps(own, tables, nq, R)
    own.close()

    def call(a):
        window = np.full(extent, 0xFF if a.poison == ga.P1 else 0x00, np.uint8)        # the padding inside the extent is poisoned too
        window[:size * cs] = codes.reshape(-1)
        d_codes = a.place(window, 16 if align == "min" else align, "in", name="d_codes (its readable extent)")
        d_labels = a.place(labels, 4 if align == "min" else align, "in", guard=quiet, name="d_labels") if labelled else None
        idx = pyqadc.Index(M)
        a.snapshot()
        idx.add_partition_device(a.ptr(d_codes), size, a.ptr(d_labels) if labelled else None, keepalive=a.buf)
        idx.finalize(0.5)
        got = heaps(idx, tables, nq, R)
        a.check_untouched([])
        idx.close()
        return got

    got = ga.under_both_poisons(call, backend="torch", capacity=1 << 20)
    assert ga.same(got, want) is None, "%s differs from the index that owns the partition (%s)" % (ga.same(got, want), scan_path)


def test_a_borrowed_partition_below_the_stated_alignment_is_refused(pyqadc, scan_path):
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 256, (304, 8), dtype=np.uint8)
    labels = np.arange(304, dtype=np.uint32) + 16
    a = ga.Arena(ga.P2, backend="torch", capacity=1 << 20)
    low = a.place(codes, 8, "in", name="d_codes at 8 bytes")
    good = a.place(codes, 16, "in", name="d_codes")
    lab = a.place(labels, 4, "in", name="d_labels")
    L, E = pyqadc.lib(), pyqadc.QADC_E_ARG
    idx = pyqadc.Index(16)
    a.snapshot()
    assert L.qadc_index_add_partition_device(idx._h, C.c_void_p(a.ptr(low)), C.c_void_p(a.ptr(lab)), 304) == E
    assert b"d_codes must be 16-byte aligned" in L.qadc_last_error()
    assert L.qadc_index_add_partition_device(idx._h, C.c_void_p(a.ptr(good)), C.c_void_p(a.ptr(lab) + 2), 304) == E
    assert b"d_labels must be 4-byte aligned" in L.qadc_last_error()
    assert idx.partition_count() == 0
    idx.add_partition_device(a.ptr(good), 304, a.ptr(lab), keepalive=a.buf)
    idx.finalize(0.5)
    tables = float_tables(rng, 2, 1, 16)
    got = heaps(idx, tables, 2, 50)
    a.check_untouched([])
    own = pyqadc.Index(16)
    own.add_partitions([codes], [labels])
    own.finalize(0.5)
    assert ga.same(got, heaps(own, tables, 2, 50)) is None
    idx.close()
    own.close()
