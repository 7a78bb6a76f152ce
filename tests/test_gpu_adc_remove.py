"""Remove by label on the float-ADC index (qadc_adc_index_remove_labels, pyqadc.AdcIndex.remove_labels):
the rows whose label is in the caller's list leave their partitions in device memory, the others keep their order.

Every comparison is for equality — the call does no arithmetic on codes.  The model is numpy: partition p keeps
codes[~np.isin(labels, removed)], in order.  Partitions are made from random code bytes with add_partitions, so their sizes are
exact, and looked at through read_partition.  kRemoveTile (csrc/qadc_adc_kernels.h) is the number of rows one iteration of the
compaction holds in registers; the sizes and the removal patterns sit on its edges."""
import os
import re

import numpy as np
import pytest

import pyqadc
from helpers import path_independent
from test_gpu_adc_add import Quantizers, append, assert_partitions, group, read_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"constexpr int kRemoveTile = (\d+);", open(os.path.join(ROOT, "quick-adc_amd", "csrc", "qadc_adc_kernels.h")).read()).group(1))
SHAPES = [(4, 8), (8, 8), (16, 8), (2, 16), (4, 16), (8, 16)]                    # rows of 4, 8 and 16 bytes from both code widths
SIZES = [0, 1, T - 1, T, T + 1, 2 * T + 3]


def shape_id(s):
    return "%dx%d" % s


def new_index(shape):
    nsq, bits = shape
    return pyqadc.AdcIndex(nsq, 8) if bits == 8 else pyqadc.AdcIndex.create16(nsq)


def random_partitions(shape, sizes, seed):
    """[(codes, labels)] of the given sizes: random code bytes, labels distinct over the whole index, in no order"""
    nsq, bits = shape
    rng = np.random.default_rng(seed)
    total = int(np.sum(sizes))
    labels = rng.permutation(4 * total + 64)[:total].astype(np.uint32)
    parts, at = [], 0
    for n in sizes:
        codes = rng.integers(0, 1 << bits, (n, nsq)).astype(np.uint8 if bits == 8 else np.uint16)
        parts.append((codes, labels[at:at + n].copy()))
        at += n
    return parts


def build(shape, parts):
    idx = new_index(shape)
    idx.add_partitions([c for c, _ in parts], [l for _, l in parts])
    return idx


def model_remove(parts, removed):
    """-> (the partitions without the rows whose label is in `removed`, the number of rows that went)"""
    removed = np.asarray(removed, np.uint32)
    out, gone = [], 0
    for c, l in parts:
        keep = ~np.isin(l, removed)
        out.append((c[keep], l[keep]))
        gone += int((~keep).sum())
    return out, gone


def check(idx, want, what=""):
    # (an index that holds no row at all cannot say whether it is labelled: read_partition then hands out no labels)
    got = [(gc, wl if gl is None and len(wl) == 0 else gl) for (gc, gl), (_, wl) in zip(read_all(idx), want)]
    assert idx.partition_count() == len(want), what
    assert_partitions(got, want, what)
    assert [idx.partition_size(p) for p in range(len(want))] == [len(c) for c, _ in want], what


# ---- 1. partition sizes x removal patterns -------------------------------------------------------------------------------------

PATTERNS = {
    "nothing": lambda n: np.zeros(n, bool),
    "every-row": lambda n: np.ones(n, bool),
    "row-0": lambda n: np.arange(n) == 0,                                        # the writes overlap the tile being read
    "last-row": lambda n: np.arange(n) == n - 1,
    "every-other-row": lambda n: np.arange(n) % 2 == 0,
    "run-across-a-tile-edge": lambda n: (np.arange(n) >= T - 2) & (np.arange(n) < T + 2),
    "all-of-tile-0": lambda n: np.arange(n) < T,                                 # the write lags a whole tile
    "all-but-the-last-row": lambda n: np.arange(n) != n - 1,                     # the last row moves from n - 1 to 0
}


@path_independent
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_pattern_on_every_partition_size(shape):
    parts = random_partitions(shape, SIZES, 100 * shape[0] + shape[1])
    absent = np.uint32(max(int(l.max()) for _, l in parts if len(l)) + 5)
    for name, pattern in PATTERNS.items():
        removed = np.concatenate([l[pattern(len(l))] for _, l in parts] + [np.array([absent], np.uint32)])
        want, gone = model_remove(parts, removed)
        assert gone == len(removed) - 1 and (name != "nothing" or gone == 0)
        idx = build(shape, parts)
        try:
            moved = idx.relocations()
            assert idx.remove_labels(np.random.default_rng(1).permutation(removed)) == gone, name
            check(idx, want, name)
            assert idx.relocations() == moved, name
        finally:
            idx.close()


# ---- 2. label edges ------------------------------------------------------------------------------------------------------------

@path_independent
def test_label_edges():
    shape = (8, 8)
    top = 2 ** 32 - 1
    parts = [(c, l + np.uint32(10000)) for c, l in random_partitions(shape, [40, T + 3, 0, 17], 7)]   # labels from 10000, then the hand-made ones
    parts[0][1][:6] = [0, top, 999, 1000, 1036, 1037]
    parts[1][1][[0, T, T + 2]] = [1010, 1001, top - 1]
    parts[3][1][:3] = [1010, 1, 998]                                             # 1010: two rows in two partitions
    idx = build(shape, parts)
    try:
        def step(removed, gone, what):
            nonlocal parts
            parts, model_gone = model_remove(parts, removed)
            assert model_gone == gone, what
            assert idx.remove_labels(removed) == gone, what
            check(idx, parts, what)

        before = idx.relocations()
        step([2000, 2001, 5000], 0, "a list that hits nothing")
        step([], 0, "an empty list")
        assert idx.relocations() == before
        # lo = 1000 and hi = 1036 are held and go; 999 and 1037 are held and stay; the span, 37 bits, is no multiple of 32
        step([1036, 1000, 1036, 1000, 1000], 2, "lo and hi, duplicates")
        assert all(x in np.concatenate([l for _, l in parts]) for x in (999, 1037))
        step([1010, 1010], 2, "a label held by two rows in two partitions")
        step([top, 0], 2, "labels 0 and 2^32 - 1: the whole label space")
        step(np.array([top - 1, 1], np.uint32), 2, "a span that ends one below the top")
        assert idx.relocations() == before
    finally:
        idx.close()


# ---- 3. partition counts -------------------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("K", [1, 300])
def test_partition_counts(K):
    shape = (4, 16)
    sizes = np.zeros(K, np.int64)
    sizes[[0, K // 2, K - 1][:K]] = [T + 5, 9, 300][:K]                          # K = 300: most partitions empty
    if K == 300:
        sizes[[7, 280]] = [50, 2 * T]                                            # ... and two that hold rows and are not hit
    parts = random_partitions(shape, sizes, K)
    hit = [p for p in (0, K // 2, K - 1) if p < K]
    removed = np.concatenate([parts[p][1][::3] for p in sorted(set(hit))])
    want, gone = model_remove(parts, removed)
    idx = build(shape, parts)
    try:
        assert idx.remove_labels(removed) == gone > 0
        check(idx, want)
    finally:
        idx.close()


# ---- 4. interplay with growth --------------------------------------------------------------------------------------------------

@path_independent
def test_add_vectors_fills_the_freed_room_in_place():
    q = Quantizers(8, 8, 64, n=4000, seed=9)
    a, codes = q.encoded()
    first = 1000
    idx = q.index()
    try:
        idx.reserve(np.bincount(a[:first], minlength=q.K))                       # full partitions: one more row would relocate
        idx.add_vectors(q.vectors[:first])
        assert idx.relocations() == 0
        model = group(a[:first], codes[:first], q.K)
        removed = np.arange(0, first, 3, dtype=np.uint32)
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == len(removed)
        # fewer new rows than were removed from each partition, more than the row a 16-byte region rounds up to
        freed = np.bincount(a[:first][removed], minlength=q.K)
        assert (freed >= 4).all()
        pick = np.concatenate([first + np.flatnonzero(a[first:] == p)[:freed[p] - 1] for p in range(q.K)])
        pick.sort()
        assert (np.bincount(a[pick], minlength=q.K) == freed - 1).all()
        idx.add_vectors(q.vectors[pick], labels_offset=50000)
        assert idx.relocations() == 0                                            # the freed room took them
        model = append(model, group(a[pick], codes[pick], q.K, 50000))
        check(idx, model, "the new rows stand behind the survivors")
        # an add that does relocate, then another removal
        rest = np.setdiff1d(np.arange(first, 4000), pick)
        idx.add_vectors(q.vectors[rest], labels_offset=100000)
        assert idx.relocations() == 1
        model = append(model, group(a[rest], codes[rest], q.K, 100000))
        removed = np.concatenate([np.arange(1, first, 3), 50000 + np.arange(0, len(pick), 2), 100000 + np.arange(5, len(rest), 7)]).astype(np.uint32)
        model, gone = model_remove(model, removed)
        assert idx.remove_labels(removed) == gone == len(removed)
        assert idx.relocations() == 1
        check(idx, model, "after the relocation")
    finally:
        idx.close()


# ---- 5. queries after a removal ------------------------------------------------------------------------------------------------

def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                                                        y.view(np.uint32) if y.dtype == np.float32 else y)


@path_independent
@pytest.mark.parametrize("shape", [(8, 8, 64), (2, 16, 16)], ids=lambda s: "%dx%d-d%d" % s)
def test_search_after_a_removal_equals_a_fresh_index(shape):
    nsq, bits, dim = shape
    n, ma, R, nq = 6000, 3, 100, 5
    q = Quantizers(nsq, bits, dim, n=n, seed=12)
    a, codes = q.encoded()
    rng = np.random.default_rng(45)
    queries = (q.coarse[rng.integers(0, q.K, nq)] + rng.normal(size=(nq, dim))).astype(np.float32)
    full = group(a, codes, q.K)
    small = int(np.argmin([len(c) for c, _ in full]))
    removed = np.concatenate([rng.permutation(n)[:n * 2 // 5], full[small][1][7:]]).astype(np.uint32)   # 40 %, and all but 7 rows of one partition
    model, gone = model_remove(full, removed)
    assert 0 < min(len(c) for c, _ in model) < R
    got, ref = q.index(), q.index()
    try:
        got.add_partitions([c for c, _ in full], [l for _, l in full])
        ref.add_partitions([c for c, _ in model], [l for _, l in model])
        assert got.remove_labels(removed) == gone
        check(got, model)
        assign, tables = ref.search_tables(queries, ma)
        for finish in (0, 1):
            got.set_finish(finish)
            ref.set_finish(finish)
            for x, y in zip(got.search(queries, ma, R), ref.search(queries, ma, R)):
                assert same_bits(x, y), "search differs, finish %d" % finish
            for x, y in zip(got.query_scan(assign, tables, R), ref.query_scan(assign, tables, R)):
                assert same_bits(x, y), "query_scan differs, finish %d" % finish
    finally:
        got.close()
        ref.close()


# ---- 6. the list in device memory ----------------------------------------------------------------------------------------------

@path_independent
@pytest.mark.parametrize("shape", [(16, 8, 32), (4, 16, 64)], ids=lambda s: "%dx%d-d%d" % s)
def test_remove_labels_device_equals_remove_labels(shape):
    import torch
    nsq, bits, dim = shape
    q = Quantizers(nsq, bits, dim, n=T + 900, seed=13)
    a, codes = q.encoded()
    full = group(a, codes, q.K)
    host, dev = q.index(), q.index()
    try:
        for idx in (host, dev):
            idx.add_partitions([c for c, _ in full], [l for _, l in full])
        keys, _, sizes = dev.search_device(torch.from_numpy(q.vectors[:6]).to("cuda:0"), 2, 50)   # "remove what this search returned"
        flat = keys.reshape(-1)
        removed = flat.cpu().numpy().view(np.uint32)
        model, gone = model_remove(full, removed)
        assert gone >= int(sizes.max().item()) > 0                               # a heap holds distinct rows
        assert dev.remove_labels_device(flat) == gone
        assert host.remove_labels(removed) == gone
        check(dev, model, "device list")
        check(host, model, "host list")
        assert dev.remove_labels_device(flat) == 0                               # they are gone
        check(dev, model)
    finally:
        host.close()
        dev.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

def refused(idx, code, match, f, *args):
    before = read_all(idx)
    with pytest.raises(pyqadc.QadcError, match=match) as e:
        f(*args)
    assert "qadc error %d:" % code in str(e.value)
    assert_partitions(read_all(idx), before, "after the refused call")


@path_independent
def test_refusals_leave_the_index_as_it_was():
    import torch
    q = Quantizers(8, 8, 64, n=300, seed=14)
    a, codes = q.encoded()
    some = np.arange(5, dtype=np.uint32)

    flat = q.index(coarse=False)                                                 # a flat index keys by position
    try:
        flat.add_vectors(q.vectors[:100])
        refused(flat, pyqadc.QADC_E_ARG, "by position", flat.remove_labels, some)
        refused(flat, pyqadc.QADC_E_ARG, "by position", flat.remove_labels_device, torch.arange(5, dtype=torch.int32, device="cuda:0"))
        assert flat.partition_size(0) == 100
    finally:
        flat.close()

    unl = q.index()                                                              # unlabelled add_partitions
    try:
        unl.add_partitions([codes[k:k + 3] for k in range(q.K)])
        refused(unl, pyqadc.QADC_E_ARG, "by position", unl.remove_labels, some)
    finally:
        unl.close()

    ivf = q.index()
    try:
        ivf.add_vectors(q.vectors)
        refused(ivf, pyqadc.QADC_E_ARG, "labels is null", ivf.remove_labels_raw, None, 3)
        before = read_all(ivf)
        for bad, exc in ((torch.arange(5, dtype=torch.int64, device="cuda:0"), TypeError),       # the wrong dtype
                         (torch.arange(5, dtype=torch.float32, device="cuda:0"), TypeError),
                         (some, TypeError),                                                       # no tensor at all
                         (torch.arange(5, dtype=torch.int32), pyqadc.QadcError),                  # the wrong device
                         (torch.zeros((5, 2), dtype=torch.int32, device="cuda:0"), pyqadc.QadcError),
                         (torch.zeros(10, dtype=torch.int32, device="cuda:0")[::2], pyqadc.QadcError)):
            with pytest.raises(exc):
                ivf.remove_labels_device(bad)
        assert_partitions(read_all(ivf), before)
        assert ivf.remove_labels_raw(None, 0) == 0                               # count 0 looks at no list
        assert ivf.remove_labels(some) == 5                                      # the good call
        assert_partitions(read_all(ivf), model_remove(group(a, codes, q.K), some)[0])
    finally:
        ivf.close()

    src = pyqadc.Index(16, 0)                                                    # a view owns no rows
    try:
        src.add_partitions([np.zeros((64, 8), np.uint8)], [np.arange(64, dtype=np.uint32)])
        src.finalize(0.01)
        view = pyqadc.AdcIndex.view_of(src)
        try:
            for f, args in ((view.remove_labels, (some,)), (view.remove_labels_device, (torch.arange(5, dtype=torch.int32, device="cuda:0"),))):
                with pytest.raises(pyqadc.QadcError, match="view") as e:
                    f(*args)
                assert "qadc error %d:" % pyqadc.QADC_E_ARG in str(e.value)
            assert view.partition_size(0) == 64
        finally:
            view.close()
        assert np.array_equal(src.read_partition(0)[1], np.arange(64, dtype=np.uint32))
    finally:
        src.close()
