"""GPU: the empty-cluster repair alone (qadc_pq_repair_host; pyqadc.pq_repair; include/qadc.h "Empty-cluster repair", DESIGN.md
section 11.18) on crafted codes against the definition in numpy (tests/pq_repair_compose.py): codes and moved bit for bit.

Shapes, each at its smallest dim: 16x4 (dim 32), 32x4 (dim 64), 4x8 (dim 8), 16x8 (dim 16), 2x16 (dim 4), 8x16 (dim 16); n 1 (one
vector), 255 (under a workgroup's tile), 1025 (two workgroups of the row kernels), and 70000 (more vectors than 16-bit centroids,
several workgroups of the count kernel) for the 16-bit shapes and 4x8.  The patterns are prc.PATTERNS: every vector in one cluster
(E = K - 1 against n - 1 eligible: the "fewer eligible than E" branch at small n, the full one at large n), every cluster alive,
equal distances on an integer grid across the selection boundary, both nibbles of one byte rewritten at 4 bits, first and last
cluster empty, the farthest vector being its cluster's first, members at distance 0, rows with NaN and +-inf, a NaN centroid with
members."""
import numpy as np
import pytest

import pq_repair_compose as prc
import pyqadc
from helpers import path_independent

pytestmark = pytest.mark.gpu

CASES = [(s, n) for s in prc.SHAPES for n in (1, 255, 1025)] + [(s, 70000) for s in prc.SHAPES if s[1] == 16 or s == (4, 8, 8)]


@path_independent
@pytest.mark.parametrize("shape,n", CASES, ids=["%dx%d-d%d-n%d" % (s + (n,)) for s, n in CASES])
def test_crafted_codes_against_the_definition(shape, n):
    nsq, bits, dim = shape
    branches = set()
    for pattern in prc.PATTERNS:
        if pattern == "both_nibbles" and bits != 4:
            continue
        x, cb, codes = prc.crafted(pattern, nsq, bits, dim, n)
        want, want_moved = prc.repair(x, cb, codes)
        keep = codes.copy()
        got, moved = pyqadc.pq_repair(x, cb, codes)
        assert np.array_equal(codes, keep)                                  # the caller's codes are copied
        prc.same_codes(got, want, pattern)
        assert moved.dtype == np.uint32 and np.array_equal(moved, want_moved), (pattern, moved, want_moved)
        E = (prc.counts(codes, nsq, bits) == 0).sum(axis=1)
        branches |= {"fewer"} if (moved < E).any() else set()
        branches |= {"full"} if ((moved == E) & (E > 0)).any() else set()
        if pattern == "all_alive" and n >= 1 << bits:
            assert moved.sum() == 0 and np.array_equal(got, codes)          # every cluster alive: codes returned untouched
        if pattern == "both_nibbles" and n > 1:
            a, b = prc.unpack(codes, 4), prc.unpack(got, 4)
            assert ((a[:, 0::2] != b[:, 0::2]) & (a[:, 1::2] != b[:, 1::2])).any()
    assert ("fewer" if n < 1 << bits else "full") in branches


@path_independent
def test_the_same_call_twice_and_a_good_call_after_a_refused_one():
    x, cb, codes = prc.crafted("one_cluster", 4, 8, 8, 1025)
    first = pyqadc.pq_repair(x, cb, codes)
    with pytest.raises(pyqadc.QadcError, match="sq_count"):
        pyqadc.pq_repair(np.zeros((10, 6), np.float32), np.zeros((3, 256, 2), np.float32), np.zeros((10, 3), np.uint8))
    again = pyqadc.pq_repair(x, cb, codes)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    # a repaired set has no empty cluster left to fill where moved == E: repairing it again moves nothing
    E = (prc.counts(codes, 4, 8) == 0).sum(axis=1)
    assert (first[1] == E).all() and pyqadc.pq_repair(x, cb, first[0])[1].sum() == 0
