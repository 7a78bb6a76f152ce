"""GPU: the memory behaviour of the three new _device forms at the C-ABI, on guard-band arenas
(tests/guard_arena.py): qadc_pq_train_repair_device, qadc_pq_train16_repair_device and qadc_opq_train_repair_device with repair = 1.
d_vectors is their only device pointer, so the learning set is a window of an arena handed to pyqadc's *_device functions, which pass
its address on unchanged and allocate nothing on the device themselves.

W  no byte of the arena changes (the bands are intact and the vectors unchanged: the repair reads the learning set and writes only
the call's own codes and scratch); R  codebooks, codes, empty and repaired are bit-identical under the two guard poisons and equal
the host form's; A  d_vectors at the smallest alignment include/qadc.h states for the width (4 bytes; 16 for the 16-bit training:
its encoder loads 16 bytes), and at 256.  Every case has empty clusters to fill, and an n that is no multiple of a workgroup's tile."""
import numpy as np
import pytest

import guard_arena as ga
import pq_repair_compose as prc
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALIGNS = ["min", 256]


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


def named(names, values):
    return {k: np.asarray(v) for k, v in zip(names, values)}


def on_arena(vectors, minimum, align, run):
    def call(a):
        v = a.place(vectors, minimum if align == "min" else align, "in", name="d_vectors")
        a.snapshot()
        got = run(v)
        a.check_untouched([])
        return got
    return ga.under_both_poisons(call, backend="torch", capacity=vectors.nbytes + (1 << 20))


NAMES = ("codebooks", "codes", "empty", "repaired")
TRAIN = [(16, 4, 32, 1301), (4, 8, 8, 1301)]


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("nsq,bits,dim,n", TRAIN, ids=["%dx%d" % t[:2] for t in TRAIN])
def test_pq_train_repair_device(pyqadc, nsq, bits, dim, n, align):
    v, seed = prc.train_case(nsq, bits, dim, n, "repeated")
    want = named(NAMES, pyqadc.train_pq(v, seed, 2, repair=True))
    assert want["repaired"] > 0
    got = on_arena(v, 4, align, lambda t: named(NAMES, pyqadc.train_pq_device(t, seed, 2, repair=True)))
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
def test_pq_train16_repair_device(pyqadc, align):
    v, seed = prc.train_case(2, 16, 4, 1301, "repeated")
    want = named(NAMES, pyqadc.train_pq16(v, seed, 1, repair=True))
    assert want["repaired"] > 0
    got = on_arena(v, 16, align, lambda t: named(NAMES, pyqadc.train_pq16_device(t, seed, 1, repair=True)))
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)


@path_independent
@pytest.mark.parametrize("align", ALIGNS)
def test_opq_train_repair_device(pyqadc, align):
    v, seed = prc.train_case(8, 8, 16, 1301, "repeated")
    names = ("rotation", "codebooks", "codes", "empty", "rounds_done", "repaired")
    want = named(names, pyqadc.train_opq(v, seed, 1, 1, repair=True))
    assert want["repaired"] > 0
    got = on_arena(v, 4, align, lambda t: named(names, pyqadc.train_opq_device(t, seed, 1, 1, repair=True)))
    assert ga.same(got, want) is None, "%s differs from the host form" % ga.same(got, want)
