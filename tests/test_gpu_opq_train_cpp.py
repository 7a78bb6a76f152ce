"""Learning an OPQ rotation from C++14 (quick-adc_amd/host/db_build.hpp: learn_opq_hip; tests/cpp/opq_train_demo.cpp): the .opq.data
file the demo writes from a small .fvecs learning set holds the header dim, m, b, the codebooks and the rotation pyqadc.train_opq
returns for the same learning set and seed, and reads back through pq_from_data_file."""
import os
import struct
import subprocess

import numpy as np
import pytest

import adc_compose as ac
import io_formats as iof
import opq_compose as oc
import pq_train_compose as ptc
from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "cpp", "opq_train_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(DEMO + ".cpp", DEMO)
    return DEMO


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("nsq,bits,dim,n", [(16, 4, 32, 1000), (8, 8, 32, 3000)], ids=["16x4", "8x8"])
def test_learn_opq_hip_writes_the_quantizer_file(demo, tmp_path, nsq, bits, dim, n):
    import pyqadc
    outer, inner = 3, 2
    rng = np.random.default_rng(nsq)
    v = np.ascontiguousarray((rng.normal(size=(n, dim)) * 0.9 ** np.arange(dim)).astype(np.float32) @ ac.random_rotation(rng, dim), np.float32)
    learn, out, back = (str(tmp_path / name) for name in ("learn.fvecs", "learned.opq.data", "readback.bin"))
    iof.write_vecs(learn, v)
    run = subprocess.run([demo, learn, str(nsq), str(bits), str(outer), str(inner), out, back], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    rot, cb, _, empty, done = pyqadc.train_opq(v, ptc.seed_rows(v, nsq, bits, range(1 << bits)), outer, inner)
    assert done == outer and oc.orthogonality(rot) <= 2.0 ** -22 and not np.array_equal(rot, np.eye(dim, dtype=np.float32))
    assert run.stdout.decode().strip() == "opq dim=%d m=%d b=%d n=%d empty=%d rounds=%d" % (dim, nsq, bits, n, empty, done)
    raw = open(out, "rb").read()
    assert struct.unpack("<iii", raw[:12]) == (dim, nsq, bits) and len(raw) == 12 + 4 * cb.size + 4 * dim * dim
    ac.assert_same_floats(np.frombuffer(raw[12:12 + 4 * cb.size], np.float32).reshape(cb.shape), cb, "the file's codebooks")
    ac.assert_same_floats(np.frombuffer(raw[12 + 4 * cb.size:], np.float32).reshape(dim, dim), rot, "the file's rotation")
    rb = np.fromfile(back, np.float32)
    ac.assert_same_floats(rb[:cb.size].reshape(cb.shape), cb, "read back through pq_from_data_file")
    ac.assert_same_floats(rb[cb.size:].reshape(dim, dim), rot, "the rotation read back")
