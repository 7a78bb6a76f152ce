"""Learning a product quantizer of 16-bit sub-quantizers from C++14 (quick-adc_amd/host/db_build.hpp: learn_pq_hip routes sq_bits 16
to qadc_pq_train16_host; tests/cpp/pq_train_demo.cpp as it is): the .pq.data file the demo writes from a .fvecs learning set holds
the header dim, m, 16 and, read back through pq_from_data_file, the codebooks pyqadc.train_pq16 returns for the same learning set
and seed."""
import os
import struct
import subprocess

import numpy as np
import pytest

import adc_compose as ac
import io_formats as iof
import pq_train16_compose as p16
from helpers import path_independent
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "cpp", "pq_train_demo")


@pytest.fixture(scope="module")
def demo():
    _compile(DEMO + ".cpp", DEMO)
    return DEMO


@pytest.mark.gpu
@path_independent
@pytest.mark.parametrize("nsq,dim,n", [(2, 8, 66000), (8, 16, 65536)], ids=["2x16", "8x16"])
def test_learn_pq_hip_writes_a_16_bit_quantizer_file(demo, tmp_path, nsq, dim, n):
    import pyqadc
    iters = 2
    v = np.random.default_rng(nsq).normal(size=(n, dim)).astype(np.float32)
    learn, out, back = (str(tmp_path / name) for name in ("learn.fvecs", "learned.pq.data", "readback.bin"))
    iof.write_vecs(learn, v)
    run = subprocess.run([demo, learn, str(nsq), "16", str(iters), out, back], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    want_cb, _, empty = pyqadc.train_pq16(v, p16.seed_rows(v, nsq, range(65536)), iters)
    assert run.stdout.decode().strip() == "pq dim=%d m=%d b=16 n=%d empty=%d" % (dim, nsq, n, empty)
    raw = open(out, "rb").read()
    assert struct.unpack("<iii", raw[:12]) == (dim, nsq, 16) and len(raw) == 12 + 4 * want_cb.size
    ac.assert_same_floats(np.frombuffer(raw[12:], np.float32).reshape(want_cb.shape), want_cb, "the file's codebooks")
    ac.assert_same_floats(np.fromfile(back, np.float32).reshape(want_cb.shape), want_cb, "read back through pq_from_data_file")
