"""GPU: the learning calls started from k-means++ seeding.  train_pq, train_pq16 and kmeans_iterations from
pyqadc.kmeans_seed equal the twin chain bit for bit — the seed of the CPU twin (tests/kmeans_seed_compose.py), then the rounds as
the trainers' own tests compose them; the Python wrappers' shapes and errors; and the C++ route (tests/cpp/kmeans_seed_demo.cpp:
learn_coarse_quantizer_hip and learn_pq_hip with a 64-bit seed), whose .pq.data reads back through host/qadc_io.hpp with the Python
route's codebooks."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import adc_compose as ac
import io_formats as iof
import kmeans_seed_compose as ks
import pq_train16_compose as p16
import pq_train_compose as ptc
from helpers import path_independent
from test_scanner_hip_cpp import _compile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "cpp", "kmeans_seed_demo")


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def driver():
    return ks.build_driver()


@path_independent
def test_train_pq_from_the_seed(pyqadc, po, driver, tmp_path):
    v = ks.real_set(700, 16)
    twin_seed = ks.twin(driver, tmp_path, v, 256, 8, seed=5)[0]
    seed = pyqadc.pq_seed_pp(v, 8, 8, 5)
    assert seed.shape == (8, 256, 2)
    ac.assert_same_floats(seed, twin_seed, "the seed")
    want_cb, want_codes, _ = ptc.train(po, v, twin_seed, 2)
    cb, codes, empty = pyqadc.train_pq(v, seed, 2)
    assert np.array_equal(codes, want_codes) and empty == ptc.empty_count(want_cb)
    ac.assert_same_floats(cb, want_cb, "codebooks after two rounds from the seed")


@path_independent
def test_train_pq16_from_the_seed(pyqadc):
    """65536 centres per sub-space: the k = 65536 case, whose twin rows are recorded (kmeans_seed_compose.record_big); a round is then
    the encoder's codes under the seed and the compose update of those codes, as tests/test_gpu_pq_train16.py checks rounds."""
    with open(ks.BIG_GOLDEN) as f:
        golden = json.load(f)
    v = ks.big_set()
    seed, rows, fallbacks = pyqadc.pq_seed_pp(v, 2, 16, ks.BIG["seed"], return_rows=True)
    assert seed.shape == (2, 65536, 2) and ks.rows_digest(rows) == golden["rows_sha256"] and fallbacks == golden["fallbacks"]
    ks.check_centres(v, seed, rows, 2)
    cb, codes, empty = pyqadc.train_pq16(v, seed, 1)
    assert np.array_equal(codes, pyqadc.adc_encode16(seed, v)[1])
    ac.assert_same_floats(cb, p16.update(v, codes)[0], "codebooks after a round from the seed")
    assert empty == p16.empty_count(cb)


@path_independent
def test_kmeans_iterations_from_the_seed(pyqadc, po, driver, tmp_path):
    v = ks.real_set(900, 12)
    K = 10
    twin_seed = ks.twin(driver, tmp_path, v, K, 1, seed=8)[0][0]
    seed = pyqadc.kmeans_seed(v, K, seed=8)
    assert seed.shape == (K, 12)
    ac.assert_same_floats(seed, twin_seed, "the seed")
    want = twin_seed.copy()
    for _ in range(3):
        assign = ptc.assign_slice(po, want, v)
        want = ptc.update_slice(v, assign, K)
    cen, got_assign = pyqadc.kmeans_iterations(v, seed, 3)
    assert np.array_equal(got_assign, assign)
    ac.assert_same_floats(cen, want, "centroids after three rounds from the seed")


@path_independent
def test_wrapper_shapes_and_errors(pyqadc):
    v = ks.real_set(300, 12)
    assert pyqadc.kmeans_seed(v, 5).shape == (5, 12)
    c, rows, fallbacks = pyqadc.kmeans_seed(v, 5, seed=3, return_rows=True)
    assert c.shape == (5, 12) and rows.shape == (5,) and rows.dtype == np.uint32 and fallbacks == 0
    assert np.array_equal(c, v[rows.astype(np.int64)])
    c, rows, _ = pyqadc.kmeans_seed(v, 5, sq_count=3, seed=3, return_rows=True)
    assert c.shape == (3, 5, 4) and c.dtype == np.float32 and rows.shape == (3, 5)
    assert pyqadc.pq_seed_pp(v, 3, 4, 3).shape == (3, 16, 4) and pyqadc.pq_seed_pp(v, 1, 4, 3).shape == (1, 16, 12)
    assert np.array_equal(pyqadc.pq_seed_pp(v, 3, 4, 3), pyqadc.kmeans_seed(v, 16, sq_count=3, seed=3))
    assert pyqadc.kmeans_seed(v.astype(np.float64), 5, seed=3).dtype == np.float32             # converted like the trainers' input
    with pytest.raises(pyqadc.QadcError, match="1 <= k <= n"):
        pyqadc.kmeans_seed(v, 301)
    with pytest.raises(pyqadc.QadcError, match="multiple of sq_count"):
        pyqadc.kmeans_seed(v, 5, sq_count=5)
    with pytest.raises(pyqadc.QadcError, match="dim must be <= 4096"):
        pyqadc.kmeans_seed(np.zeros((4, 4100), np.float32), 2)
    with pytest.raises(pyqadc.QadcError, match="seed must be"):
        pyqadc.kmeans_seed(v, 5, seed=1.5)
    assert pyqadc.kmeans_seed(v, 5).shape == (5, 12)                                           # the refusals left nothing behind


@pytest.fixture(scope="module")
def demo():
    _compile(DEMO + ".cpp", DEMO)
    return DEMO


@path_independent
def test_the_cpp_route_writes_the_python_routes_quantizers(pyqadc, demo, tmp_path):
    n, dim, K, nsq, bits, iters, seed = 1500, 16, 6, 8, 8, 2, 77
    v = ks.real_set(n, dim)
    learn, out, back = (str(tmp_path / name) for name in ("learn.fvecs", "learned.pq.data", "readback.bin"))
    iof.write_vecs(learn, v)
    run = subprocess.run([demo, learn, str(K), str(nsq), str(bits), str(iters), str(seed), out, back], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    coarse, _ = pyqadc.kmeans_iterations(v, pyqadc.kmeans_seed(v, K, seed=seed), 48)           # kmeans_iter_max - 2
    cb, _, empty = pyqadc.train_pq(v, pyqadc.pq_seed_pp(v, nsq, bits, seed, coarse=coarse), iters, coarse=coarse)
    assert run.stdout.decode().strip() == "seeded dim=%d K=%d m=%d b=%d n=%d empty=%d" % (dim, K, nsq, bits, n, empty)
    raw = open(out, "rb").read()
    assert struct.unpack("<iii", raw[:12]) == (dim, nsq, bits) and len(raw) == 12 + 4 * cb.size
    ac.assert_same_floats(np.frombuffer(raw[12:], np.float32).reshape(cb.shape), cb, "the file's codebooks")
    rb = np.fromfile(back, np.float32)
    ac.assert_same_floats(rb[:K * dim].reshape(K, dim), coarse, "the coarse quantizer")
    ac.assert_same_floats(rb[K * dim:].reshape(cb.shape), cb, "read back through pq_from_data_file")
