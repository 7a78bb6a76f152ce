"""CPU: the host twin of the float-ADC feeders and the new C-ABI surface.

1. pq_bytes with the OPQ rotation under flat_database_t / ivf_database_t<pq_bytes> and nns_engine (host/scanner_simple.hpp,
   host/query_driver.hpp; driver tests/cpp/adc_feeders_host.cpp) against the composition of the oracle's functions
   (tests/adc_compose.py): assign, both table forms, codes and heaps, bit for bit.
2. every qadc_adc_* symbol include/qadc.h declares is exported by the library, and host/adc_search_hip.hpp compiles as C++14 with
   -Wall -Werror."""
import os
import re
import subprocess

import numpy as np
import pytest

import adc_compose as ac
from test_gpu_adc import expected
from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "adc_feeders_host")


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "adc_feeders_host.cpp"), EXE, link=False)
    return EXE


def run_driver(exe, tmp_path, nsq, dim, coarse, rotation, codebooks, queries, vectors, ma, R):
    K = 0 if coarse is None else len(coarse)
    nq, n = len(queries), len(vectors)
    fin, fout = str(tmp_path / "case.in"), str(tmp_path / "case.out")
    with open(fin, "wb") as f:
        np.array([nsq, dim, K, rotation is not None, nq, ma, n, R], np.int32).tofile(f)
        for a in (codebooks, rotation, coarse, queries, vectors):
            if a is not None:
                np.ascontiguousarray(a, np.float32).tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    td = nsq * 256
    with open(fout, "rb") as f:
        got = dict(
            part=np.fromfile(f, np.int32, n), codes=np.fromfile(f, np.uint8, n * nsq).reshape(n, nsq),
            assign=np.fromfile(f, np.int32, nq * ma).reshape(nq, ma),
            direct=np.fromfile(f, np.float32, nq * ma * td).reshape(nq, ma, td),
            expansion=np.fromfile(f, np.float32, nq * ma * td).reshape(nq, ma, td),
            sizes=np.fromfile(f, np.int32, nq), keys=np.fromfile(f, np.uint32, nq * R).reshape(nq, R),
            vals=np.fromfile(f, np.float32, nq * R).reshape(nq, R))
        assert f.read() == b""
    return got


@pytest.mark.parametrize("nsq", [4, 8, 16])
@pytest.mark.parametrize("sq_dim", [8, 16, 32, 12])
@pytest.mark.parametrize("opq", [False, True], ids=["pq", "opq"])
@pytest.mark.parametrize("ivf", [False, True], ids=["flat", "ivf"])
def test_host_twin_equals_the_composition(po, driver, tmp_path, nsq, sq_dim, opq, ivf):
    rng = np.random.default_rng(nsq * 1000 + sq_dim * 10 + 2 * opq + ivf)
    dim, K, nq, n, R = nsq * sq_dim, 16, 4, 1500, 50
    ma = 5 if ivf else (1 if opq else 3)                          # (flat: ma == 1 takes nns_engine's direct form)
    codebooks = rng.normal(size=(nsq, 256, sq_dim)).astype(np.float32)
    rotation = ac.random_rotation(rng, dim) if opq else None
    coarse = (rng.normal(size=(K, dim)) * 2).astype(np.float32) if ivf else None
    vectors = rng.normal(size=(n, dim)).astype(np.float32)
    queries = rng.normal(size=(nq, dim)).astype(np.float32)
    if ivf:
        vectors += coarse[rng.integers(0, K - 2, n)]              # (the last two partitions stay nearly empty)
        queries += coarse[rng.integers(0, K, nq)]
    got = run_driver(driver, tmp_path, nsq, dim, coarse, rotation, codebooks, queries, vectors, ma, R)

    want_part, want_codes = ac.encode(po, codebooks, vectors, coarse, rotation)
    assert np.array_equal(got["part"], np.zeros(n, np.int32) if want_part is None else want_part)
    assert np.array_equal(got["codes"], want_codes)
    a = ac.assign(po, queries, coarse, ma)
    assert np.array_equal(got["assign"], a)
    res = ac.residuals(queries, coarse, a, rotation)
    ac.pin_to_reference(po, codebooks, res.reshape(-1, dim)[:4])
    direct, expansion = ac.tables(po, codebooks, res, 0), ac.tables(po, codebooks, res, 1)
    assert np.array_equal(got["direct"].view(np.uint32), direct.view(np.uint32))
    assert np.array_equal(got["expansion"].view(np.uint32), expansion.view(np.uint32))
    if ivf:
        members = [np.flatnonzero(want_part == k) for k in range(K)]
        parts, labels = [want_codes[m] for m in members], [m.astype(np.uint32) for m in members]
    else:
        parts, labels = [want_codes], None
    used = direct if ma == 1 else expansion
    for q in range(nq):
        wk, wv = expected(po, nsq, [parts[k] for k in a[q]], None if labels is None else [labels[k] for k in a[q]], used[q], R)
        size = int(got["sizes"][q])
        assert size == len(wk)
        assert np.array_equal(got["keys"][q, :size], wk) and np.array_equal(got["vals"][q, :size].view(np.uint32), wv.view(np.uint32))


def test_host_twin_encoder_picks_like_the_compiled_heap_on_nan(po, driver, tmp_path):
    """a NaN centroid at index 0, inside and at 255, exact ties and duplicate centroids: pq_bytes::encode = the composition"""
    rng = np.random.default_rng(5)
    nsq, sq_dim, n = 8, 8, 400
    dim = nsq * sq_dim
    codebooks = rng.integers(-1, 2, (nsq, 256, sq_dim)).astype(np.float32)
    codebooks[:, 200:] = codebooks[:, :56]
    codebooks[0, 0, 0] = np.nan
    codebooks[1, 100, 3] = np.nan
    codebooks[2, 255, 7] = np.nan
    codebooks[3, [0, 63, 64, 191], 1] = np.nan
    vectors = rng.integers(-1, 2, (n, dim)).astype(np.float32)
    queries = rng.normal(size=(1, dim)).astype(np.float32)
    got = run_driver(driver, tmp_path, nsq, dim, None, None, codebooks, queries, vectors, 1, 5)
    with np.errstate(all="ignore"):
        _, want = ac.encode(po, codebooks, vectors)
    assert np.array_equal(got["codes"], want)
    assert (want[:, 2] == 255).all()


def test_library_exports_the_feeder_entry_points():
    import pyqadc
    hdr = open(os.path.join(ROOT, "include", "qadc.h")).read()
    declared = set(re.findall(r"\b(qadc_adc_[a-z0-9_]+)\s*\(", hdr))
    new = {"qadc_adc_index_set_pq", "qadc_adc_index_set_rotation", "qadc_adc_index_set_coarse", "qadc_adc_index_set_table_budget",
           "qadc_adc_search", "qadc_adc_search_candidates", "qadc_adc_search_tables", "qadc_adc_encode_host"}
    assert new <= declared, new - declared
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = pyqadc.lib()
    for s in declared:
        assert hasattr(lib, s), s
    for name in ("set_pq", "set_rotation", "set_coarse", "set_table_budget", "search", "search_candidates", "search_tables"):
        assert callable(getattr(pyqadc.AdcIndex, name))
    assert callable(pyqadc.adc_encode)


def test_search_engine_header_builds_as_cxx14(tmp_path):
    """host/adc_search_hip.hpp instantiated over both databases, driven by process_queries<>: C++14, -Wall -Werror"""
    src = tmp_path / "engine_builds.cpp"
    src.write_text('''
#include "%(root)s/quick-adc_amd/host/adc_search_hip.hpp"
#include "%(root)s/quick-adc_amd/host/scanner_simple.hpp"
using namespace qadc;
template <typename Db>
double drive(Db& db, const float* queries, int count, const unsigned* truth) {
    adc_search_engine_hip<Db> engine(db, 8, 32, 100);
    query_metrics m;
    double recall = 0;
    process_queries<adc_search_engine_hip<Db>, float_heap>(engine, queries, count, db.pq->dim, 100, truth, m, recall);
    return recall;
}
template double drive(flat_database_t<pq_bytes>&, const float*, int, const unsigned*);
template double drive(ivf_database_t<pq_bytes>&, const float*, int, const unsigned*);
int main() { return 0; }
''' % dict(root=ROOT))
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-fsyntax-only", str(src)])
