"""GPU: the stateless PQ decoder, qadc_pq_decode_host / _device (include/qadc.h "Reconstruction"), bit for
bit against the CPU twin (quick-adc_amd/host/pq_decode.hpp through tests/cpp/pq_decode_host.cpp): every (sq_count, sq_bits) pair,
with and without rotation and coarse quantizer, host and device forms, the row counts around a wavefront and a pass, sub-vector
sizes 1, 3 and 8, dims that are no multiple of the rotation tile, the largest dim, both sides of the LDS threshold, NaN and infinite
centroids, missing rows, and the error chain (exactly 0 on the exactness fixtures)."""
import numpy as np
import pytest

import pq_decode_compose as pdc
from helpers import path_independent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    return pyqadc


@pytest.fixture(scope="module")
def driver():
    return pdc.build_driver()


def on_device(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.astype("<u2").view(np.uint8).reshape(a.shape[0], 2 * a.shape[1])         # the little-endian bytes
    return torch.from_numpy(a).cuda()


def decode_host(pyqadc, c, err=True):
    return pyqadc.pq_decode(c["cb"], c["codes"], assign=c["assign"], coarse=c["coarse"], rotation=c["rotation"],
                            vectors=c["vectors"] if err else None)


def decode_device(pyqadc, c, err=True):
    got = pyqadc.pq_decode_device(c["cb"], on_device(c["codes"]), assign=on_device(c["assign"]), coarse=c["coarse"], rotation=c["rotation"],
                                  vectors=on_device(c["vectors"]) if err else None)
    return tuple(t.cpu().numpy() for t in got) if err else got.cpu().numpy()


def check(pyqadc, driver, tmp_path, c, what, forms=("host", "device")):
    want = pdc.twin(driver, tmp_path, c["cb"], c["codes"], c["assign"], c["coarse"], c["rotation"], c["vectors"])
    for form in forms:
        got = (decode_host if form == "host" else decode_device)(pyqadc, c)
        pdc.same_floats(got[0], want[0], "%s, %s form: out" % (what, form))
        pdc.same_floats(got[1], want[1], "%s, %s form: err" % (what, form))
    return want


DSUB = {(16, 4): 1, (32, 4): 3, (4, 8): 8, (8, 8): 3, (16, 8): 1, (2, 16): 8, (4, 16): 3, (8, 16): 1}


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("K", [0, 5], ids=["flat", "ivf"])
@pytest.mark.parametrize("nsq,bits", pdc.PAIRS, ids=[pdc.pair_id(p) for p in pdc.PAIRS])
def test_every_pair(pyqadc, driver, tmp_path, nsq, bits, K, rotated):
    rng = np.random.default_rng(100 * nsq + bits + K)
    c = pdc.random_case(rng, nsq, bits, nsq * DSUB[nsq, bits], 65, K, rotated)
    if K:
        c["assign"][[0, 33, 64]] = (-1, K, 1 << 30)                         # outside [0, K): missing rows, not a refusal
    want = check(pyqadc, driver, tmp_path, c, "%dx%d" % (nsq, bits))
    if K:
        assert (want[0][[0, 33, 64]].view(np.uint32) == pdc.NAN_BITS).all()
    out_only = decode_device(pyqadc, c, err=False)                           # without vectors and err_out
    pdc.same_floats(out_only, want[0], "no err_out")


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_row_counts(pyqadc, driver, tmp_path, n, rotated):
    for nsq, bits, dim in ((16, 4, 16), (8, 8, 24), (2, 16, 6)):
        c = pdc.random_case(np.random.default_rng(n + bits), nsq, bits, dim, n, 3, rotated)
        got = check(pyqadc, driver, tmp_path, c, "n = %d" % n)
        assert got[0].shape == (n, dim) and got[1].shape == (n,)


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
def test_one_pass_and_one_row(pyqadc, driver, tmp_path, rotated):
    """QADC_DECODE_CHUNK + 1 rows: the second pass holds one row, and its output starts off a 16-byte boundary when dim is odd"""
    n = pdc.CHUNK + 1
    nsq, bits, dim = (16, 4, 16) if rotated else (4, 8, 12)
    c = pdc.random_case(np.random.default_rng(5), nsq, bits, dim, n, 2, rotated)
    check(pyqadc, driver, tmp_path, c, "one pass + 1", forms=("device",) if rotated else ("host", "device"))


@path_independent
@pytest.mark.parametrize("nsq,bits,dim,n", [(2, 16, 24, 70), (4, 8, 100, 70), (4, 8, 4096, 3), (16, 4, 2048, 3)],
                         ids=["dim24", "dim100", "dim4096", "dim2048-4bit"])
def test_rotation_tile_edges_and_the_largest_dims(pyqadc, driver, tmp_path, nsq, bits, dim, n):
    rng = np.random.default_rng(dim)
    c = pdc.random_case(rng, nsq, bits, dim, n, 3, rotated=dim <= 100)
    if dim > 100:                                                           # any matrix is this chain: no QR of a 4096 x 4096 matrix
        c["rotation"] = (rng.normal(size=(dim, dim)) / np.sqrt(dim)).astype(np.float32)
    check(pyqadc, driver, tmp_path, c, "dim %d" % dim, forms=("device",))
    c["rotation"] = None
    check(pyqadc, driver, tmp_path, c, "dim %d, plain" % dim, forms=("device",))


@path_independent
@pytest.mark.parametrize("nsq,bits,dim", [(16, 4, 1008), (16, 4, 1024), (4, 8, 60), (4, 8, 64), (16, 8, 48), (16, 8, 64)])
def test_lds_threshold_from_both_sides(pyqadc, driver, tmp_path, nsq, bits, dim):
    """the codebooks staged in LDS (1008, 60, 48) and read through the L2 (1024, 64, 64): tests/test_pq_decode_plan_host.py pins which"""
    c = pdc.random_case(np.random.default_rng(dim), nsq, bits, dim, 300, 4, False)
    check(pyqadc, driver, tmp_path, c, "dim %d" % dim)
    c["coarse"] = c["assign"] = None
    check(pyqadc, driver, tmp_path, c, "dim %d, flat" % dim, forms=("device",))


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("nsq,bits,dim", [(16, 4, 32), (4, 8, 12), (2, 16, 8)])
def test_nonfinite_centroids(pyqadc, driver, tmp_path, nsq, bits, dim, rotated):
    rng = np.random.default_rng(bits)
    c = pdc.random_case(rng, nsq, bits, dim, 90, 3, rotated)
    a = pdc.unpack(c["codes"], bits)
    a[[2, 5, 9], 1] = (10, 11, 12)
    c["codes"] = pdc.pack(a, bits)
    for code, val in ((10, np.nan), (11, np.inf), (12, -np.inf)):
        c["cb"][1, code, 0] = val
    c["cb"][0, a[40, 0], :] = np.float32(3e38)                              # overflows in the chains
    want = check(pyqadc, driver, tmp_path, c, "non-finite centroids")         # bit for bit: a NaN made by arithmetic is 0x7FC00000
    nan = np.isnan(want[0])
    assert (want[0].view(np.uint32)[nan] == pdc.NAN_BITS).all() and nan.any()
    c["coarse"] = c["assign"] = None
    flat = check(pyqadc, driver, tmp_path, c, "non-finite centroids, flat")
    if not rotated:                                                         # a copy keeps the centroid's bits, NaN payload included
        c["cb"][1, 10, 0] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
        kept = check(pyqadc, driver, tmp_path, c, "a NaN payload copied")[0]
        assert kept.view(np.uint32)[2, dim // nsq] == 0x7FC12345
    ds = dim // nsq
    if rotated:
        assert np.isnan(want[0][2]).all()                                   # one NaN component of y: the whole row
    else:
        assert np.isnan(want[0][2]).sum() == 1 and np.isposinf(want[0][5, ds]) and np.isneginf(want[0][9, ds])


EXACT = [(16, 4, 32), (32, 4, 32), (4, 8, 8), (8, 8, 16), (16, 8, 32), (2, 16, 4), (2, 16, 8)]


@path_independent
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("K", [0, 6], ids=["flat", "ivf"])
@pytest.mark.parametrize("nsq,bits,dim", EXACT, ids=["%dx%d-dim%d" % s for s in EXACT])
def test_exactness_fixtures(pyqadc, driver, tmp_path, nsq, bits, dim, K, rotated):
    """decode(encode(x)) == x with the library's own encoders, encode(decode(codes)) == codes, and err == +0.0 exactly"""
    fx = pdc.exact_fixture(nsq, bits, dim, K, rotated)
    codes, assign = pdc.exact_rows(fx, 200)
    c = dict(cb=fx["cb"], codes=codes, assign=assign, coarse=fx["coarse"], rotation=fx["rotation"], vectors=None)
    x = decode_device(pyqadc, c, err=False)
    pdc.same_floats(x, pdc.twin(driver, tmp_path, fx["cb"], codes, assign, fx["coarse"], fx["rotation"]), "decode")
    if bits == 4:
        got_assign, got_codes = pyqadc.ivf_encode(fx["cb"], x, coarse=fx["coarse"], rotation=fx["rotation"])
    else:
        got_assign, got_codes = (pyqadc.adc_encode if bits == 8 else pyqadc.adc_encode16)(fx["cb"], x, coarse=fx["coarse"], rotation=fx["rotation"])
    assert np.array_equal(np.asarray(got_codes).view(np.uint8), np.asarray(codes).view(np.uint8)), "encode(decode(codes)) != codes"
    if K:
        assert np.array_equal(got_assign, assign)
    c.update(codes=got_codes, assign=got_assign if K else None, vectors=x)
    for got in (decode_host(pyqadc, c), decode_device(pyqadc, c)):
        pdc.same_floats(got[0], x, "decode(encode(x))")
        assert (got[1].view(np.uint32) == 0).all()
    err, total = pyqadc.quant_error(x, c["assign"], got_codes, fx["cb"], coarse=fx["coarse"], rotation=fx["rotation"])
    assert (err.view(np.uint32) == 0).all() and total == 0.0 and isinstance(total, np.float64)


@path_independent
def test_quant_error_sums_in_float64_in_row_order(pyqadc, driver, tmp_path):
    c = pdc.random_case(np.random.default_rng(8), 8, 8, 64, 1000, 4, True)
    want = pdc.twin(driver, tmp_path, c["cb"], c["codes"], c["assign"], c["coarse"], c["rotation"], c["vectors"])[1]
    err, total = pyqadc.quant_error(c["vectors"], c["assign"], c["codes"], c["cb"], coarse=c["coarse"], rotation=c["rotation"])
    pdc.same_floats(err, want, "err")
    acc = 0.0
    for e in want:
        acc += float(e)
    assert total == acc and total > 0
