"""The 16-bit encoder's entry point without a GPU: qadc_adc_encode16_host is declared, exported and bound, and refuses bad
arguments with QADC_E_ARG before it touches a device.  What it computes: tests/test_gpu_adc16_encode.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pyqadc():
    import pyqadc
    if not os.path.exists(pyqadc.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    pyqadc.lib()
    return pyqadc


def test_the_header_declares_and_the_library_exports_the_call(pyqadc):
    hdr = open(os.path.join(ROOT, "include", "qadc.h")).read()
    assert re.search(r"\bint\s+qadc_adc_encode16_host\s*\(", hdr)
    assert re.search(r"#define\s+QADC_ADC_ENCODE16_CHUNK\s+262144\b", hdr)
    assert hasattr(pyqadc.lib(), "qadc_adc_encode16_host")
    assert "qadc_adc_encode16_host" in pyqadc.SYMBOLS
    assert callable(pyqadc.adc_encode16)
    assert pyqadc.QADC_ADC_ENCODE16_CHUNK == 262144


def call(pyqadc, sq_count, dim, codebooks=True, K=0, coarse=False, sum_mode=1, n=2):
    """The raw call on small host buffers (a refused call reads none of them) -> (return code, message)"""
    f32p = C.POINTER(C.c_float)
    cb = np.zeros(16, np.float32)
    co = np.zeros(max(1, K) * max(1, dim), np.float32)
    v = np.zeros(n * max(1, dim), np.float32)
    codes = np.zeros(n * 2 * max(1, sq_count), np.uint8)
    assign = np.zeros(n, np.int32)
    L = pyqadc.lib()
    rc = L.qadc_adc_encode16_host(sq_count, dim, cb.ctypes.data_as(f32p) if codebooks else None, None, K,
                                  co.ctypes.data_as(f32p) if coarse else None, v.ctypes.data_as(f32p), n, sum_mode,
                                  assign.ctypes.data_as(C.POINTER(C.c_int32)), codes.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
    return rc, L.qadc_last_error().decode()


@pytest.mark.parametrize("kwargs", [
    dict(sq_count=3, dim=48), dict(sq_count=16, dim=64), dict(sq_count=4, dim=18), dict(sq_count=2, dim=4098),
    dict(sq_count=2, dim=16, codebooks=False), dict(sq_count=2, dim=16, K=8, coarse=False), dict(sq_count=2, dim=16, sum_mode=2),
], ids=["sq_count-3", "sq_count-16", "dim-not-a-multiple", "dim-over-4096", "null-codebooks", "K-without-coarse", "sum_mode-2"])
def test_refusals_need_no_gpu(pyqadc, kwargs):
    rc, msg = call(pyqadc, **kwargs)
    assert rc == pyqadc.QADC_E_ARG, (rc, msg)
    assert "2, 4 or 8" in msg


def test_the_8_bit_call_still_refuses_two_sub_quantizers(pyqadc):
    f32p = C.POINTER(C.c_float)
    z = np.zeros(64, np.float32)
    codes = np.zeros(16, np.uint8)
    rc = pyqadc.lib().qadc_adc_encode_host(2, 16, z.ctypes.data_as(f32p), None, 0, None, z.ctypes.data_as(f32p), 2, 1, None,
                                           codes.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
    assert rc == pyqadc.QADC_E_ARG
