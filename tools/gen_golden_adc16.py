"""TEST INFRASTRUCTURE — generates tests/golden/ref_scan_standard_u16_cases.npz: the heaps the REFERENCE'S OWN
scanner_simple::query_scan leaves for the 16-bit code shapes (2,16) (4,16) (8,16), i.e. get_scan_func's
scan_standard<uint16_t, NSQ> as g++ compiles it with the reference's flags.

Runs only where the reference tree exists (REF, default /root/reference).  In a temporary directory, deleted afterwards:
  1. oracle/ref_extract.sh cuts the reference's line ranges (unchanged, sha256-checked);
  2. tools/adc16_ref_harness.cpp — the project's own text — is compiled with REF_FLAGS of oracle/Makefile against them;
  3. its one entry point drives get_scan_func + scanner_simple::query_scan for every case below.
The fixture holds data only: codes, labels, R, the reference's heap arrays and the compiler string.  A table [nsq][65536] is
stored sparse — per (probe, sub-quantizer) the centroid indices the probed partition's codes use, their values, and one fill
value for the entries no code reads (tests/adc16_compose.py expands them).

Cases, per shape: 1000 codes in two partitions (600 + 400), code values 0, 255, 256, 0xff00 and 0xffff in every column, a
third of the codes drawn from 8 values per column (equal candidates);
  tables "mixed"   mixed sign over 24 binades, some entries -0.0 (built from the bit pattern: the fast-math build folds the literal)
         "ties"    small integers of either sign and -0.0: ties everywhere
         "negzero" every entry -0.0: the candidate is -0.0 only without a leading "0 +"
  with and without labels, R in {1, 7, 100}.

    python tools/gen_golden_adc16.py
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference")
OUT = os.environ.get("QADC_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden", "ref_scan_standard_u16_cases.npz")
SPECIAL = np.array([0, 255, 256, 0xff00, 0xffff], np.uint16)
NEG_ZERO = np.array([0x80000000], np.uint32).view(np.float32)[0]
FILL = np.float32(1.0e30)


def ref_flags():
    """REF_FLAGS of oracle/Makefile, continuation lines joined"""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    return re.search(r"^REF_FLAGS\s*=\s*(.*)$", text, re.M).group(1).split()


def build_harness(tmp):
    subprocess.check_call([os.path.join(ROOT, "oracle", "ref_extract.sh"), REF, tmp])
    so = os.path.join(tmp, "libadc16_ref.so")
    subprocess.check_call(["g++"] + ref_flags() + ["-ffile-prefix-map=%s=ref_extract" % tmp, "-shared", "-fPIC", "-I" + tmp, "-I" + REF,
                                                   os.path.join(ROOT, "tools", "adc16_ref_harness.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.adc16_ref_compiler.restype = C.c_char_p
    return lib


def ref_query_scan(lib, nsq, parts, labels, tables, R):
    u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    parts = [np.ascontiguousarray(p, "<u2") for p in parts]
    pa = (u8p * len(parts))(*[p.ctypes.data_as(u8p) for p in parts])
    la = None
    if labels is not None:
        labels = [np.ascontiguousarray(l, np.uint32) for l in labels]
        la = (u32p * len(labels))(*[l.ctypes.data_as(u32p) for l in labels])
    sizes = np.array([len(p) for p in parts], np.uint32)
    tb = np.ascontiguousarray(tables, np.float32).copy()
    keys, vals, size = np.zeros(R, np.uint32), np.zeros(R, np.float32), C.c_int(0)
    rc = lib.adc16_ref_query_scan(nsq, len(parts), pa, la, sizes.ctypes.data_as(u32p), tb.ctypes.data_as(C.POINTER(C.c_float)), R,
                                  keys.ctypes.data_as(u32p), vals.ctypes.data_as(C.POINTER(C.c_float)), C.byref(size))
    assert rc == 0 and size.value == R, (rc, size.value)
    return keys, vals


def make_codes(rng, n, nsq):
    codes = rng.integers(0, 65536, (n, nsq)).astype(np.uint16)
    pool = rng.integers(0, 65536, (8, nsq)).astype(np.uint16)
    few = rng.random(n) < 1 / 3
    pick = rng.integers(0, 8, (n, nsq))
    codes[few] = pool[pick, np.arange(nsq)][few]
    for i in range(5):
        codes[i, :] = SPECIAL[i]                                         # every column reads every special value
        codes[5 + i, :] = SPECIAL[(i + np.arange(nsq)) % 5]              # and mixes of them within one code
    return codes


def make_values(rng, kind, count):
    if kind == "mixed":
        v = (rng.normal(size=count) * np.exp2(rng.integers(-12, 12, count))).astype(np.float32)
        v[rng.random(count) < 0.02] = NEG_ZERO
    elif kind == "ties":
        v = rng.integers(-1, 3, count).astype(np.float32)
        v[rng.random(count) < 0.1] = NEG_ZERO
    elif kind == "negzero":
        v = np.full(count, NEG_ZERO, np.float32)
    else:
        raise ValueError(kind)
    return v


def main():
    assert os.path.isdir(REF), "the reference tree %s is not here" % REF
    tmp = tempfile.mkdtemp()
    try:
        lib = build_harness(tmp)
        rng = np.random.default_rng(2016)
        d, cases = {"compiler": np.array(lib.adc16_ref_compiler().decode()), "fill": FILL}, []
        for nsq in (2, 4, 8):
            parts = [make_codes(rng, 600, nsq), make_codes(rng, 400, nsq)]
            perm = (rng.permutation(1000) + 7).astype(np.uint32)
            labels = [perm[:600].copy(), perm[600:].copy()]
            for p in range(2):
                d["s%d_codes%d" % (nsq, p)] = parts[p]
                d["s%d_labels%d" % (nsq, p)] = labels[p]
            for kind in ("mixed", "ties", "negzero"):
                tid = "s%d_%s" % (nsq, kind)
                full = np.full((2, nsq, 65536), FILL, np.float32)
                idx, val, off = [], [], [0]
                for a in range(2):
                    for m in range(nsq):
                        used = np.unique(parts[a][:, m])
                        v = make_values(rng, kind, len(used))
                        full[a, m, used] = v
                        idx.append(used.astype(np.uint16))
                        val.append(v)
                        off.append(off[-1] + len(used))
                d[tid + "_idx"], d[tid + "_val"], d[tid + "_off"] = np.concatenate(idx), np.concatenate(val), np.array(off, np.int32)
                for labelled in (0, 1):
                    for R in (1, 7, 100):
                        cid = "c%02d" % len(cases)
                        keys, vals = ref_query_scan(lib, nsq, parts, labels if labelled else None, full.reshape(2, -1), R)
                        d[cid + "_keys"], d[cid + "_vals"] = keys, vals
                        cases.append((cid, nsq, kind, labelled, R))
        d["case_ids"] = np.array([c[0] for c in cases])
        d["case_kind"] = np.array([c[2] for c in cases])
        d["case_meta"] = np.array([(c[1], c[3], c[4]) for c in cases], np.int64)   # nsq, labelled, R
        np.savez_compressed(OUT, **d)
        print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases,", str(d["compiler"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
