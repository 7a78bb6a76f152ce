"""What the float-ADC engine must return on 16-bit codes (pyqadc.AdcIndex.create16, qadc_adc_index_create16): the heap arrays of
scanner_simple::query_scan over scan_standard<uint16_t, NSQ>, composed in three steps —
  1. numpy gathers t[n][NSQ] = table[m][code[m]];
  2. the NSQ entries are added in float32 in the grouping of the sum mode (1: as the reference compiles — NSQ 2 t0 + t1, NSQ 4
     (t1+t2) + (t3+t0), NSQ 8 ((t1+t2)+(t3+t4)) + ((t5+t6)+(t7+t0)); 0: source order from +0);
  3. the R sentinels (0, FLT_MAX) and then every (key, candidate) in scan order go through the reference's own kv_binheap
     (po.ref_heap_replay_f32; the oracle's restatement where that build is absent), whose push rejects !(v < max) itself.
The grouping of step 2 is pinned to the reference's text as compiled by tests/golden/ref_scan_standard_u16_cases.npz
(tools/gen_golden_adc16.py), which fixture() loads; tests/test_adc16_host.py holds this helper to it.
tables_expansion / tables_direct: the tables [nsq][65536] the feeders must build, tests/adc_compose.py's steps with 65536-row
codebooks."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_scan_standard_u16_cases.npz")
FLT_MAX = np.float32(np.finfo(np.float32).max)
SPECIAL = (0, 255, 256, 0xff00, 0xffff)


def gather(nsq, codes, table):
    """codes uint16 [n][nsq], table [nsq*65536] -> t float32 [n][nsq]"""
    codes = np.asarray(codes, np.uint16).reshape(-1, nsq)
    return np.asarray(table, np.float32).reshape(nsq, 65536)[np.arange(nsq), codes]


def candidates(nsq, codes, table, sum_mode=1):
    """-> float32 [n]: every code's candidate, each add rounded to float32"""
    t = gather(nsq, codes, table)
    with np.errstate(all="ignore"):
        if sum_mode == 0:
            s = np.zeros(len(t), np.float32)
            for m in range(nsq):
                s = s + t[:, m]
            return s
        if nsq == 2:
            return t[:, 0] + t[:, 1]
        if nsq == 4:
            return (t[:, 1] + t[:, 2]) + (t[:, 3] + t[:, 0])
        assert nsq == 8
        return ((t[:, 1] + t[:, 2]) + (t[:, 3] + t[:, 4])) + ((t[:, 5] + t[:, 6]) + (t[:, 7] + t[:, 0]))


def stream(nsq, parts, labels, tables, sum_mode=1):
    """The (key, candidate) pairs of one query in scan order: parts / labels = the probed partitions in assign order (labels None,
    or per partition None: key = position), tables [ma][nsq*65536].  NaN candidates are left out: scan_standard's own test
    `candidate < min` never passes them on to the heap."""
    tables = np.asarray(tables, np.float32).reshape(len(parts), nsq * 65536)
    keys, vals = [], []
    for a, p in enumerate(parts):
        v = candidates(nsq, p, tables[a], sum_mode)
        lab = None if labels is None else labels[a]
        k = np.arange(len(v), dtype=np.uint32) if lab is None else np.asarray(lab, np.uint32)
        ok = ~np.isnan(v)
        keys.append(k[ok])
        vals.append(v[ok])
    return np.concatenate(keys), np.concatenate(vals)


def replay(po, keys, vals, R):
    f = po.ref_heap_replay_f32 if po.have_ref() else po.heap_replay_f32
    return f(np.concatenate([np.zeros(R, np.uint32), keys]), np.concatenate([np.full(R, FLT_MAX, np.float32), vals]), R)


def heap(po, nsq, parts, labels, tables, R, sum_mode=1):
    """-> (keys, values): the heap arrays of one query"""
    k, v = stream(nsq, parts, labels, tables, sum_mode)
    return replay(po, k, v, R)


def tables_expansion(po, codebooks, x, sum_mode):
    """x [n][dim] -> [n][nsq*65536]: per sub-quantizer the oracle's compute_cross_dists_blas restatement"""
    nsq, _, ds = codebooks.shape
    out = np.zeros((x.shape[0], nsq, 65536), np.float32)
    for m in range(nsq):
        out[:, m, :] = po.cross_dists(codebooks[m], x[:, m * ds:(m + 1) * ds], sum_mode)
    return out.reshape(x.shape[0], nsq * 65536)


def tables_direct(po, codebooks, x, sum_mode):
    """x [n][dim] -> [n][nsq*65536]: the oracle's compute_dists_single_simd_cg restatement, written for 16 centroids: the codebooks
    [nsq][65536][ds] go in as [nsq*4096][16][ds] and every sub-vector is repeated 4096 times"""
    nsq, _, ds = codebooks.shape
    cb = np.ascontiguousarray(codebooks, np.float32).reshape(nsq * 4096, 16, ds)
    out = np.zeros((x.shape[0], nsq * 65536), np.float32)
    for i in range(x.shape[0]):
        out[i] = po.tables_direct(cb, np.repeat(x[i].reshape(nsq, ds), 4096, axis=0).reshape(-1), sum_mode)
    return out


_fixture = None


def fixture():
    """-> list of cases: nsq, kind, labelled, R, parts [2] uint16 [n][nsq], labels [2] or None, tables float32 [2][nsq*65536]
    (expanded from the sparse form), keys / vals = the reference's heap arrays, compiler"""
    global _fixture
    if _fixture is None:
        g = np.load(GOLDEN)
        tables = {}
        out = []
        for cid, kind, (nsq, labelled, R) in zip(g["case_ids"], g["case_kind"], g["case_meta"]):
            nsq, R = int(nsq), int(R)
            tid = "s%d_%s" % (nsq, kind)
            if tid not in tables:
                full = np.full((2 * nsq, 65536), g["fill"], np.float32)
                idx, val, off = g[tid + "_idx"], g[tid + "_val"], g[tid + "_off"]
                for j in range(2 * nsq):
                    full[j, idx[off[j]:off[j + 1]]] = val[off[j]:off[j + 1]]
                full = full.reshape(2, nsq * 65536)
                full.setflags(write=False)
                tables[tid] = full
            out.append(dict(cid=str(cid), nsq=nsq, kind=str(kind), labelled=bool(labelled), R=R,
                            parts=[g["s%d_codes%d" % (nsq, p)] for p in range(2)],
                            labels=[g["s%d_labels%d" % (nsq, p)] for p in range(2)] if labelled else None,
                            tables=tables[tid], keys=g[cid + "_keys"], vals=g[cid + "_vals"], compiler=str(g["compiler"])))
        _fixture = out
    return _fixture


def assert_heap(got, want, q, what=""):
    keys, vals, sizes = got
    wk, wv = want
    n = int(sizes[q])
    assert n == len(wk), "%s query %d: heap size %d, expected %d" % (what, q, n, len(wk))
    assert np.array_equal(keys[q, :n], wk), "%s query %d: keys differ" % (what, q)
    assert np.array_equal(np.asarray(vals[q, :n]).view(np.uint32), wv.view(np.uint32)), "%s query %d: values differ" % (what, q)
