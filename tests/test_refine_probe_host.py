"""CPU: the host twin of the probed exact search (refine::knn_probed of quick-adc_amd/host/refine.hpp, driver
tests/cpp/refine_probe_host.cpp) — the written definition of qadc_refine_knn_probed, to which the GPU is held
bit for bit.

The twin is compared, bit for bit, with an independent numpy restatement (tests/refine_probe_cases.py), with the twin's own rerank fed
the entries the driver lists itself where they fit rerank's 8192, and, at ma = K with labels equal to the store's keys, with
refine::knn."""
import subprocess

import numpy as np
import pytest

import refine_knn_cases as kc
import refine_probe_cases as pc


@pytest.fixture(scope="module")
def driver():
    return pc.build_driver()


def check(exe, tmp_path, cases, names, want_rerank=True):
    for name, c, got in zip(names, cases, pc.run_twin(exe, tmp_path, cases)):
        pc.assert_same(got, pc.run_numpy(c), name)
        for i, g in enumerate(got):
            assert (g["rr"] is not None) == want_rerank, name
            if g["rr"] is not None:
                diff = pc.same(g, g["rr"])
                assert diff is None, "%s call %d: %s differs from rerank of the entries" % (name, i, diff)


def mixed_calls(rng, dim, K, rows, labels):
    """probes of 1, 2 and K partitions, a repeat, entries outside [0, K) (skipped, the device form's rule), a query whose probes are
    all empty or outside, R below, at and above the rows, and filters"""
    q = rng.normal(size=(5, dim)).astype(np.float32)
    a2 = pc.probes(rng, 5, 2, K)
    a2[0] = (0, 0)                                           # partition 0 is empty: size 0 and fillers
    a2[1] = (4, 4)                                           # a repeat counts once
    a2[2] = (-1, 3)
    a2[3] = (K, K + 7)                                       # nothing probed
    calls = [pc.call(q, pc.probes(rng, 5, 1, K), 10), pc.call(q, a2, 20), pc.call(q, pc.probes(rng, 5, K, K), rows + 5),
             pc.call(q, pc.probes(rng, 5, K, K), rows), pc.call(q, pc.probes(rng, 5, K, K), rows - 1), pc.call(q[:1], [[3, 4]], 1)]
    pick = rng.choice(labels, len(labels) // 3, replace=False)
    for mode in ("exclude", "allow"):
        calls += [pc.call(q, pc.probes(rng, 5, 3, K), 50, (mode, s)) for s in (pick, np.zeros(0, np.uint32), labels)]
    return calls


@pytest.mark.parametrize("dtype", ["f32", "f16", "sq8"])
def test_the_twin_equals_the_numpy_restatement_and_its_own_rerank(driver, tmp_path, dtype):
    rng = np.random.default_rng(61 + pc.DTYPES[dtype])
    K, rows = len(pc.SIZES), sum(pc.SIZES)
    cases, names = [], []
    for dim in (1, 65, 128):
        for keyed in (False, True):
            cases.append(pc.dense_case(rng, dim, dtype, lambda vec, labels: mixed_calls(rng, dim, K, rows, labels), lo=1000, keyed=keyed))
            names.append("labelled dim %d %s keyed %d" % (dim, dtype, keyed))
        # labels that repeat within and across partitions, and labels the store does not hold
        c = pc.dense_case(rng, dim, dtype, lambda vec, labels: [], lo=0)
        dup = [np.array(p[0]) for p in c["parts"]]
        dup[3][:40] = dup[4][:40]                            # across partitions
        dup[4][100:120] = dup[4][200:220]                    # within one
        dup[3][50:60] = np.arange(5000, 5010)                # missing
        dup[2][:5] = 0xFFFFFFFF                              # never held
        c["parts"] = [pc.part(l) for l in dup]
        c["calls"] = mixed_calls(rng, dim, K, rows, np.concatenate(dup))
        c["index_filter"] = ("exclude", np.concatenate([dup[4][:10], dup[3][50:53]]).astype(np.uint32))
        cases.append(c)
        names.append("repeated labels dim %d %s" % (dim, dtype))
        # an unlabelled index: key = position, so the partitions' keys overlap
        c = pc.dense_case(rng, dim, dtype, lambda vec, labels: [], lo=0)
        c["parts"] = [pc.part(None, 0, n) for n in pc.SIZES]
        c["calls"] = mixed_calls(rng, dim, K, rows, np.arange(700, dtype=np.uint32))
        cases.append(c)
        names.append("unlabelled dim %d %s" % (dim, dtype))
    check(driver, tmp_path, cases, names)


def test_more_entries_than_rerank_takes(driver, tmp_path):
    rng = np.random.default_rng(7)
    sizes = (5000, 4000, 3000)
    c = pc.dense_case(rng, 4, "f32", lambda vec, labels: [pc.call(vec[:3], [[0, 1, 2]] * 3, 1024), pc.call(vec[:2], [[1, 0], [2, 0]], 7)], sizes=sizes)
    check(driver, tmp_path, [c], ["12000 entries"], want_rerank=False)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_every_partition_probed_with_the_stores_keys_as_labels_is_knn(driver, tmp_path, dtype):
    rng = np.random.default_rng(11)
    knn_exe = kc.build_driver()
    K, rows = len(pc.SIZES), sum(pc.SIZES)
    for keyed in (False, True):
        for dim in (63, 128):
            vec = rng.normal(size=(rows, dim)).astype(np.float32)
            q = rng.normal(size=(4, dim)).astype(np.float32)
            labels = rng.permutation(np.arange(300, 300 + rows, dtype=np.uint32))
            flt = ("allow", labels[::3])
            store = [kc.put(np.arange(300, 300 + rows, dtype=np.uint32), vec)] if keyed else [kc.add(300, vec)]
            everything = np.tile(np.arange(K, dtype=np.int32), (4, 1))
            probed = pc.case(keyed, dim, dtype, store, pc.split_labels(labels),
                             [pc.call(q, everything, R, f) for R in (1, 100, rows + 5) for f in (None, flt)])
            whole = kc.case(keyed, dim, dtype, store + [kc.knn(q, R, f) for R in (1, 100, rows + 5) for f in (None, flt)])
            got = pc.run_twin(driver, tmp_path, [probed])[0]
            want = kc.run_twin(knn_exe, tmp_path, [whole])[0]
            for g, w in zip(got, want):
                assert g["missing"] == 0 and kc.same(g, w) is None


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "refine_probe_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           pc.EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(9)
    K, rows = len(pc.SIZES), sum(pc.SIZES)
    cases = [pc.dense_case(rng, 65, dtype, lambda vec, labels: mixed_calls(rng, 65, K, rows, labels), keyed=keyed)
             for dtype, keyed in (("f32", False), ("f16", True), ("sq8", False))]
    for c, got in zip(cases, pc.run_twin(exe, tmp_path, cases)):
        pc.assert_same(got, pc.run_numpy(c))
