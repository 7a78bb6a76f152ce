"""CPU: the host twin of the keyed refine store (refine::keyed_store in quick-adc_amd/host/refine.hpp, driver
tests/cpp/refine_keyed_host.cpp) — the written definition of qadc_refine_put, _remove and of _rerank over a keyed store (DESIGN.md
section 11.14), to which the GPU store is held bit for bit.

The twin runs scripts of put, remove and rerank and is compared, operation by operation and bit for bit, with an independent
numpy restatement (tests/refine_keyed_cases.py: a dict from key to row, refine_cases.np_distance, a sort of words).  The two kinds
of store are two types in the twin, so a put on a dense store does not compile there; the mode errors of the C calls are tested on
the library (tests/test_gpu_refine_keyed.py)."""
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_keyed_cases as kc


@pytest.fixture(scope="module")
def driver():
    return kc.build_driver()


def life(rng, dim):
    """last-wins duplicates, overwrite, remove then re-put, remove of absent keys and of keys listed twice, the edge keys, the
    refused filler key; after every step a rerank over every key ever used and some never used"""
    v = lambda n: rng.normal(size=(n, dim)).astype(np.float32)
    a = np.array([0, 0xFFFFFFFE, 7, 7, 1 << 31, 12345, 7, 99], np.uint32)                 # key 7 three times: the last wins
    b = np.array([12345, 0, 500, 501], np.uint32)                                         # overwrites two, adds two
    ever = np.unique(np.concatenate([a, b, np.array([1, 2, 0xFFFFFFFD, 0xFFFFFFFF, 98, 100], np.uint32)]))
    q = v(3)
    look = lambda: kc.rerank(q, np.stack([rng.permutation(ever) for _ in range(3)]), len(ever) + 2)
    script = [look(), kc.put(a, v(len(a))), look(), kc.put(b, v(len(b))), look(),
              kc.remove(np.array([7, 7, 3, 500, 0xFFFFFFFF, 7], np.uint32)), look(),                       # 7 listed three times, 3 and the filler absent
              kc.remove(np.array([7, 3], np.uint32)), look(),                                             # nothing left to remove
              kc.put(np.array([7, 500], np.uint32), v(2)), look(),                                        # re-put with new vectors
              kc.put(np.array([5, 0xFFFFFFFF, 6], np.uint32), v(3)), look(),                              # refused: the map unchanged
              kc.remove(ever), look(),
              kc.put(np.array([0xFFFFFFFE], np.uint32), v(1)), look()]
    return script


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim", [1, 65, 128])
def test_the_twin_equals_the_numpy_restatement(driver, tmp_path, dim, dtype):
    rng = np.random.default_rng(31 + dim + rc.DTYPES[dtype])
    script = life(rng, dim)
    got = kc.run_twin(driver, tmp_path, dim, dtype, script)
    kc.assert_same(got, kc.run_numpy(dim, dtype, script), "dim %d %s" % (dim, dtype))
    # the life holds what it is built for
    puts = [g for g, op in zip(got, script) if op[0] == "put"]
    removes = [g for g, op in zip(got, script) if op[0] == "remove"]
    assert [p["ok"] for p in puts] == [1, 1, 1, 0, 1] and [p["live"] for p in puts] == [6, 8, 8, 8, 1]
    assert [r["removed"] for r in removes] == [2, 0, 8] and [r["live"] for r in removes] == [6, 6, 0]
    ranks = [g for g, op in zip(got, script) if op[0] == "rerank"]
    assert ranks[0]["missing"] == 3 * 14 and (ranks[0]["sizes"] == 0).all()
    assert ranks[5]["sizes"].tolist() == ranks[6]["sizes"].tolist() == [8, 8, 8] and rc.same(ranks[5], ranks[6]) is None


def test_values_counts_and_a_converted_half_go_through_a_keyed_store(driver, tmp_path):
    """the dense twin's edge cases, their rows put under sparse keys: skipped entries, counts, ties, R above the survivors; and
    the half range through put"""
    rng = np.random.default_rng(33)
    for dtype, c in (("f32", rc.edge_case(rng, 65, "f32")), ("f16", rc.edge_case(rng, 64, "f16")), ("f16", rc.half_range_case(rng, 63))):
        lo, vec = c["adds"][0]
        spread = lambda k: ((k.astype(np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(0xFFFFFFFF)).astype(np.uint32)
        labels = spread(np.arange(lo, lo + len(vec), dtype=np.uint32))
        assert len(np.unique(labels)) == len(labels)
        keys = spread(c["keys"])
        script = [kc.put(labels, vec), kc.rerank(c["queries"], keys, c["R"], c["counts"], c["values"])]
        got = kc.run_twin(driver, tmp_path, c["dim"], dtype, script)
        kc.assert_same(got, kc.run_numpy(c["dim"], dtype, script), dtype)
        if c["counts"] is not None:                                              # the dense twin's result, its keys mapped: holds() is all that differs
            (dense,) = rc.run_twin(rc.build_driver(), tmp_path, [c])
            assert got[1]["sizes"].tolist() == dense["sizes"].tolist() and got[1]["missing"] == dense["missing"]
            assert np.array_equal(np.sort(got[1]["dist"].view(np.uint32), axis=1), np.sort(dense["dist"].view(np.uint32), axis=1))


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "refine_keyed_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           kc.EXE + ".cpp", "-o", exe])
    rng = np.random.default_rng(9)
    for dim, dtype in ((65, "f16"), (1, "f32")):
        script = life(rng, dim)
        kc.assert_same(kc.run_twin(exe, tmp_path, dim, dtype, script), kc.run_numpy(dim, dtype, script))
