"""CPU: the host twin of SQ8 refine rows and of the read-back (quick-adc_amd/host/refine.hpp) against an
independent numpy restatement of encode, decode, range and the clamp count (tests/refine_sq_cases.py), bit for bit: stored bytes,
decoded rows, the counter, keys, the distances' bit patterns, sizes and missing counts."""
import numpy as np
import pytest

import refine_sq_cases as sq

F32 = np.float32


@pytest.fixture(scope="module")
def exe():
    return sq.build_driver()


def check(exe, tmp_path, scripts):
    got = sq.run_twin(exe, tmp_path, scripts)
    wants = sq.isolated(tmp_path, "run_numpy_all", scripts)                           # (numpy under the default floating-point environment)
    for s, g, want in zip(scripts, got, wants):
        assert sq.same(g, want) is None, "dim %d %s keyed=%s: %s" % (s["dim"], s["dtype"], s["keyed"], sq.same(g, want))
    return got


def test_exact_grid(exe, tmp_path):
    """vmin an integer, step a power of two: |x - decode(encode(x))| <= step / 2 exactly, ties at k + 0.5 go to the even byte"""
    pairs = [sq.grid_script(dim) for dim in sq.DIMS]
    got = check(exe, tmp_path, [s for s, _ in pairs])
    for (s, v), g in zip(pairs, got):
        rows, raw, info = g["ops"][1]["rows"], g["ops"][2]["bytes"], g["ops"][3]
        assert g["ops"][1]["found"].all() and int(info["clamped"][0]) == 0
        assert (np.abs(v - rows) <= F32(0.125)).all()                                # exact: every difference is a multiple of 2^-4
        u = (v - F32(-3.0)) * F32(4.0)                                                # exact
        tie = (u - np.floor(u)) == F32(0.5)
        assert tie.any() and (np.floor(u[tie]) % 2 == 0).any() and (np.floor(u[tie]) % 2 == 1).any()
        assert (raw[tie] % 2 == 0).all(), "a tie went to the odd byte"
        assert np.array_equal(raw[tie], (np.floor(u[tie]) + (np.floor(u[tie]) % 2)).astype(np.uint8))
        on = u == np.floor(u)
        assert np.array_equal(raw[on], u[on].astype(np.uint8)) and np.array_equal(rows[on], v[on])


@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_edges(exe, tmp_path, keyed):
    scripts = [sq.edge_script(dim, keyed) for dim in sq.DIMS]
    got = check(exe, tmp_path, scripts)
    for s, g in zip(scripts, got):
        raw, clamped = g["ops"][-2]["bytes"], int(g["ops"][-1]["clamped"][0])
        bits = s["step"].view(np.uint32)                                              # (steps are >= +0: their bits order as they do,
        live = bits > 0                                                               # and a subnormal step stays one in a process
        normal = bits > np.array([1e-30], F32).view(np.uint32)[0]                     # that flushes subnormals)
        # rows 0 .. 12 are the specials of edge_script, in its order
        assert (raw[0][normal] == 0).all() and (raw[1][normal] == 255).all()          # x == vmin, x == vmin + 255 step
        assert (raw[2] == 0).all() and (raw[3][normal] == 255).all()                  # just outside both ends
        assert (raw[5][live] == 255).all() and (raw[6] == 0).all()                    # +inf, -inf
        assert (raw[7] == 0).all() and (raw[8] == 0).all()                            # NaN of either sign
        assert (raw[:, ~live] == 0).all()                                             # constant dimensions
        _, cl = sq.isolated(tmp_path, "np_encode", s["ops"][0][2] if keyed else np.concatenate([s["ops"][0][2], s["ops"][1][2]]), s["vmin"],
                            s["step"])
        assert clamped == int(cl.sum()) and clamped > 0
        assert not cl[0][~live].any() and cl[7].all() and cl[2].all()                 # x == vmin on step 0: not counted; NaN: counted
        if s["dim"] >= 3:
            assert (raw[4][2] == 255) and cl[4][2]                                    # subnormal step: one ulp above vmin is +inf steps


def test_range_and_refusals(exe, tmp_path):
    got = check(exe, tmp_path, sq.range_scripts())
    for g in got[:3]:
        full, none, one = g["ops"][0], g["ops"][1], g["ops"][2]
        dim = len(full["vmin"])
        assert full["vmin"][dim // 2] == 0 and full["step"][dim // 2] == 0           # nothing finite in the column
        assert not none["vmin"].any() and not none["step"].any()                     # n = 0
        assert not one["step"].any()                                                 # one row: max == min in every column
    zero = got[3]["ops"][0]
    assert np.array_equal(zero["vmin"].view(np.uint32), np.array([0x80000000, 0x80000000, 0x80000000], np.uint32))   # -0 below +0
    assert np.array_equal(zero["step"].view(np.uint32)[:2], np.zeros(2, np.uint32))
    assert np.isinf(got[4]["ops"][0]["step"][0])                                     # max - min overflows
    refused = check(exe, tmp_path, sq.refusal_scripts())
    assert all(g["refused"] == 1 for g in refused)


@pytest.mark.parametrize("dim", sq.DIMS)
def test_keyed_put_overwrite_remove(exe, tmp_path, dim):
    s = sq.keyed_script(dim)
    g = check(exe, tmp_path, [s])[0]
    v = s["ops"][0][2]
    _, cl = sq.np_encode(v, s["vmin"], s["step"])
    winners = [7, 5, 4, 6] + list(range(8, 60))                                      # the last inputs of keys 5, 9, 12, 7, then 100 ..
    assert int(g["ops"][1]["clamped"][0]) == int(cl[winners].sum()) < int(cl.sum())
    assert list(g["ops"][2]["found"]) == [1, 1, 1, 1, 0, 0]
    assert list(g["ops"][7]["found"]) == [0, 1, 1, 0, 1]
    assert (g["ops"][7]["rows"][0].view(np.uint32) == 0x7FC00000).all()


@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_rerank_and_knn(exe, tmp_path, keyed):
    scripts = [sq.rerank_script(dim, keyed, r_in, rows=120, nq=4) for dim in (1, 65, 260) for r_in in (17, 65)]
    scripts += [sq.knn_script(dim, keyed, nq, rows=90) for dim, nq in ((1, 2), (96, 5), (260, 3))]
    check(exe, tmp_path, scripts)


def test_get_of_float_and_half_stores(exe, tmp_path):
    got = check(exe, tmp_path, sq.plain_get_scripts())
    dense = got[0]["ops"][1]
    assert list(dense["found"]) == [0, 1, 1, 0, 0, 0, 1, 1, 1]


def test_a_thread_that_flushes_subnormals_changes_no_stored_bit(exe, tmp_path):
    """The host side of the definition — the parameters' check, inv, the encode, the clamp count, the range — runs in the default
    floating-point environment whatever the caller's: the driver with subnormals flushed gives the same bytes, counts and ranges."""
    import platform
    if platform.machine() not in ("x86_64", "AMD64"):
        pytest.skip("the driver sets the flush bits of MXCSR")
    N = 0x80000000                                                                    # (from bits: this process may flush conversions too)
    tiny = np.array([[71362, 2140873, N | 1427248], [3568120, N | 71362, 1427248], [0, 7136238, 0]], np.uint32).view(F32)   # subnormals
    scripts = [sq.edge_script(dim, keyed) for dim in (63, 260) for keyed in (False, True)] + [sq.script(3, "f32", [("range", tiny)])]
    scripts += sq.refusal_scripts()
    scripts.append(sq.script(2, "sq8", [], vmin=np.zeros(2), step=np.array([0x3F800000, N | 71362], np.uint32).view(F32)))   # a negative subnormal step
    plain, flushed = sq.run_twin(exe, tmp_path, scripts), sq.run_twin(exe, tmp_path, scripts, flush=True)
    for s, a, b in zip(scripts, plain, flushed):
        assert a["refused"] == b["refused"]
        for op, x, y in zip(s["ops"], a["ops"], b["ops"]):
            if op[0] in ("bytes", "info", "range"):
                for name in x:
                    assert np.array_equal(np.ascontiguousarray(x[name]).view(np.uint8), np.ascontiguousarray(y[name]).view(np.uint8)), \
                        "dim %d: %s of %s differs under flushed subnormals" % (s["dim"], name, op[0])
    assert plain[-1]["refused"] == 1 and (plain[4]["ops"][0]["step"].view(np.uint32) != 0).all()
