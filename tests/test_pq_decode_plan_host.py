"""CPU: the launch geometry of the PQ decode kernels (quick-adc_amd/host/pq_decode_plan.hpp, driver
tests/cpp/pq_decode_plan_host.cpp), swept without a GPU: every dim a (sq_count, sq_bits) pair allows, both sides of the LDS
threshold, the edges of the rotation tile and of a pass.  What the kernels index with is checked here: no block, tile or LDS size
that could leave a buffer reaches a launch."""
import numpy as np
import pytest

import pq_decode_compose as pdc

LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def exe():
    return pdc.build_plan_driver()


def max_dim(bits):
    return 2048 if bits == 4 else 4096


@pytest.mark.parametrize("nsq,bits", pdc.PAIRS, ids=[pdc.pair_id(p) for p in pdc.PAIRS])
def test_every_dim_of_a_pair(exe, nsq, bits):
    ns = [1, 63, 64, 65, pdc.CHUNK]
    lines = [(nsq, bits, dim, n, al) for dim in range(1, 4097) for n in (ns if dim % nsq == 0 else ns[:1]) for al in (0, 1)]
    for line, p in zip(lines, pdc.plan(exe, lines)):
        _, _, dim, n, al = line
        if dim % nsq or dim > max_dim(bits):
            assert p is None, line
            continue
        assert p is not None, line
        assert p["dim"] == dim and p["dsub"] * nsq == dim and p["centroids"] == 1 << bits
        assert p["code_bytes"] == (nsq // 2 if bits == 4 else nsq * bits // 8)
        # the gather: 16-byte stores only where every row starts on a 16-byte boundary
        assert p["vec"] == (4 if al and dim % 4 == 0 else 1) and p["lanes_per_row"] * p["vec"] == dim
        assert 1 <= p["rows_per_wg"] <= 256 and p["row_blocks"] == -(-n // p["rows_per_wg"])
        assert 1 <= p["gather_grid"] <= 1024 and p["gather_grid"] <= max(p["row_blocks"], 1)
        code_lds = -(-p["rows_per_wg"] * p["code_bytes"] // 16) * 16
        assert p["cb_bytes"] == (1 << bits) * dim * 4
        assert p["cb_in_lds"] == int(bits != 16 and p["cb_bytes"] + code_lds <= LDS_LIMIT)
        assert p["gather_lds"] == (p["cb_bytes"] if p["cb_in_lds"] else 0) + code_lds <= LDS_LIMIT
        assert p["cb_bytes"] % 16 == 0                                        # the code bytes start on a 16-byte boundary of the LDS
        # the rotation: whole tiles cover the pass, the grid fits a launch
        assert p["reg"] in (1, 2, 4) and p["tile"] == 16 * p["reg"]
        assert p["col_tiles"] == -(-dim // p["tile"]) and p["row_tiles"] == -(-n // p["tile"])
        assert p["rot_grid"] == p["col_tiles"] * p["row_tiles"] < 1 << 31
        assert p["rot_lds"] == 2 * 32 * p["tile"] * 4 <= 48 * 1024
        assert (32 * p["tile"]) % 256 == 0                                    # every lane stages a whole number of entries per window
        assert p["err_grid"] == -(-n // 64)


def test_lds_threshold_from_both_sides(exe):
    """4 bits: 16 dim 4 bytes of codebooks beside the code bytes of a block; 8 bits: 256 dim 4 bytes; 16 bits never"""
    got = pdc.plan(exe, [(16, 4, 1008, 100, 1), (16, 4, 1024, 100, 1), (4, 8, 60, 100, 1), (4, 8, 64, 100, 1), (2, 16, 2, 100, 1),
                         (16, 8, 48, 100, 0), (16, 8, 64, 100, 0)])
    assert [p["cb_in_lds"] for p in got] == [1, 0, 1, 0, 0, 1, 0]
    assert got[0]["gather_lds"] > 64512 and got[1]["gather_lds"] < 4096 and got[4]["gather_lds"] < 4096


@pytest.mark.parametrize("dim", [16, 17 * 16, 32, 48, 64, 80, 100 * 4, 24 * 4])
def test_rotation_chains_cover_the_pass_once(exe, dim):
    """every (row, column) of a pass belongs to exactly one register of one lane of one tile, at tile edges too"""
    lines = [(4, 8, dim, n, 0) for n in (1, 15, 16, 17, 63, 64, 65, 130)]
    for line, p in zip(lines, pdc.plan(exe, lines)):
        assert p is not None and p["cover"] == 1, line
    for nsq, bits, d in ((16, 4, 16), (16, 4, 32), (2, 16, 24), (2, 16, 100)):
        for p in pdc.plan(exe, [(nsq, bits, d, n, 0) for n in (1, 33, 64, 65)]):
            assert p["cover"] == 1 and p["reg"] == (1 if d <= 16 else 2 if d <= 32 else 4)


def test_refused_shapes(exe):
    lines = [(16, 4, 32, pdc.CHUNK + 1, 1), (7, 8, 14, 10, 1), (4, 4, 8, 10, 1), (16, 16, 32, 10, 1), (4, 8, 0, 10, 1), (16, 4, 2064, 10, 1),
             (4, 8, 4100, 10, 1), (4, 8, 4096, 3, 1), (16, 4, 2048, 3, 1), (4, 8, 8, 0, 1)]
    got = pdc.plan(exe, lines)
    assert [p is None for p in got] == [True] * 7 + [False] * 3
    assert got[-1]["row_blocks"] == 0 and got[-1]["rot_grid"] == 0 and got[-1]["err_grid"] == 0 and got[-1]["gather_grid"] == 1
    assert np.all([got[7]["cb_in_lds"], got[8]["cb_in_lds"]]) == 0
