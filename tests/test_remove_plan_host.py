"""CPU: the planner of remove-by-label (quick-adc_amd/host/remove_plan.hpp, driver tests/cpp/remove_plan_host.cpp; DESIGN.md
section 11.7).

qadc_adc_index_remove_labels and qadc_index_remove_labels decide four things on the host between their kernels: how large the
bitmap over [lo, hi] is, which partitions the compaction touches and from which tile, what every partition holds afterwards,
and — on the 4-bit index — which bytes behind the new last row are zeroed.  Each is checked here on the header as the library
compiles it; the zero span against a restatement of alloc_part's rule (csrc/qadc_capi.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "remove_plan_host.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "remove_plan_host")
NEVER = 2 ** 32 - 1                                                              # first[] of a partition no tile of which was hit


@pytest.fixture(scope="module")
def driver():
    _compile(SRC, EXE, link=False)
    return EXE


def run(exe, tmp_path, code_size, tile, zero_tail, spans, sizes, hits, first):
    parts = len(sizes)
    fin, fout = str(tmp_path / "remove.in"), str(tmp_path / "remove.out")
    with open(fin, "wb") as f:
        np.array([code_size, parts, tile, int(zero_tail), len(spans)], np.int32).tofile(f)
        np.asarray(spans, np.uint32).reshape(-1).tofile(f)
        for a in (sizes, hits, first):
            np.asarray(a, np.uint32).tofile(f)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stderr.decode()
    with open(fout, "rb") as f:
        got_spans = []
        for _ in spans:
            lo, last = (int(x) for x in np.fromfile(f, np.uint32, 2))
            bits, words = (int(x) for x in np.fromfile(f, np.uint64, 2))
            got_spans.append(dict(lo=lo, last=last, bits=bits, words=words))
        touched, removed = (int(x) for x in np.fromfile(f, np.uint64, 2))
        new_sizes = np.fromfile(f, np.uint32, parts).astype(np.int64)
        entries = []
        for _ in range(touched):
            part, n, first_tile, n_new = (int(x) for x in np.fromfile(f, np.uint32, 4))
            zf, zl, end = (int(x) for x in np.fromfile(f, np.uint64, 3))
            entries.append(dict(part=part, n=n, first_tile=first_tile, n_new=n_new, zero_first=zf, zero_last=zl, padded_end=end))
        assert f.read() == b""
    return got_spans, removed, new_sizes, entries


def test_the_bitmap_span_at_its_edges(driver, tmp_path):
    spans = [(0, 2 ** 32 - 1), (7, 7), (2 ** 32 - 1, 2 ** 32 - 1), (0, 0), (5, 36), (5, 37), (100, 131), (2 ** 31, 2 ** 31 + 32)]
    got, _, _, _ = run(driver, tmp_path, 8, 4096, False, spans, [], [], [])
    for (lo, hi), g in zip(spans, got):
        bits = hi - lo + 1
        assert g == dict(lo=lo, last=hi - lo, bits=bits, words=(bits + 31) // 32), (lo, hi)
    assert got[0]["bits"] == 2 ** 32 and got[0]["words"] == 2 ** 27 and got[0]["words"] * 4 == 512 << 20   # the whole label space: 512 MiB
    assert got[1]["bits"] == 1 and got[1]["words"] == 1                          # lo == hi
    assert got[4]["words"] == 1 and got[5]["words"] == 2                          # 32 bits fill a word, 33 open the next


def alloc_part_zero_span(n, cs):
    """what alloc_part (csrc/qadc_capi.cpp) guarantees of an allocation of n rows: it is align16(n * cs) + 64 bytes long and its
    last 80 bytes are cleared, of which the rows then cover those in front of n * cs"""
    length = (n * cs + 15) // 16 * 16 + 64
    return max(n * cs, length - 80), length


@pytest.mark.parametrize("code_size,zero_tail", [(4, False), (8, False), (16, False), (8, True), (16, True)])
def test_touched_partitions_new_sizes_first_tiles_and_zero_spans(driver, tmp_path, code_size, zero_tail):
    T = 4096
    #        empty  no hit  all go  one of one  odd left   first tile past the end (clamped)   a hit in the last tile   hits > n (clamped)
    sizes = [0,     100,    T + 1,  1,          3 * T,     T,                                  2 * T + 3,               5,        0,  7]
    hits = [0,      0,      T + 1,  1,          3 * T - 1, 3,                                  1,                       9,        4,  0]
    first = [NEVER, NEVER,  0,      0,          0,         8,                                  2,                       0,        0,  NEVER]
    _, removed, new_sizes, entries = run(driver, tmp_path, code_size, T, zero_tail, [], sizes, hits, first)
    want_touched = [p for p in range(len(sizes)) if sizes[p] and hits[p]]
    assert [e["part"] for e in entries] == want_touched == [2, 3, 4, 5, 6, 7]   # empty partitions and partitions with no hit are skipped
    want_new = [s - min(h, s) if s else 0 for s, h in zip(sizes, hits)]
    assert new_sizes.tolist() == want_new and removed == sum(sizes) - sum(want_new)
    for e in entries:
        p = e["part"]
        assert e["n"] == sizes[p] and e["n_new"] == want_new[p]
        last_tile = (sizes[p] - 1) // T
        assert e["first_tile"] == min(first[p], last_tile) <= last_tile          # never past the last tile
        if zero_tail:
            n = e["n_new"]
            assert e["zero_first"] == n * code_size and e["zero_last"] == e["padded_end"] == (n * code_size + 15) // 16 * 16 + 64
            assert (e["zero_first"], e["zero_last"]) == alloc_part_zero_span(n, code_size)
            assert (e["zero_last"] - e["zero_first"]) % 8 == 0 and e["zero_last"] - e["zero_first"] <= 72   # the kernel stores dwordx2
            assert e["zero_last"] <= (sizes[p] * code_size + 15) // 16 * 16 + 64  # inside what the partition had before
        else:
            assert e["zero_first"] == e["zero_last"] == 0
    if zero_tail:                                                                # n' = 0, 1 and an odd n' (at 8-byte rows: half a word) are among them
        assert {0, 1} <= {e["n_new"] for e in entries} and any(e["n_new"] % 2 and e["n_new"] > 1 for e in entries)


def test_the_zero_span_follows_index_padded_end(driver, tmp_path):
    """n' = 0, 1 and an odd n' at 8-byte rows, each as the only touched partition; and 16-byte rows beside them"""
    for cs in (8, 16):
        for n_new in (0, 1, 2, 4097, 4098):
            _, _, new_sizes, entries = run(driver, tmp_path, cs, 4096, True, [], [n_new + 3], [3], [0])
            assert new_sizes.tolist() == [n_new] and len(entries) == 1
            e = entries[0]
            assert (e["zero_first"], e["zero_last"]) == alloc_part_zero_span(n_new, cs) == (n_new * cs, e["padded_end"])
            assert e["zero_last"] - e["zero_first"] == (72 if cs == 8 and n_new % 2 else 64)


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(driver, tmp_path):
    """the planner, stand-alone, built with -fsanitize=address,undefined: the edge spans and a call's plan, no report"""
    exe = str(tmp_path / "remove_plan_asan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           SRC, "-o", exe])
    spans, removed, new_sizes, entries = run(exe, tmp_path, 8, 4096, True, [(0, 2 ** 32 - 1), (9, 9)], [0, 5, 4097, 1], [0, 2, 4097, 0],
                                             [NEVER, 0, 9, NEVER])
    assert spans[0]["words"] == 2 ** 27 and removed == 4099 and new_sizes.tolist() == [0, 3, 0, 1]
    assert [e["part"] for e in entries] == [1, 2] and entries[1]["first_tile"] == 1
