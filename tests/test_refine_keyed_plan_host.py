"""CPU: the plan of the keyed refine store (quick-adc_amd/host/refine_keyed_plan.hpp, driver tests/cpp/refine_keyed_plan_host.cpp;
DESIGN.md section 11.14).  csrc/qadc_refine.cpp sizes and rebuilds the hash table, cuts its calls into passes and sizes its grids
with this header, and the kernels probe by its hash; the header as the library compiles it is held here to what they rely on:

  * the home slot of every key is inside the table, for every table size, and is the upper bits of MurmurHash3's finalizer;
  * from any state (bits, live, dead) with used = live + dead <= slots / 2, a put that may claim `absent` slots leaves
    used <= slots / 2 at every moment: the decision falls once, before the first pass, so no pass can ask for a rebuild;
    a table never shrinks, is rebuilt only where the call would not fit, and a call that claims nothing is never rebuilt;
  * the passes of a call cover its inputs exactly once, every pass fits one launch of one thread per input, and bounds the scratch;
  * after reserve(n), puts that keep live + dead + absent <= n plan no rebuild."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "refine_keyed_plan_host")
SLOT, PUT, RESERVE, PASS, GRID, BITS_FOR = range(6)


@pytest.fixture(scope="module")
def driver():
    _compile(EXE + ".cpp", EXE, link=False)
    return EXE


def ask(exe, tmp_path, rows):
    """-> (int64 [n][3], the header's constants)"""
    fin, fout = str(tmp_path / "keyed_plan.in"), str(tmp_path / "keyed_plan.out")
    rows = [tuple(r) + (0,) * (5 - len(r)) for r in rows]
    np.asarray(rows, np.int64).reshape(-1, 5).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    words = out.stdout.decode().split()
    assert out.returncode == 0 and words[0] == "ok" and int(words[1]) == len(rows), out.stderr.decode()
    names = ("min_bits", "max_bits", "max_keys", "pass", "pass_floats", "threads", "max_grid", "slot_bytes")
    return np.fromfile(fout, np.int64).reshape(len(rows), 3), dict(zip(names, (int(w) for w in words[2:])))


def fmix32(k):
    k = np.asarray(k, np.uint64)
    m = np.uint64(0xFFFFFFFF)
    k = k ^ (k >> np.uint64(16))
    k = (k * np.uint64(0x85EBCA6B)) & m
    k = k ^ (k >> np.uint64(13))
    k = (k * np.uint64(0xC2B2AE35)) & m
    return k ^ (k >> np.uint64(16))


def test_the_home_slot_is_inside_the_table_for_every_size(driver, tmp_path):
    rng = np.random.default_rng(1)
    keys = np.concatenate([np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64),
                           rng.integers(0, 1 << 32, 2000, dtype=np.uint64), np.arange(4096, dtype=np.uint64)])
    rows = [(SLOT, int(k), bits) for bits in range(-1, 34) for k in keys]
    got, c = ask(driver, tmp_path, rows)
    got = got[:, 0].reshape(35, len(keys))
    h = fmix32(keys)
    for i, bits in enumerate(range(-1, 34)):
        want = np.zeros(len(keys), np.uint64) if bits <= 0 else h if bits >= 32 else h >> np.uint64(32 - bits)
        assert np.array_equal(got[i].astype(np.uint64), want), bits
        if c["min_bits"] <= bits <= c["max_bits"]:
            assert (got[i] >= 0).all() and (got[i] < (1 << bits)).all(), bits
    assert c["min_bits"] >= 1 and c["max_bits"] <= 31 and c["max_keys"] * 2 == 1 << c["max_bits"]
    # a sequence of keys spreads: 4096 consecutive keys in 2^13 slots leave no slot with more than a handful
    assert np.bincount(got[14][-4096:], minlength=1 << 13).max() <= 8


def states(c):
    """(bits, live, dead) with live + dead <= slots / 2, at the edges of every table size the sweep can afford"""
    for bits in [0] + list(range(c["min_bits"], c["max_bits"] + 1)):
        half = (1 << bits) // 2 if bits else 0
        used = sorted({0, 1, half // 2, max(half - 1, 0), half})
        for u in used:
            for live in sorted({0, u // 3, max(u - 1, 0), u}):
                yield bits, live, u - live


def test_a_put_keeps_the_table_at_most_half_used(driver, tmp_path):
    _, c = ask(driver, tmp_path, [(PASS, 1)])
    rows = []
    for bits, live, dead in states(c):
        half = (1 << bits) // 2 if bits else 0
        room = max(half - live - dead, 0)
        for absent in sorted({0, 1, 2, room // 2, max(room - 1, 0), room, room + 1, room + 2, 2 * room + 1, 1000, 1 << 20, (1 << 20) + 1,
                              c["max_keys"] - live, c["max_keys"] - live + 1} - {-1}):
            if absent >= 0:
                rows.append((PUT, bits, live, dead, absent))
    got, _ = ask(driver, tmp_path, rows)
    seen = dict(rebuild=0, grown=0, same=0, refused=0, plain=0)
    for (_, bits, live, dead, absent), (refused, rebuild, nbits) in zip(rows, got.tolist()):
        what = (bits, live, dead, absent, refused, rebuild, nbits)
        assert refused == (live + absent > c["max_keys"]), what
        if refused:
            seen["refused"] += 1
            continue
        half = (1 << bits) // 2 if bits else 0
        fits = bits != 0 and live + dead + absent <= half
        assert rebuild == (not fits), what                                       # only where the call would not fit
        assert nbits >= bits and c["min_bits"] <= nbits <= c["max_bits"], what   # never smaller
        before = live if rebuild else live + dead                                # a rebuild drops the dead slots
        assert before + absent <= (1 << nbits) // 2, what                        # ... whatever the passes claim, in any order
        if not rebuild:
            assert nbits == bits, what
            seen["plain"] += 1
        else:
            smaller = nbits - 1
            assert smaller < max(bits, c["min_bits"]) or live + absent + live // 4 > (1 << smaller) // 2, "a smaller table would do: %s" % (what,)
            seen["rebuild"] += 1
            seen["grown" if nbits > bits else "same"] += 1
        if absent == 0 and bits:
            assert not rebuild, what                                             # an overwrite-only call
    assert all(seen.values()), seen                                              # rebuilds at the same size (dead slots dropped) among them


def test_reserve_makes_room_for_the_keys_it_names(driver, tmp_path):
    _, c = ask(driver, tmp_path, [(PASS, 1)])
    sizes = [0, 1, 511, 512, 513, 1000, 4096, 4097, 1 << 20, (1 << 20) + 1, 10 ** 6, c["max_keys"] - 1, c["max_keys"]]
    rows = [(RESERVE, bits, n) for bits in (0, c["min_bits"], 15, 25, c["max_bits"]) for n in sizes + [c["max_keys"] + 1]]
    got, _ = ask(driver, tmp_path, rows)
    puts, meta = [], []
    for (_, bits, n), (refused, rebuild, nbits) in zip(rows, got.tolist()):
        assert refused == (n > c["max_keys"]), (bits, n)
        if refused:
            continue
        assert nbits >= max(bits, c["min_bits"]) and rebuild == (nbits > bits) and (1 << nbits) >= 2 * n, (bits, n, nbits)
        assert nbits == bits or (1 << (nbits - 1)) < 2 * n or nbits == c["min_bits"], "reserve asks for more than it needs: %s" % ((bits, n, nbits),)
        for live, dead in ((0, 0), (n // 2, 0), (n // 3, n // 3), (n, 0), (max(n - 1, 0), 0)):
            for absent in {0, 1, n - live - dead}:
                if 0 <= absent <= n - live - dead:
                    puts.append((PUT, nbits, live, dead, absent))
    got, _ = ask(driver, tmp_path, puts)
    for row, (refused, rebuild, nbits) in zip(puts, got.tolist()):
        assert not refused and not rebuild and nbits == row[1], row


def test_the_passes_cover_a_call_and_fit_one_launch(driver, tmp_path):
    dims = [0, 1, 2, 15, 16, 17, 63, 64, 65, 96, 128, 960, 4095, 4096]
    got, c = ask(driver, tmp_path, [(PASS, d) for d in dims])
    passes = dict(zip(dims, got[:, 0].tolist()))
    for dim, p in passes.items():
        assert 1 <= p <= c["pass"], (dim, p)
        assert dim == 0 or p * dim <= c["pass_floats"] or p == 1, (dim, p)
        assert dim == 0 or p == c["pass"] or (p + 1) * dim > c["pass_floats"], "a larger pass would fit: %s" % ((dim, p),)
        for count in (0, 1, p - 1, p, p + 1, 3 * p, 3 * p + 5):
            cuts = [(o, min(count, o + p)) for o in range(0, count, p)]
            assert sum(b - a for a, b in cuts) == count and all(0 < b - a <= p for a, b in cuts)
            assert all(x[1] == y[0] for x, y in zip(cuts, cuts[1:])) and (not cuts or (cuts[0][0] == 0 and cuts[-1][1] == count))
    assert passes[4096] == 4096 and passes[0] == passes[1] == c["pass"]          # the smallest pass, which the GPU tests straddle
    ns = [0, 1, 255, 256, 257, c["pass"] - 1, c["pass"], c["pass"] + 1, c["pass"] * 4096, 1 << 40]
    got, _ = ask(driver, tmp_path, [(GRID, n) for n in ns])
    for n, g in zip(ns, got[:, 0].tolist()):
        assert 1 <= g <= c["max_grid"], (n, g)
        if n <= c["pass"]:
            assert g * c["threads"] >= n and (g - 1) * c["threads"] < max(n, 1), "a pass needs one thread per input: %s" % ((n, g),)
    assert c["threads"] % 64 == 0 and c["slot_bytes"] == 12
