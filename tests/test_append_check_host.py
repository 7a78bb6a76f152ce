"""CPU: the refusals of the append path (quick-adc_amd/host/append_check.hpp; driver tests/cpp/append_check_host.cpp), which
qadc_index_add_vectors* / _reserve / _read_partition and their qadc_adc_index_* twins run before they touch the device.

Every refusal of both engines is driven once; its status and its whole text are compared with the text the engine's own source
held before the checks were shared, written out here.  The accepting cases return QADC_OK and no text."""
import os
import subprocess

import pytest

from test_scanner_hip_cpp import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "append_check_host")
OK, E_ARG, E_STATE = 0, -1, -4
# engine -> (an entry point's name, the set_pq the refusal names, the encoder's widest vector: 0 = any)
ENGINES = {"index": ("qadc_index_add_vectors_labelled", "qadc_index_set_pq", 2048),
           "adc": ("qadc_adc_index_add_vectors_labelled_device", "qadc_adc_index_set_pq", 0)}


@pytest.fixture(scope="module")
def driver():
    _compile(os.path.join(ROOT, "tests", "cpp", "append_check_host.cpp"), EXE, link=False)
    return EXE


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, timeout=60)
    assert out.returncode == 0, args
    status, text = out.stdout.decode().split("\n", 1)
    assert text.endswith("\n")
    return int(status), text[:-1]


def add(exe, engine, dim=16, K=8, labeled=-1, sizes=(), labelled=False, vectors=True, labels=False, count=10, labels_offset=0,
        sum_mode=1):
    call, set_pq, max_dim = ENGINES[engine]
    return _run(exe, "add", call, set_pq, dim, K, max_dim, labeled, ",".join(map(str, sizes)) or "-", int(labelled), int(vectors),
                int(labels), count, labels_offset, sum_mode)


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_every_add_vectors_refusal_keeps_its_status_and_text(driver, engine):
    call, set_pq, max_dim = ENGINES[engine]
    held = [3, 0, 0, 0, 0, 0, 0, 0]
    assert add(driver, engine, K=0, labelled=True, labels=True) == \
        (E_STATE, call + ": a flat index (no coarse quantizer) keys its vectors by position and takes no labels")
    assert add(driver, engine, labeled=0, sizes=held, labelled=True, labels=True) == \
        (E_STATE, call + ": the index holds unlabelled partitions, whose keys are positions")
    assert add(driver, engine, labelled=True, labels=False) == (E_ARG, "labels is null")
    assert add(driver, engine, dim=0) == (E_ARG, set_pq + " has not been called: the index has no codebooks")
    assert add(driver, engine, dim=0, K=0, labelled=True, labels=True) == \
        (E_ARG, set_pq + " has not been called: the index has no codebooks")     # (no quantizer at all: not "a flat index")
    if max_dim:
        assert add(driver, engine, dim=2064) == (E_ARG, "dim must be <= 2048 (the encoder keeps the codebooks in LDS)")
        assert add(driver, engine, dim=2048) == (OK, "")
    else:
        assert add(driver, engine, dim=2064) == (OK, "")
    for bad in (2, -1):
        assert add(driver, engine, sum_mode=bad) == (E_ARG, "sum_mode is 0 (source order) or 1 (as compiled)")
    assert add(driver, engine, vectors=False) == (E_ARG, "vectors is null")
    assert add(driver, engine, count=2 ** 32 - 1, labels_offset=1) == (E_ARG, "labels_offset + count = 4294967296 exceeds 2^32 - 1")
    assert add(driver, engine, count=2 ** 33) == (E_ARG, "labels_offset + count = 8589934592 exceeds 2^32 - 1")
    assert add(driver, engine, sizes=[0, 0, 0]) == (E_ARG, "the coarse quantizer has 8 centroids and the index 3 partitions")
    assert add(driver, engine, labeled=0, sizes=held) == \
        (E_ARG, "the index holds unlabelled partitions: vectors added through a coarse quantizer are labelled")
    assert add(driver, engine, K=0, sizes=[4, 0]) == (E_ARG, "a flat index (no coarse quantizer) has one partition: the index has 2")
    assert add(driver, engine, K=0, labeled=1, sizes=[4]) == (E_ARG, "the index is labelled: a flat index keys its vectors by position")


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_the_refusals_come_in_the_engines_order(driver, engine):
    call, set_pq, max_dim = ENGINES[engine]
    # labelled-on-flat before everything; no codebooks before sum_mode; sum_mode before vectors; vectors before the row limit; ...
    assert add(driver, engine, K=0, labelled=True, sum_mode=2, vectors=False)[0] == E_STATE
    assert add(driver, engine, dim=0, sum_mode=2)[1].startswith(set_pq)
    assert add(driver, engine, dim=4096, sum_mode=2)[1].startswith("dim must be" if max_dim else "sum_mode")
    assert add(driver, engine, sum_mode=2, vectors=False)[1].startswith("sum_mode")
    assert add(driver, engine, vectors=False, count=2 ** 33)[1] == "vectors is null"
    assert add(driver, engine, count=2 ** 33, sizes=[0, 0])[1].startswith("labels_offset + count")


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_what_is_accepted(driver, engine):
    held = [3, 0, 5, 0, 0, 0, 0, 1]
    for case in (dict(), dict(count=0, vectors=False), dict(sum_mode=0), dict(sizes=[0] * 8), dict(labeled=1, sizes=held),
                 dict(labeled=0, sizes=[0] * 8),                                 # unlabelled, but nothing held
                 dict(labelled=True, labels=True), dict(labelled=True, labels=False, count=0, vectors=False),
                 dict(labelled=True, labels=True, labeled=1, sizes=held), dict(labelled=True, labels=True, labeled=0, sizes=[0] * 8),
                 dict(count=2 ** 32 - 1), dict(count=5, labels_offset=2 ** 32 - 6),
                 dict(K=0), dict(K=0, sizes=[7], labeled=0), dict(K=0, sizes=[0], labeled=1), dict(K=0, count=0, labels_offset=9)):
        assert add(driver, engine, **case) == (OK, ""), case


def test_reserve(driver):
    for part_count, has in ((-1, 1), (-3, 0), (1, 0), (8, 0)):
        assert _run(driver, "reserve", part_count, has) == (E_ARG, "bad capacity array")
    for part_count, has in ((0, 0), (0, 1), (1, 1), (8, 1)):
        assert _run(driver, "reserve", part_count, has) == (OK, "")


def test_read_partition(driver):
    assert _run(driver, "read", "5,0,9", 3, 0, 0) == (E_ARG, "partition 3 does not exist (3 partitions)")
    assert _run(driver, "read", "5,0,9", -1, 0, 1) == (E_ARG, "partition -1 does not exist (3 partitions)")
    assert _run(driver, "read", "-", 0, 0, 0) == (E_ARG, "partition 0 does not exist (0 partitions)")
    assert _run(driver, "read", "5,0,9", 2, 4, 6) == (E_ARG, "rows [4, 10) are outside partition 2 of 9 codes")
    assert _run(driver, "read", "5,0,9", 1, 0, 1) == (E_ARG, "rows [0, 1) are outside partition 1 of 0 codes")
    assert _run(driver, "read", "5,0,9", 0, 4294967295, 4294967295) == \
        (E_ARG, "rows [4294967295, 8589934590) are outside partition 0 of 5 codes")
    for part, first, count in ((0, 0, 5), (0, 5, 0), (1, 0, 0), (2, 4, 5), (2, 9, 0)):
        assert _run(driver, "read", "5,0,9", part, first, count) == (OK, "")
