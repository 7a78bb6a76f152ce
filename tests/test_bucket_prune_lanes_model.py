"""CPU: the quarter window of tools/bucket_prune.py ("pruned groups"; bkt_prune_lanes = 16).  With 16-lane
quarters a wave iteration that runs loads only the quarters in which some lane group keeps; the tool counts windows of 16 groups
the way wave_fraction counts windows of 64.  Here the count is made directly: every key's groups laid out one by one on the group
axis, the axis cut into wave iterations of four quarters.  The columns the tool had before keep their values."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bucket_prune as bp  # noqa: E402

NKEYS = 1 << 12              # a small key space: the window count does not depend on its size
GROUPS_PER_KEY = (1, 2, 3, 8, 16, 27)      # whole groups per key, so that the direct layout is exact: 16 to 432 codes per key


def direct(keep, g):
    """(waves skipped, quarters without a load, idle quarters of run waves, waves, groups pruned) from the groups themselves."""
    groups = np.repeat(keep, g)
    nw = len(groups) // 64
    q = groups[:nw * 64].reshape(nw, 4, 16).any(axis=2)           # [wave, quarter]: some group keeps
    run = q.any(axis=1)
    return int((~run).sum()), int((~q).sum()), int((~q[run]).sum()), nw, int((~groups[:nw * 64]).sum())


def key_sets():
    rng = np.random.default_rng(2024)
    for p in (0.02, 0.2, 0.5, 0.9):
        yield rng.random(NKEYS) < p                               # iid keys
    runs = np.zeros(NKEYS, bool)                                   # stretches of kept keys, as a key-ordered table gives
    for lo in rng.integers(0, NKEYS - 40, 30):
        runs[lo:lo + rng.integers(1, 40)] = True
    yield runs
    yield np.zeros(NKEYS, bool)
    yield np.ones(NKEYS, bool)


@pytest.mark.parametrize("g", GROUPS_PER_KEY)
def test_quarter_window_equals_a_direct_count(g):
    for keep in key_sets():
        skipped, noload, idle, nw, pruned = direct(keep, g)
        cpk = 16 * g
        assert bp.wave_fraction(keep, cpk) == pytest.approx(skipped / nw, abs=1e-12)
        assert bp.window_fraction(keep, cpk, 64) == bp.wave_fraction(keep, cpk)
        assert bp.quarter_fraction(keep, cpk) == pytest.approx(noload / (4 * nw), abs=1e-12)
        assert bp.quarter_counter_fraction(keep, cpk) == pytest.approx(idle / (4 * nw), abs=1e-12)
        # a skipped wave is four quarters without a load; a quarter without a load is 16 pruned groups
        assert noload == idle + 4 * skipped and 16 * noload <= pruned
        assert bp.wave_fraction(keep, cpk) <= bp.quarter_fraction(keep, cpk) <= bp.group_fraction(keep) + 64 / (NKEYS * g)


def test_quarter_window_on_a_hand_made_layout():
    """16 groups per key: a quarter is one key, a wave four.  Keys 0-3 pruned (a skipped wave), key 5 kept alone in wave 1 (three
    idle quarters), keys 8 and 10 kept in wave 2 (two idle, not adjacent), wave 3 all kept, the rest pruned."""
    keep = np.zeros(64, bool)
    keep[[5, 8, 10, 12, 13, 14, 15]] = True
    assert direct(keep, 16)[:4] == (13, 57, 5, 16)
    assert bp.wave_fraction(keep, 256) == pytest.approx(13 / 16)
    assert bp.quarter_fraction(keep, 256) == pytest.approx(57 / 64)
    assert bp.quarter_counter_fraction(keep, 256) == pytest.approx(5 / 64)
    # 8 groups per key: a quarter is two keys and loads when either keeps
    assert bp.quarter_fraction(keep, 128) == pytest.approx(1 - 5 / 32) and bp.wave_fraction(keep, 128) == pytest.approx(6 / 8)


def test_byte_model_and_the_columns_the_tool_had():
    assert bp.plane_bytes(6, 0.0, 0.0) == pytest.approx(3.1875)
    assert bp.plane_bytes(6, 0.586, 0.001) == pytest.approx(3 * 0.414 + 0.1875 + 0.128)
    # the functions from before this option: values pinned by tests/test_bucket_prune_model.py's hand-made case, again here
    keep = np.ones(1 << 20, bool)
    keep[:16] = False
    keep[8] = True
    nwaves = (1 << 20) * 16 // 64
    assert bp.wave_fraction(keep, 256) == pytest.approx(3 / nwaves)
    assert bp.group_fraction(keep) == pytest.approx(15 / (1 << 20))
    assert bp.quarter_fraction(keep, 256) == pytest.approx(15 / (4 * nwaves))
    assert bp.octaves(int(1e9), 1 << 27) == [128.0, 256.0]
    assert bp.WAVE_GROUPS == 64 and bp.QUARTER_GROUPS == 16
