"""The table of device-probe cases (tests/probe_device_cases.py) against the oracle alone -- no GPU: what keeps
tests/test_gpu_probe_device.py from passing emptily.

A sphere that occludes nothing, or everything, or a stream whose accepted draws are the same with and without it, cannot tell a
library that honours the renderer's answers from one that drops them.  So every case but the three degenerate ones is held to:
the sphere occludes some of the segments the oracle asks about and not all (counted by a CFUNCTYPE wrapper around the oracle's
sphere occluder), and the oracle's probed accepted-draw list differs from its unprobed one.  The degenerate cases are held to
what makes them degenerate.  The oracle's runs are shared (probe_device_cases.oracle: once per case and kind of run)."""
import numpy as np
import pytest

import probe_device_cases as pc


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("case", pc.PARITY, ids=pc.ids(pc.PARITY))
def test_the_sphere_bites(orc, case):
    counted, free = pc.oracle(orc, case, "counted"), pc.oracle(orc, case, "free")
    k = counted.counting
    assert 0 < k.occluded < k.probed, (k.occluded, k.probed)
    assert not _same(pc.sorted_log(counted), pc.sorted_log(free)), "the probed list is the unprobed one"
    assert counted.counters().redistributed_visits == free.counters().redistributed_visits > 100


def test_the_degenerate_cases_are_degenerate(orc):
    none = pc.oracle(orc, pc.BY_NAME["no-highlights"], "counted")
    assert none.counting.probed == 0 and none.counters().redistributed_visits == 0
    zero = pc.oracle(orc, pc.BY_NAME["radius-0"], "counted")
    assert zero.counting.probed > 1000 and zero.counting.occluded == 0
    assert _same(pc.sorted_log(zero), pc.sorted_log(pc.oracle(orc, pc.BY_NAME["radius-0"], "free")))
    # (every try of every attempt is asked about and lost: millions of calls -- not through the counting wrapper)
    every = pc.oracle(orc, pc.BY_NAME["lens-swallowed"], "probed")
    assert every.counters().accepted_draws == 0 and every.counters().redistributed_visits > 100
    assert pc.oracle(orc, pc.BY_NAME["lens-swallowed"], "free").counters().accepted_draws > 1000


def test_the_table_is_the_one_described():
    assert {c["camera"] for c in pc.PARITY} == {"po", "tl", "tlc"}
    assert pc.BY_NAME["overflow"]["env"] == {"LENTIL_PROBE_DEVICE_CAP": "64"}
    assert pc.BY_NAME["sub-batches"]["env"] == {"LENTIL_MAX_POOL_UNITS": "20000", "LENTIL_CHUNKS": "5"} and pc.BY_NAME["sub-batches"]["S"] == 64
    assert all(c["sphere"] == pc.SPHERE for c in pc.PARITY)
    assert [c["name"] for c in pc.CASES if c["exempt"]] == ["no-highlights", "radius-0", "lens-swallowed"]
