"""tests/list_draw_probe_cases.py held to what its cases are there for, on the oracle alone (no GPU): in every case the
sphere bites -- some but not all of the segments the oracle asks about are occluded, and the draw log under the probe differs
from the free one -- and the highlights' world positions are pairwise distinct, which the GPU test's "no segment asked
twice" relies on (a segment's origin names its visit).  The oracle's passes are cached per process."""
import numpy as np
import pytest

import list_draw_probe_cases as pc


@pytest.mark.parametrize("name", pc.ALL)
def test_the_sphere_bites(orc, name):
    s = pc.setup(name)
    probed, free = pc.oracle_pass(orc, name), pc.oracle_pass(orc, name, probed=False)
    assert probed["redistributed"] == free["redistributed"] > 0
    pos = s["cols"]["pos_z"][s["highlights"], :3]
    assert np.unique(pos.view(np.uint32), axis=0).shape[0] == pos.shape[0]
    answers = probed["answers"]
    print(name, "asked", answers.size, "occluded", int(answers.sum()), "draws", probed["accepted"], "free", free["accepted"],
          "attempts", probed["attempted"], "free", free["attempted"])
    if name == "retries-1":
        # no try is made: nothing is asked, nothing is drawn, every visit makes its 5 * samples attempts
        assert answers.size == 0 and probed["accepted"] == 0 and probed["attempted"] == 5 * s["samples"] * probed["redistributed"]
        return
    assert 0 < int(answers.sum()) < answers.size
    assert probed["log"].shape != free["log"].shape or not np.array_equal(probed["log"], free["log"])
    assert probed["attempted"] > free["attempted"]            # (an occluded try costs the visit a try or an attempt)
    # every origin is a highlight's world position, bit for bit
    org = np.unique(probed["segments"][:, :3].view(np.uint32), axis=0)
    hi = {r.tobytes() for r in pos.view(np.uint32)}
    assert all(r.tobytes() in hi for r in org)


def test_swallowed_visits_make_every_attempt_and_list_nothing(orc):
    s = pc.setup("swallowed")
    probed, free = pc.oracle_pass(orc, "swallowed"), pc.oracle_pass(orc, "swallowed", probed=False)
    gone = np.setdiff1d(np.unique(free["log"][:, 0]), np.unique(probed["log"][:, 0]))
    assert gone.size > 0
    # all their segments are occluded
    pos = s["cols"]["pos_z"][:, :3].view(np.uint32)
    seg = probed["segments"][:, :3].view(np.uint32)
    for v in gone[:8]:
        mine = (seg == pos[v]).all(axis=1)
        assert mine.any() and probed["answers"][mine].all()


def test_skydome_samples_are_redistributed_and_never_asked_about(orc):
    s = pc.setup("skydome")
    probed = pc.oracle_pass(orc, "skydome")
    sky = s["skydome"]
    assert sky.size > 0
    drawn = np.intersect1d(np.unique(probed["log"][:, 0]), sky)
    assert drawn.size > 0                                       # the oracle redistributes some of them
    pos = s["cols"]["pos_z"][:, :3].view(np.uint32)
    org = {r.tobytes() for r in np.unique(probed["segments"][:, :3].view(np.uint32), axis=0)}
    assert not any(pos[v].tobytes() in org for v in sky)        # ... and asks about none
    # a skydome sample's substitute position is its direction times 99999999: no origin is that either
    assert np.abs(probed["segments"][:, :3]).max() < 1e6
