"""tests/trace_point_probe_cases.py against the oracle alone (no GPU): the seed-by-seed model of its five small cases
reproduces the oracle's probed pass, and the sphere bites -- conditions on the inputs of tests/test_gpu_trace_points_probed.py,
so that what the kernel is compared with is the reference's behaviour and is not trivially unoccluded."""
import numpy as np
import pytest

import list_draw_probe_cases as pc
import trace_point_probe_cases as tpc


@pytest.mark.parametrize("name", tpc.ORACLE_MODEL)
def test_the_model_reproduces_the_oracles_probed_log(orc, name):
    want = pc.oracle_pass(orc, name)
    b, o = tpc.batch(name), tpc.oracle_model(orc, name)
    assert b["visits"].size == want["redistributed"] and o["k"] == 5 * pc.setup(name)["samples"]
    inside = o["pixel"] < tpc.OUTSIDE
    made = tpc.made(inside, b["samples"])
    below = np.arange(o["k"])[None, :] < made[:, None]
    at = np.nonzero(inside & below)
    got = np.stack([b["visits"][at[0]], at[1]], axis=1).astype(np.uint32)
    log = want["log"]
    # the logged attempts are exactly the queries below the attempts made whose passing seed lands in the frame ...
    assert got.shape == log[:, :2].shape and np.array_equal(got, log[:, :2])
    assert int(made.sum()) == want["attempted"]
    # ... and they land where the log says (the pixel is the log's; the model's mapping is tests/trace_point_cases.py's)
    m_made, landed = tpc.made_from_log(log, b["visits"], b["samples"])
    assert np.array_equal(m_made, made)
    assert np.array_equal(landed[at], o["pixel"][at]) and np.array_equal(landed[at], log[:, 2])


@pytest.mark.parametrize("name", tpc.ORACLE_MODEL)
def test_the_sphere_bites(orc, name):
    b, o = tpc.batch(name), tpc.oracle_model(orc, name)
    k = o["k"]
    assert (o["tries"] >= o["free_tries"]).all()
    # without the sphere the walk is orc_trace_ray_bw_po's own
    free = tpc.walk(o["passes"], np.zeros_like(o["occ"]), k, o["retries"])
    assert np.array_equal(free["tries"], o["free_tries"])
    asked, occ = o["asked"], o["occ"]
    assert asked.any()
    share = occ[asked].mean()
    made = tpc.made(o["pixel"] < tpc.OUTSIDE, b["samples"])
    below = np.arange(k)[None, :] < made[:, None]
    if name == "no-dof":
        # every seed of a point has the aperture point (0, 0): a point is occluded as a whole or not at all
        assert np.array_equal(occ.all(axis=1), occ.any(axis=1)) and 0 < occ[:, 0].sum() < occ.shape[0]
    else:
        assert 0.0 < share < 1.0
    if name == "retries3":
        assert (o["tries"] > o["free_tries"]).any()
    if name == "swallowed":
        assert ((o["hit"] < 0) | ~below).all(axis=1).any()          # some point: no query of its made range gets through
    print(name, "points", b["visits"].size, "k", k, "asked", int(asked.sum()), "occluded share %.3f" % share)
