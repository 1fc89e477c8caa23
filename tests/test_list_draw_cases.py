"""The case table of the lentil_hip_list_draws tests (tests/list_draw_cases.py) held to conditions on the oracle alone -- no
GPU --, so that no test of tests/test_gpu_list_draws.py can pass vacuously: what a case is there for must be in the oracle's
draw log of it.
"""
import numpy as np
import pytest

import list_draw_cases as lc
from pota_amd import _abi


def test_the_table_is_the_one_the_tests_are_written_for():
    assert lc.SAMPLES_N == (4, 16, 63, 64, 65, 130, 200)
    assert [lc.CASES["samples-%d" % s]["samples"] for s in lc.SAMPLES_N] == list(lc.SAMPLES_N)
    assert sorted(lc.CASES["retries%d" % r]["params"]["vignetting_retries"] for r in (-1, 0, 3, 15)) == [-1, 0, 3, 15]
    assert lc.CASES["formula"]["samples"] == 0 and lc.CASES["ragged"]["samples"] == 0
    for c in lc.CASES.values():
        w, h = c["frame"]
        assert 32 <= w <= 96 and 24 <= h <= 64 and 0.02 <= c["f_hi"] <= 0.05
    assert [lc.CASES[n]["path"] for n in lc.LENS_CASES] == [
        _abi.DRAWS_PATH_COMPILED_IN, _abi.DRAWS_PATH_COMPILED_IN, _abi.DRAWS_PATH_INTERPRETER, _abi.DRAWS_PATH_INTERPRETER]
    assert lc.CASES["tl-plain"]["path"] == _abi.DRAWS_PATH_THIN_LENS
    assert lc.setup("lens-anamorphic")["table"].lens_outer_pupil_geometry != _abi.GEOM_SPHERICAL
    assert lc.setup("lambda")["p"].lambda_bw != lc.setup("lambda")["p_oracle"].lambda_bw
    assert lc.setup("ragged")["visits"].visits_per_pixel == 0 and lc.setup("moving-camera")["keys"].shape == (2, 4, 4)


@pytest.mark.parametrize("name", lc.ALL)
def test_every_case_accepts_draws(orc, name):
    """... except the one that makes no try at all; and its counters add up"""
    o, s = lc.oracle_pass(orc, name), lc.setup(name)
    print(name, {k: o[k] for k in ("visits", "redistributed", "attempted", "accepted")})
    assert o["visits"] == s["n"] and o["redistributed"] >= 100 and o["log"].shape[0] == o["accepted"]
    if name == "retries-1":
        assert o["accepted"] == 0 and o["attempted"] == 5 * s["samples"] * o["redistributed"]
        return
    assert o["accepted"] >= 1000 and o["attempted"] > o["accepted"]
    assert int(o["log"][:, 1].max()) < (1 << 30)                       # no channel bits: neither chromatic mode
    vis, count, last, contiguous = lc.per_visit(o["log"])
    if s["samples"]:
        assert count.max() == s["samples"] and last.max() < 5 * s["samples"]


def test_a_full_visit_with_a_gap_in_its_attempts(orc):
    """(a): visits with exactly `samples` records whose attempt numbers are not contiguous -- dozens where tries are scarce
    or the lens vignettes"""
    found = {}
    for name in lc.ALL:
        s = lc.setup(name)
        if not s["samples"] or name == "retries-1":
            continue
        vis, count, last, contiguous = lc.per_visit(lc.oracle_pass(orc, name)["log"])
        found[name] = int(((count == s["samples"]) & ~contiguous).sum())
    print(found)
    assert sum(found.values()) >= 100
    for name in ("retries0", "retries3", "short-po", "short-tl", "tl-coma-vignetting", "lens-petzval", "lens-anamorphic"):
        assert found[name] >= 10, (name, found[name])


@pytest.mark.parametrize("name", ["short-po", "short-tl"])
def test_short_cases_run_into_the_attempt_limit(orc, name):
    """(b): redistributed visits with fewer than `samples` records (they ran into 5 * samples) and visits with all of them"""
    o, s = lc.oracle_pass(orc, name), lc.setup(name)
    vis, count, last, contiguous = lc.per_visit(o["log"])
    short, full = int((count < s["samples"]).sum()), int((count == s["samples"]).sum())
    none = o["redistributed"] - vis.size                                # visits without a single record
    print(name, "short", short, "full", full, "none", none)
    assert short >= 10 and full >= 10 and none >= 10
    # a visit is short only because it made all 5 * samples attempts
    assert o["attempted"] >= (short + none) * 5 * s["samples"] + full * s["samples"]


def test_the_slab_boundary_streams_differ(orc):
    """(c): samples_override 63, 64 and 65 give pairwise different lists"""
    logs = [lc.oracle_pass(orc, "samples-%d" % s)["log"] for s in (63, 64, 65)]
    for i in range(3):
        for j in range(i + 1, 3):
            assert logs[i].shape != logs[j].shape or not np.array_equal(logs[i], logs[j])
    # ... and 5 * samples is no multiple of 64 where the table says so
    assert (5 * 63) % 64 and (5 * 65) % 64 and (5 * 130) % 64 and (5 * 200) % 64 and not (5 * 64) % 64


def test_the_formula_case_straddles_a_slab(orc):
    """(d): draw counts below and above 64, and the log has as many records as the formula says for the visits that got
    all their draws"""
    vis, samples = lc.formula_samples(orc, "formula")
    print("formula: draw counts", int(samples.min()), "...", int(samples.max()))
    assert (samples < 64).sum() >= 20 and (samples > 64).sum() >= 20 and np.unique(samples).size >= 20
    lvis, count, last, contiguous = lc.per_visit(lc.oracle_pass(orc, "formula")["log"])
    assert np.isin(lvis, vis).all()
    want = samples[np.searchsorted(vis, lvis)]
    assert (count <= want).all() and (count == want).mean() > 0.9


def test_the_variants_change_the_lists(orc):
    """a sampler, a unit, a wavelength or a camera motion that left the oracle's list as it is would test nothing"""
    base = lc.oracle_pass(orc, "retries15")["log"]                      # samples 16, the default everything
    for name in ("moving-camera", "lambda", "retries3", "retries0"):
        other = lc.oracle_pass(orc, name)["log"]
        assert other.shape != base.shape or not np.array_equal(other, base), name
    # the two units restate the centimetre scene: the same visits are redistributed
    for name in ("unit-mm", "unit-m"):
        assert lc.oracle_pass(orc, name)["redistributed"] == lc.oracle_pass(orc, "retries15")["redistributed"]
    s = lc.setup("add-energy")
    assert s["p"].bidir_add_energy > 0
