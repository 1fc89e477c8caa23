"""tests/spectral_cases.py held to its purpose, on the oracle alone (no GPU).

A spectral batch is worth testing only where the wavelength matters: where it moves the results, and where it decides
whether a ray or a query retries, so that the lanes of one wave -- each with a wavelength of its own in the camera-rays
kernel -- disagree about going round the retry loop again.  Every polynomial-optics case is traced here at two of its own
wavelengths (its smallest and its largest) and must show, between the two:
  - at least 90 % of its rays (any of the 21 words or the try count) or queries (the sensor position, the try count or
    whether it got through) differ;
  - at least one ray or query has a different try count;
and, at the wavelengths it is run with, at least one ray or query retries.

The enable_dof = 0 ray cases cannot show the second: without depth of field a try starts on the axis' direction, so what
stops it is the inner-pupil test on the sensor position alone, which reads no polynomial -- over 2601 radii from the centre
to 1.3 half-widths, at two angles, every shipped lens vignettes at the same radius at 0.40 and at 0.70 um (double gauss
0.6015, both Petzvals 0.4745 ... 0.4750 half-widths).  No input makes their try counts depend on the wavelength; they are
held to the other two conditions (every try of a vignetted ray repeats the first, so "retries" is all-or-nothing there).
"""
import numpy as np
import pytest

import spectral_cases as sc

MIN_MOVED = 0.90


@pytest.mark.parametrize("name", sc.RAY_CASES)
def test_ray_cases_depend_on_the_wavelength(orc, name):
    (out_a, tries_a), (out_b, tries_b) = sc.oracle_ray_pair(orc, name)
    out, tries = sc.oracle_ray_case(orc, name)
    moved = (out_a.view(np.uint32) != out_b.view(np.uint32)).any(1) | (tries_a != tries_b)
    print("%s: %d rays, %.1f %% differ between %.3f and %.3f um, try counts of %d differ, %d retry" % (
        name, moved.size, 100.0 * moved.mean(), *sc.ray_setup(name)["pair"], int((tries_a != tries_b).sum()), int((tries > 0).sum())))
    assert moved.mean() >= MIN_MOVED
    if sc.ray_setup(name)["p"].enable_dof:
        assert (tries_a != tries_b).any()
    assert (tries > 0).any()
    # and the case is neither of the two: its own wavelengths give a third result
    assert not np.array_equal(out.view(np.uint32), out_a.view(np.uint32)) and not np.array_equal(out.view(np.uint32), out_b.view(np.uint32))


@pytest.mark.parametrize("name", sc.POINT_CASES)
def test_point_cases_depend_on_the_wavelength(orc, name):
    a, b = sc.oracle_point_pair(orc, name)
    own = sc.oracle_point_case(orc, name)
    with np.errstate(invalid="ignore"):
        moved = (a["ok"] != b["ok"]) | (a["tries"] != b["tries"]) | (a["sensor"].view(np.uint64) != b["sensor"].view(np.uint64)).any(-1)
    print("%s: %d queries, %.1f %% differ, try counts of %d differ, %d retry" % (
        name, moved.size, 100.0 * moved.mean(), int((a["tries"] != b["tries"]).sum()), int((own["tries"] > 0).sum())))
    assert moved.mean() >= MIN_MOVED
    assert (a["tries"] != b["tries"]).any()
    assert (own["tries"] > 0).any()


def test_the_wavelengths_are_what_the_oracles_take():
    assert all(0.40 <= lam <= 0.70 for lam in sc.ray_lambdas(sc.N_RAYS))
    lam = sc.float32_lambdas(64, 1)
    assert np.array_equal(lam, lam.astype(np.float32).astype(np.float64)) and np.unique(lam).size == 64
    assert len(set(sc.LAM_PALETTE)) == 3
