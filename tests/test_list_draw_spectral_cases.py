"""tests/list_draw_spectral_cases.py held to what its cases are there for, on the oracle alone (no GPU): in every
polynomial-optics case the wavelength changes what is listed -- between 0.45 and 0.65 at least a quarter of the listed visits
differ in their accepted attempts or in a pixel, and where vignetting decides (retries0, short-po) at least one visit in ten
differs in which attempts are accepted --, all four palette entries occur among the redistributed visits, some 64-visit
group holds redistributed neighbours with different wavelengths, and some visit with entry 0 has records.  The oracle's
passes are cached per process."""
import numpy as np
import pytest

import list_draw_cases as lc
import list_draw_spectral_cases as ls

# where no retry hides a vignetted try, the wavelength decides which attempts are accepted
ATTEMPT_CASES = (("plain", "retries0"), ("plain", "short-po"), ("probed", "retries0"))


@pytest.mark.parametrize("kind,name", ls.ALL, ids=ls.IDS)
def test_the_wavelength_bites(orc, kind, name):
    s = ls.setup(kind, name)
    assert tuple(s["frame"]) in ls.FRAMES and float(s["p"].lambda_bw) == ls.LAMBDA_BW != float(np.float32(0.55))
    lam = ls.lambdas(kind, name)
    blocks = ls.lambdas(kind, name, "blocks")
    c1, c2 = ls.cuts(s["n"])
    assert lam.shape == blocks.shape == (s["n"],) and set(np.unique(lam)) == set(ls.PALETTE)
    assert (blocks[:c1] == ls.BLOCKS[0]).all() and (blocks[c1:c2] == ls.BLOCKS[1]).all() and (blocks[c2:] == ls.BLOCKS[2]).all()
    blue, red = ls.oracle_pass(orc, kind, name, ls.LAM_BLUE), ls.oracle_pass(orc, kind, name, ls.LAM_RED)
    assert blue["redistributed"] == red["redistributed"] > 0
    if s["camera"] == "tl":
        # the thin lens reads no wavelength: one pass is every pass
        assert blue is red and ls.expected_log(orc, kind, name, lam) is not None
        assert np.array_equal(ls.expected_log(orc, kind, name, lam), blue["log"])
        return
    listed, differ, attempts = ls.visit_differences(blue["log"], red["log"])
    print(kind, name, "listed", len(listed), "differ", len(differ), "in their accepted attempts", len(attempts),
          "draws blue / red", blue["accepted"], red["accepted"])
    assert 4 * len(differ) >= len(listed) > 0
    if (kind, name) in ATTEMPT_CASES:
        assert 10 * len(attempts) >= len(listed)

    # the assignment: every palette entry among the redistributed visits, different neighbours within a 64-visit group, and
    # records at entry 0 -- which are the pass's at LAMBDA_BW, not at the default wavelength
    want = ls.expected_log(orc, kind, name, lam)
    red_visits = np.nonzero(s["highlights"])[0]
    drawn = np.unique(np.concatenate([ls.oracle_pass(orc, kind, name, v)["log"][:, 0] for v in ls.PALETTE]))
    assert np.isin(drawn, red_visits).all()
    assert set(np.unique(lam[drawn])) == set(ls.PALETTE)
    group = drawn // 64
    neighbours = (group[1:] == group[:-1]) & (lam[drawn][1:] != lam[drawn][:-1])
    assert neighbours.any()
    at_zero = want[lam[want[:, 0]] == 0.0]
    assert at_zero.shape[0] > 0
    bw = ls.oracle_pass(orc, kind, name, 0.0)["log"]
    assert np.array_equal(at_zero, bw[lam[bw[:, 0]] == 0.0])
    # ... and the list is no single pass's
    for v in ls.PALETTE:
        one = ls.oracle_pass(orc, kind, name, v)["log"]
        assert one.shape != want.shape or not np.array_equal(one, want)
    # the blocks assignment puts records into each of its three sub-ranges
    wb = ls.expected_log(orc, kind, name, blocks)
    assert (wb[:, 0] < c1).any() and ((wb[:, 0] >= c1) & (wb[:, 0] < c2)).any() and (wb[:, 0] >= c2).any()


@pytest.mark.parametrize("kind,name", [("plain", "samples-65"), ("plain", "short-po"), ("probed", "swallowed")])
def test_attempts_per_visit_add_up_to_the_oracles_counter(orc, kind, name):
    """attempts_per_visit, which the GPU test sums per wavelength, against the oracle's own attempted_draws of every pass: the
    redistributed visits are the stream's highlights here, their draw count the case's samples_override"""
    s = ls.setup(kind, name)
    red = np.nonzero(s["highlights"])[0]
    assert s["samples"] > 0
    for v in ls.PALETTE:
        o = ls.oracle_pass(orc, kind, name, v)
        assert o["redistributed"] == red.size
        made = ls.attempts_per_visit(o["log"], red, np.full(red.size, s["samples"]))
        assert int(made.sum()) == o["attempted"]
        assert (made <= 5 * s["samples"]).all() and (made > 0).all()
