"""The table of retry cases (tests/retry_cases.py) against the oracle alone -- no GPU: what keeps tests/test_gpu_retries.py
from passing emptily.

A case whose accepted draws are all first tries says nothing about how a walker counts tries, and two retry counts with the
same oracle list cannot tell a walker that stops one try early from one that does not.  So: every case accepts draws (but
the one that must not), every list at R > 0 differs from the same stream's at R = 0 -- some accepted draw is a retry --, and
around the LDS window's limit the neighbours' lists are pairwise different for each of the three walkers.  The oracle's
runs are shared with one another here (retry_cases.oracle: once per stream and retry count)."""
import itertools

import numpy as np
import pytest

import common
import retry_cases as rc

PO_CASES = [c for c in rc.CASES if c["family"] != "negative"]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def test_the_window_constant_is_the_one_the_cases_stand_around():
    with open(common.ROOT + "/pota_amd/csrc/lentil_kernels.h") as f:
        assert "constexpr uint32_t kAcceptWinRetries = %d;" % rc.WIN in f.read()
    for fam in ("base", "aov16", "chroma", "lean"):
        have = set(c["R"] for c in rc.named(fam))
        assert {rc.WIN, rc.WIN + 1} <= have, (fam, sorted(have))
    assert rc.WIN - 1 in set(c["R"] for c in rc.named("base"))
    # the widths new to the wide walker run with the window full
    assert all(rc.WIN in set(c["R"] for c in rc.named("wide-g%d" % g)) for g in (5, 6, 7, 8, 12))


@pytest.mark.parametrize("case", PO_CASES, ids=rc.ids(PO_CASES))
def test_case_accepts_draws_and_some_are_retries(orc, case):
    ref = rc.oracle(orc, case)
    k = ref.counters()
    assert k.redistributed_visits > 50 and k.accepted_draws > 0 and k.attempted_draws > 0
    if case["chroma"] == 0.0:
        assert k.accepted_draws <= k.attempted_draws
    if case["R"] > 0:
        first_tries_only = rc.oracle(orc, case, R=0)
        assert first_tries_only.counters().redistributed_visits == k.redistributed_visits
        assert not _same(rc.sorted_log(ref), rc.sorted_log(first_tries_only)), "no accepted draw of this case is a retry"


def test_base_shape_is_the_one_described(orc):
    """234 redistributed visits; one attempt less per retry around the window's limit"""
    by_r = {c["R"]: rc.oracle(orc, c).counters() for c in rc.named("base") if c["lens_mode"] == 0}
    assert all(k.redistributed_visits == 234 for k in by_r.values())
    assert by_r[63].attempted_draws > by_r[64].attempted_draws > by_r[65].attempted_draws


@pytest.mark.parametrize("family", sorted(rc.BOUNDARY))
def test_neighbours_of_the_window_limit_differ(orc, family):
    stream = rc.named(family)[0]          # (the family's cases differ in R alone; 63 is not always one of them)
    logs = {R: rc.sorted_log(rc.oracle(orc, stream, R=R)) for R in rc.BOUNDARY[family]}
    for a, b in itertools.combinations(rc.BOUNDARY[family], 2):
        assert not _same(logs[a], logs[b]), "%s: the oracle's lists at %d and %d retries are the same" % (family, a, b)


def test_all_base_lists_differ(orc):
    cases = [c for c in rc.named("base") if c["lens_mode"] == 0]
    logs = [rc.sorted_log(rc.oracle(orc, c)) for c in cases]
    for (ca, a), (cb, b) in itertools.combinations(zip(cases, logs), 2):
        assert not _same(a, b), (ca["name"], cb["name"])


def test_no_try_at_all(orc):
    """vignetting_retries < 0: `tries <= vignetting_retries` (src/lentil.h:592) never holds -- every redistributed visit uses up
    its 5 x samples attempts, nothing is accepted, and those visits add nothing to the frame."""
    (case,) = rc.named("negative")
    ref = rc.oracle(orc, case)
    k = ref.counters()
    assert (k.redistributed_visits, k.attempted_draws, k.accepted_draws) == (234, 234 * 5 * case["S"], 0)
    assert ref.log().shape[0] == 0
    # the frame: the visits that stay in their pixel, and those alone -- the same stream with no highlight redistributed has them
    zero = rc.oracle(orc, rc.BY_NAME["base-r0"])
    assert zero.counters().visits == k.visits
    untouched = zero.weight() == ref.weight()
    assert untouched.mean() > 0.5 and np.array_equal(zero.buffer(0)[untouched], ref.buffer(0)[untouched])
    assert float(ref.weight().sum()) < float(zero.weight().sum())


def test_thin_lens_ignores_the_parameter(orc):
    runs = []
    for R in rc.THIN_R:
        p = common.tl_setup(64, 40, samples_override=32, vignetting_retries=R)
        visits, cols = common.make_stream(p, 64, 40, 9, f_hi=0.01)
        ref = common.run_oracle(orc, p, None, visits)
        k = ref.counters()
        runs.append(((k.redistributed_visits, k.attempted_draws, k.accepted_draws), rc.sorted_log(ref)))
        ref.close()
    assert runs[0][0][2] > 0
    assert all(r[0] == runs[0][0] and _same(r[1], runs[0][1]) for r in runs[1:])
