"""tests/spectral_pass_cases.py held to what it promises, on the oracle alone (no GPU): the frame that the stream run in runs of
equal wavelength leaves is the pass in which visit v is at lam[v] -- its log is list_draw_spectral_cases.expected_log() record
for record --, cutting a stream into ranges changes no bit of what the oracle accumulates, and in every polynomial-optics case
the column changes the pass: a GPU pass that ignored it would fail against these frames."""
import numpy as np
import pytest

import common
import list_draw_spectral_cases as ls
import spectral_pass_cases as sp

# the least number of visits whose records differ between the pass with the column and the scalar pass at lambda_bw, asked
# of every polynomial-optics case
MIN_VISITS_THAT_DIFFER = 5


@pytest.mark.parametrize("case", sp.ALL, ids=sp.IDS)
def test_the_runs_are_the_pass_with_a_wavelength_per_visit(orc, case):
    kind, name, assignment = case
    s = ls.setup(kind, name)
    lam = sp.column(case)
    fr = sp.oracle_frame(orc, case)
    log = common.sort_log(fr.log())
    want = ls.expected_log(orc, kind, name, lam)
    assert log.shape == want.shape and np.array_equal(log, want)
    c = fr.counters()
    assert int(c.visits) == s["n"] and int(c.accepted_draws) == want.shape[0] > 0
    scalar = ls.oracle_pass(orc, kind, name, 0.0)
    assert int(c.redistributed_visits) == scalar["redistributed"]
    listed, differ, attempts = ls.visit_differences(log, scalar["log"])
    print(sp.IDS[sp.ALL.index(case)], "runs", len(sp.runs(lam)), "visits listed", len(listed), "differ from the scalar pass", len(differ))
    if s["camera"] == "tl":
        assert not differ
    else:
        assert len(differ) >= MIN_VISITS_THAT_DIFFER


@pytest.mark.parametrize("kind,name", ls.ALL, ids=ls.IDS)
def test_cutting_a_stream_into_ranges_changes_no_bit(orc, kind, name):
    """one effective wavelength, every visit a range of its own (the column alternates 0 and LAMBDA_BW) against the uncut run"""
    s = ls.setup(kind, name)
    case = (kind, name, "random")
    whole = sp.oracle_frame(orc, case, lam=np.zeros(s["n"]))
    cut = sp.oracle_frame(orc, case, lam=sp.alternating(s["n"]))
    try:
        assert len(sp.runs(sp.alternating(s["n"]))) == s["n"] and len(sp.runs(np.zeros(s["n"]))) == 1
        a, b = whole.log(), cut.log()
        assert a.shape[0] > 0 and np.array_equal(a, b)                               # (in the oracle's own order)
        assert np.array_equal(common.sort_log(a), ls.oracle_pass(orc, kind, name, 0.0)["log"])
        assert np.array_equal(whole.buffer(0).view(np.uint32), cut.buffer(0).view(np.uint32))
        assert np.array_equal(whole.weight().view(np.uint32), cut.weight().view(np.uint32))
        assert np.array_equal(whole.buffer64(0).view(np.uint64), cut.buffer64(0).view(np.uint64))
        assert np.array_equal(whole.weight64().view(np.uint64), cut.weight64().view(np.uint64))
        ca, cb = whole.counters(), cut.counters()
        assert bytes(ca) == bytes(cb) and int(ca.accepted_draws) == a.shape[0]
    finally:
        whole.close()
        cut.close()
