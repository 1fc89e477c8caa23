"""The case table of the LENTIL_DRAWS_CHANNELS tests (tests/list_draw_chroma_cases.py) held to conditions on the oracle alone --
no GPU --, so that no test of tests/test_gpu_list_draws_chroma.py can pass vacuously: what a case is there for must be in the
oracle's draw log of it.
"""
import numpy as np
import pytest

import list_draw_cases as lc
import list_draw_chroma_cases as cc


def _stats(orc, name):
    o, s = cc.oracle_pass(orc, name), cc.setup(name)
    w = cc.walk(o["log"], s["samples"])
    return o, s, w


def test_the_table_is_the_one_the_tests_are_written_for():
    assert cc.ALL == sorted(["pos-16", "neg-16", "one-16", "samples-4", "samples-63", "samples-64", "samples-65", "short-r0",
                             "short-r3", "retries-1", "petzval", "interpreter", "bokeh-image", "blades5-neg", "add-energy"])
    for name in cc.ALL:
        s = cc.setup(name)
        assert s["camera"] == "po" and s["p"].abb_chromatic != 0.0 and s["samples"] > 0 and s["lam"] == 0.0
    assert cc.setup("neg-16")["p"].abb_chromatic < 0 and cc.setup("blades5-neg")["p"].abb_chromatic < 0
    assert cc.setup("one-16")["p"].abb_chromatic == 1.0 and cc.setup("short-r3")["p"].abb_chromatic == 1.0
    assert cc.setup("add-energy")["p"].bidir_add_energy > 0
    assert not [k for k in lc.CASES if k.startswith("chroma:")]                 # nothing stays registered
    assert set(cc.POSITION_CASES) <= set(cc.ALL) and set(cc.OWN_FILM_CASES) <= set(cc.ALL)


@pytest.mark.parametrize("name", cc.ALL)
def test_every_case_obeys_the_counting_rule(orc, name):
    """at most 11 * samples records per visit, all three channels, the counters add up, and the rule count += successes - 2
    walked over a visit's log ends where the log ends"""
    o, s, w = _stats(orc, name)
    S = s["samples"]
    print(name, {k: o[k] for k in ("visits", "redistributed", "attempted", "accepted")})
    assert o["visits"] == s["n"] and o["redistributed"] >= 100 and o["log"].shape[0] == o["accepted"]
    if name == "retries-1":
        assert o["accepted"] == 0 and o["attempted"] == 5 * 16 * o["redistributed"]
        return
    v, n, c = cc.split_log(o["log"])
    assert set(np.unique(c).tolist()) == {0, 1, 2}
    vis, count = np.unique(v, return_counts=True)
    assert count.max() <= 11 * S and n.max() < 5 * S
    last = {int(a): int(b) for a, b in zip(vis, [n[v == x].max() for x in vis])}
    attempts = 0
    for x, (made, low, final, records) in w.items():
        if final >= S:
            assert final == S and last[x] == made - 1, (x, made, final, last[x])
        else:
            assert made == 5 * S and last[x] < made
        assert records == final + 2 * made
        attempts += made
    # (a redistributed visit without a record made all its attempts)
    assert o["attempted"] == attempts + (o["redistributed"] - vis.size) * 5 * S


@pytest.mark.parametrize("name", ["pos-16", "one-16"])
def test_partial_attempts_falling_counts_and_visits_that_run_out(orc, name):
    o, s, w = _stats(orc, name)
    av, an, succ = cc.per_attempt(o["log"])
    ones, twos, threes = (int((succ == k).sum()) for k in (1, 2, 3))
    down = sum(1 for made, low, final, records in w.values() if low < 0)
    ran_out = sum(1 for made, low, final, records in w.values() if final < s["samples"]) + o["redistributed"] - len(w)
    print(name, "attempts with 1 / 2 / 3 successes:", ones, twos, threes, "counts that went down:", down, "ran to 5 * samples:", ran_out)
    assert ones >= 1 and twos >= 1 and threes >= 1
    assert down >= 1 and ran_out >= 1


@pytest.mark.parametrize("name", ["neg-16", "blades5-neg"])
def test_white_channels_land_together(orc, name):
    """abb_chromatic < 0: every logged attempt has three records with one pixel"""
    o = cc.oracle_pass(orc, name)
    log = o["log"]
    v, n, c = cc.split_log(log)
    order = np.lexsort((c, n, v))
    v, n, c, pix = v[order], n[order], c[order], log[order, 2]
    assert log.shape[0] % 3 == 0 and log.shape[0] > 0
    assert np.array_equal(c.reshape(-1, 3), np.tile([0, 1, 2], (log.shape[0] // 3, 1)))
    for a in (v, n, pix):
        a = a.reshape(-1, 3)
        assert (a == a[:, :1]).all()


def test_short_r0_mostly_runs_into_the_attempt_limit(orc):
    o, s, w = _stats(orc, "short-r0")
    ran_out = sum(1 for made, low, final, records in w.values() if final < s["samples"])
    down = sum(1 for made, low, final, records in w.values() if low < 0)
    print("short-r0: visits with records", len(w), "ran to 5 * samples", ran_out, "counts that went down", down)
    assert ran_out > len(w) / 2


def test_short_r3_reaches_the_bound(orc):
    o, s, w = _stats(orc, "short-r3")
    most = max(records for made, low, final, records in w.values())
    print("short-r3: most records of one visit", most)
    assert most == 11 * s["samples"]


def test_samples_64_ends_on_the_slab_boundary(orc):
    v, n, c = cc.split_log(cc.oracle_pass(orc, "samples-64")["log"])
    assert n.max() == 5 * 64 - 1
