"""The draw pass across vignetting_retries, on both sides of kAcceptWinRetries = 64 (tests/retry_cases.py has the cases and
says which code each of them selects; tests/test_retry_cases.py checks the table against the oracle alone).

Every pass against the oracle on the same stream, at the project's own bars: accepted-draw lists bit for bit, the counters
(redistributed visits, attempted draws, accepted draws) equal, the frame within 1e-5 (check_frame); with abb_chromatic the
2e-5 bars of test_po_chromatic_aberration.  The oracle's frames are computed once per stream and retry count and shared.
"""
import numpy as np
import pytest

import common
import oracle_lib
import retry_cases as rc
from pota_amd import capi
from test_gpu_parity import TOL, check_frame, check_logs, gpu_run
from test_gpu_probe import _run_gpu as probe_run

pytestmark = pytest.mark.gpu


def _counters(c):
    return (c.redistributed_visits, c.attempted_draws, c.accepted_draws)


def _check_chroma_frame(ctx, ref):
    """test_po_chromatic_aberration's bars (kinds [0, 0, 1]): three splats per attempt -- buffers and weight within 2e-5 of the
    exact sums, the resolved image within twice that of the exact quotient, the closest AOV exact"""
    tol = 2 * TOL
    w64 = ref.weight64()
    for a in (0, 1):
        buf, w = ctx.download_accum(a)
        exact = ref.buffer64(a)
        m = exact != 0
        assert np.array_equal(buf != 0, ref.buffer(a) != 0)
        assert float(np.max(np.abs(buf[m] - exact[m]) / np.abs(exact[m]))) < tol
        eimg = np.where(w64[:, None] != 0, exact / np.where(w64 != 0, w64, 1.0)[:, None], exact)
        img = ctx.download_aov(a)
        mi = eimg != 0
        assert float(np.max(np.abs(img[mi] - eimg[mi]) / np.abs(eimg[mi]))) < 2 * tol
    mw = w64 != 0
    assert float(np.max(np.abs(ctx.download_accum(0)[1][mw] - w64[mw]) / w64[mw])) < tol
    buf, _ = ctx.download_accum(2)
    assert np.array_equal(buf, ref.buffer(2))


def _check_pass(ctx, ref, case, c):
    assert _counters(c) == _counters(ref.counters()), (_counters(c), _counters(ref.counters()))
    check_logs(ctx, ref)
    if case["chroma"] != 0.0:
        chan = ctx.draw_log()[:, 1] >> 30
        assert set(np.unique(chan)) == {0, 1, 2}
        _check_chroma_frame(ctx, ref)
        return
    kinds = case["kinds"]
    check_frame(ctx, ref, n_aovs=rc.n_aovs(case), kinds=kinds)
    for a, kind in enumerate(kinds or []):
        if kind == 1:                       # closest: exact, as in test_closest_filter_aovs
            buf, _ = ctx.download_accum(a)
            assert np.array_equal(buf, ref.buffer(a))
            img = ctx.download_aov(a)
            assert np.array_equal(img, ref.resolve(a))
            assert np.all(img[buf.any(axis=1), 3] == 1.0)


def _first_pass(orc, ctx, case):
    p, table, visits, keep = rc.setup(case)
    ref = rc.oracle(orc, case)
    c = gpu_run(ctx, p, table, visits, n_aovs=rc.n_aovs(case), kinds=case["kinds"], lens_mode=case["lens_mode"])
    assert c.streamed == 0
    _check_pass(ctx, ref, case, c)


ACROSS = rc.named("base", "base-coc", "petzval")


@pytest.mark.parametrize("case", ACROSS, ids=rc.ids(ACROSS))
def test_pass_across_retry_counts(orc, gpu_ctx_factory, case):
    """accept_item_wide with the window growing to its limit (R <= 64: the last attempt of a step reads win[my_i + R]), then
    accept_item reading global memory (R > 64) -- chosen for the retry count alone, the record being five floats."""
    _first_pass(orc, gpu_ctx_factory(), case)


NARROW = rc.named("aov16")


@pytest.mark.parametrize("case", NARROW, ids=rc.ids(NARROW))
def test_narrow_walker_on_both_sides_of_the_window(orc, gpu_ctx_factory, case):
    """sixteen gaussian AOVs: accept_item whatever the count -- nothing staged beyond the step's own 256 at R = 0, the window
    full at 64, every try from global memory at 65"""
    _first_pass(orc, gpu_ctx_factory(), case)


CHROMA = rc.named("chroma", "chroma-neg")


@pytest.mark.parametrize("case", CHROMA, ids=rc.ids(CHROMA))
def test_chromatic_walker_on_both_sides_of_the_window(orc, gpu_ctx_factory, case):
    """accept_item_chroma: three windows of 256 + R at R <= 64, three chains of global reads above"""
    _first_pass(orc, gpu_ctx_factory(), case)


WIDTHS = rc.named(*["wide-g%d" % g for g in (5, 6, 7, 8, 12)]) + rc.named("mixed-a", "mixed-b")


@pytest.mark.parametrize("case", WIDTHS, ids=rc.ids(WIDTHS))
def test_wide_walker_record_widths(orc, gpu_ctx_factory, case):
    """accept_item_wide's lanes serve 64 / U draws per instruction, U = 4 G + 1 for G gaussian AOVs: 3 draws at G = 5 (63
    lanes), 2 at 6 and 7, 1 at 8 and 12; closest AOVs among them take no lanes and compare bit for bit"""
    _first_pass(orc, gpu_ctx_factory(), case)


STREAMED = rc.named("streamed")


@pytest.mark.parametrize("case", STREAMED, ids=rc.ids(STREAMED))
def test_streamed_passes(orc, case):
    """second and third pass of a context: streamed -- publish_kernel sizes the first batches from the count, the first accept
    runs beside the second round's solves"""
    p, table, visits, keep = rc.setup(case)
    ref = rc.oracle(orc, case)
    ctx = capi.Context(0)
    try:
        for k in range(3):
            c = gpu_run(ctx, p, table, visits)
            assert c.streamed == (1 if k else 0), (k, ctx.last_redo_note())
            assert c.fallback_chunks == 0
            _check_pass(ctx, ref, case, c)
    finally:
        ctx.close()


LEAN = rc.named("lean")


@pytest.mark.parametrize("case", LEAN, ids=rc.ids(LEAN))
def test_lean_pass_on_both_sides_of_the_window(orc, monkeypatch, case):
    """First batches from the model (LENTIL_PREDICT=1), no second round in flight: at 64 retries the first accept is
    accept_kernel<3> (items whose parked solves are through, whole), at 65 ready_accept is false for the count alone and the
    pass runs accept_kernel<1> and <2>.  The passes that ran lean and kept it report one round."""
    monkeypatch.setenv("LENTIL_PREDICT", "1")
    p, table, visits, keep = rc.setup(case)
    ref = rc.oracle(orc, case)
    ctx = capi.Context(0)
    try:
        kept = []
        for k in range(4):
            before = ctx.batch_model_stats()
            c = gpu_run(ctx, p, table, visits)
            after = ctx.batch_model_stats()
            rounds = ctx.last_launches()[1]
            print("pass %d: streamed %d rounds %d model %s" % (k, c.streamed, rounds, after))
            assert c.streamed == (1 if k else 0), (k, ctx.last_redo_note())
            _check_pass(ctx, ref, case, c)
            if after[1] > before[1] and after[2] == before[2]:
                kept.append(rounds)
        built, lean, lost, margin = ctx.batch_model_stats()
        assert built == 1 and lean >= 1, (built, lean, lost, margin)
        assert kept and all(r == 1 for r in kept), (kept, lean, lost)
    finally:
        ctx.close()


PROBE = rc.named("probe")


@pytest.mark.parametrize("case", PROBE, ids=rc.ids(PROBE))
def test_occluded_tries_cost_retries(orc, case):
    """an occluded try is a failed one: with R = 0 it ends the attempt, with 65 the walk goes on through global memory"""
    p, table, visits, keep = rc.setup(case)
    ref = rc.oracle(orc, case)
    sphere = np.array(rc.SPHERE, np.float32)
    ctx = capi.Context(0)
    try:
        c = probe_run(ctx, p, table, visits, (oracle_lib.sphere_occluder(orc), sphere.ctypes.data))
        _check_pass(ctx, ref, case, c)
        probed, occluded, calls = ctx.probe_stats()
        assert 0 < occluded < probed, (probed, occluded, calls)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def thin_ref(orc):
    p = common.tl_setup(64, 40, samples_override=32)
    visits, cols = common.make_stream(p, 64, 40, 9, f_hi=0.01)
    ref = common.run_oracle(orc, p, None, visits)
    yield ref
    ref.close()


@pytest.mark.parametrize("R", rc.THIN_R)
def test_thin_lens_ignores_the_parameter(orc, gpu_ctx_factory, thin_ref, R):
    """the oracle's frame at the default count (tests/test_retry_cases.py: the same at all three)"""
    p = common.tl_setup(64, 40, samples_override=32, vignetting_retries=R)
    visits, cols = common.make_stream(p, 64, 40, 9, f_hi=0.01)
    ctx = gpu_ctx_factory()
    c = gpu_run(ctx, p, None, visits)
    assert _counters(c) == _counters(thin_ref.counters()) and c.accepted_draws > 0
    check_logs(ctx, thin_ref)
    check_frame(ctx, thin_ref)


def test_no_try_at_all(orc, gpu_ctx_factory):
    """vignetting_retries < 0: the reference's `tries <= vignetting_retries` is false before the first try, so every
    redistributed visit uses up its 5 x samples attempts, nothing is accepted and those visits add nothing to the frame --
    in a context's first pass and in its second, and what the library's own trace_ray_bw_po says.  (0 is one try.)  A third
    pass at 15 retries: the context goes back to drawing."""
    (case,) = rc.named("negative")
    p, table, visits, keep = rc.setup(case)
    ref = rc.oracle(orc, case)
    ctx = gpu_ctx_factory()
    for k in range(2):
        c = gpu_run(ctx, p, table, visits)
        assert _counters(c) == (234, 234 * 5 * case["S"], 0)
        _check_pass(ctx, ref, case, c)
        assert ctx.draw_log().shape[0] == 0
    rng = np.random.default_rng(3)
    n = 256
    target = np.stack([rng.uniform(-600, 600, n), rng.uniform(-400, 400, n), rng.uniform(500, 5000, n)], 1)
    xy, ok = ctx.test_trace_bw_po(target, rng.integers(0, 64, n), rng.integers(0, 40, n), rng.integers(0, 160, n))
    assert not ok.any()
    usual = rc.BY_NAME["base-r15"]
    p, table, visits, keep = rc.setup(usual)
    c = gpu_run(ctx, p, table, visits)
    _check_pass(ctx, rc.oracle(orc, usual), usual, c)
