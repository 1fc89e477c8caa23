"""lentil_hip_redistribute with a wavelength per visit (lentil_hip_set_visit_lambdas; csrc/lentil_kernels.h:
solve_po_spectral_kernel) against the oracle's pass in which visit v is at lam[v] (tests/spectral_pass_cases.py): the
accepted-draw list bit for bit, counters equal, accumulators, weights and the resolved image at test_gpu_parity's bar.
tests/test_spectral_pass_cases.py holds the cases to frames that a pass which ignored the column would miss."""
import numpy as np
import pytest

import common
import list_draw_spectral_cases as ls
import spectral_pass_cases as sp
from pota_amd import _abi, capi
from test_gpu_list_draws_spectral import _code, _ctx, _device_probe, _host_probe
from test_gpu_parity import check_frame, check_logs

pytestmark = pytest.mark.gpu

LOG_CAP = 1 << 20


def _frame(ctx, n_aovs=1, kinds=None):
    ctx.alloc_frame(n_aovs, kinds)
    ctx.set_draw_log(LOG_CAP)


def _pass(ctx):
    ctx.clear_frame(); ctx.redistribute(); ctx.resolve(); ctx.sync()
    c = ctx.counters()
    assert c.worklist_overflow == 0
    return c


def _same_counters(c, rc):
    assert (c.visits, c.redistributed_visits, c.attempted_draws, c.accepted_draws) == (
        rc.visits, rc.redistributed_visits, rc.attempted_draws, rc.accepted_draws)


def _log(ctx):
    return common.sort_log(ctx.draw_log())


# ---- 1. against the oracle, per plain case and assignment ------------------------------------------------------------------
@pytest.mark.parametrize("case", sp.PLAIN, ids=sp.ids(sp.PLAIN))
def test_the_pass_is_the_oracles_visit_by_visit(orc, gpu_ctx_factory, monkeypatch, case):
    kind, name, assignment = case
    ref = sp.oracle_frame(orc, case)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    _frame(ctx)
    ctx.set_visit_lambdas(sp.column(case))
    thin = s["camera"] == "tl"
    for n_pass in (1, 2):                                     # (the second pass: blind chunks, sized from the first)
        c = _pass(ctx)
        _same_counters(c, ref.counters())
        assert c.streamed == 0 or thin
        check_logs(ctx, ref)
        err = check_frame(ctx, ref)
        st = ctx.spectral_pass_stats()
        print(sp.IDS[sp.ALL.index(case)], "pass", n_pass, "accepted", c.accepted_draws, "tries", c.tries, "iterations", c.newton_iterations,
              "lane rounds", c.lane_rounds, "stats", st, "max rel err %.2e" % err)
        if thin:
            assert st == (0, 0, 0, 0)
        else:
            assert st[0] == n_pass and st[1] > 0 and st[2] == s["path"] and st[3] == 0
            assert c.slow_solves == 0 and c.tries > 0 and c.lane_rounds >= c.newton_iterations >= c.tries


# ---- 2. under the occlusion probe, host and device callback -----------------------------------------------------------------
@pytest.mark.parametrize("callback", ["host", "device"])
@pytest.mark.parametrize("case", sp.PROBED, ids=sp.ids(sp.PROBED))
def test_the_probed_pass_is_the_oracles(orc, gpu_ctx_factory, monkeypatch, case, callback):
    kind, name, assignment = case
    ref = sp.oracle_frame(orc, case)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    _frame(ctx)
    if callback == "host":
        _host_probe(ctx, orc, s)
    else:
        _device_probe(ctx, s)
    ctx.set_visit_lambdas(sp.column(case))
    before = ctx.probe_stats()
    c = _pass(ctx)
    after = ctx.probe_stats()
    _same_counters(c, ref.counters())
    assert c.streamed == 0
    check_logs(ctx, ref)
    check_frame(ctx, ref)
    print(sp.IDS[sp.ALL.index(case)], callback, "probes", after[0] - before[0], "occluded", after[1] - before[1])
    assert after[0] > before[0] and after[1] > before[1]      # the probe bites
    if s["camera"] != "tl":
        st = ctx.spectral_pass_stats()
        assert st[0] == 1 and st[1] > 0 and st[2] == s["path"]


def test_a_table_compiled_at_run_time_is_served_by_the_interpreter(orc, gpu_ctx_factory, monkeypatch):
    """... in a pass with a column; the scalar passes of the same context, before and after, keep their run-time kernel"""
    case = ("plain", "lens-anamorphic", "random")
    kind, name, assignment = case
    ref = sp.oracle_frame(orc, case)
    scalar = ls.oracle_pass(orc, kind, name, 0.0)["log"]
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name, jit=True)
    assert not ctx.lens_is_compiled()
    ctx.lens_jit_wait(600.0)                                  # (seconds from the cache on disk)
    assert ctx.lens_jit_status()[0] == 2, ctx.lens_jit_status()
    _frame(ctx)
    for column in (None, sp.column(case), None):
        ctx.set_visit_lambdas(column)
        c = _pass(ctx)
        if column is None:
            assert np.array_equal(_log(ctx), scalar)
        else:
            _same_counters(c, ref.counters())
            check_logs(ctx, ref)
            check_frame(ctx, ref)
    assert ctx.spectral_pass_stats()[0] == 1 and ctx.spectral_pass_stats()[2] == _abi.DRAWS_PATH_INTERPRETER


# ---- 3. what a column means ------------------------------------------------------------------------------------------------
COLUMN_CASES = [("plain", "samples-65"), ("plain", "lens-interpreter")]


@pytest.mark.parametrize("kind,name", COLUMN_CASES, ids=["%s/%s" % k for k in COLUMN_CASES])
def test_a_constant_column_is_the_scalar_pass_at_that_wavelength(orc, gpu_ctx_factory, monkeypatch, kind, name):
    case = (kind, name, "random")
    x = ls.LAM_BLUE
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    _frame(ctx)
    ctx.set_visit_lambdas(np.full(s["n"], x))
    c = _pass(ctx)
    assert c.streamed == 0 and ctx.spectral_pass_stats()[0] == 1
    # the scalar pass of a context whose lambda_bw is x
    other = gpu_ctx_factory()
    px = type(s["p"]).from_buffer_copy(s["p"])
    px.lambda_bw = x
    assert float(px.lambda_bw) == x
    other.set_params(px)
    other.set_lens(s["table"])
    if s["lens_mode"] is not None:
        other.set_lens_mode(s["lens_mode"])
    other.upload_visits(s["visits"])
    _frame(other)
    co = _pass(other)
    assert other.spectral_pass_stats() == (0, 0, 0, 0)
    _same_counters(c, co)
    mine, theirs = _log(ctx), _log(other)
    assert mine.shape[0] > 0 and np.array_equal(mine, theirs)
    assert np.array_equal(mine, ls.oracle_pass(orc, kind, name, x)["log"])
    assert not np.array_equal(mine, ls.oracle_pass(orc, kind, name, 0.0)["log"])            # (the wavelength shows)
    ref = sp.oracle_frame(orc, case, lam=np.full(s["n"], x))
    try:
        check_frame(ctx, ref)
        check_frame(other, ref)
    finally:
        ref.close()


def test_zeros_are_lambda_bw_and_none_switches_the_column_off(orc, gpu_ctx_factory, monkeypatch):
    kind, name = "plain", "samples-65"
    case = (kind, name, "random")
    scalar = ls.oracle_pass(orc, kind, name, 0.0)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    _frame(ctx)
    ref = sp.oracle_frame(orc, case, lam=np.zeros(s["n"]))
    try:
        # a column of zeros: the scalar pass, through the spectral kernel
        ctx.set_visit_lambdas(np.zeros(s["n"]))
        c = _pass(ctx)
        assert c.streamed == 0 and ctx.spectral_pass_stats()[0] == 1
        assert np.array_equal(_log(ctx), scalar["log"])
        check_frame(ctx, ref)
        # the case's own column, then none: the next two passes are the scalar pass, and stream where a context that never had
        # a column streams
        ctx.set_visit_lambdas(sp.column(case))
        _pass(ctx)
        assert not np.array_equal(_log(ctx), scalar["log"])
        ctx.set_visit_lambdas(None)
        fresh, _ = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
        _frame(fresh)
        streamed = []
        for turn in range(2):
            c, cf = _pass(ctx), _pass(fresh)
            _same_counters(c, cf)
            assert (c.accepted_draws, c.attempted_draws) == (scalar["accepted"], scalar["attempted"])
            assert np.array_equal(_log(ctx), scalar["log"]) and np.array_equal(_log(fresh), scalar["log"])
            check_frame(ctx, ref)
            streamed.append((c.streamed, cf.streamed))
        print("streamed (switched off, never set):", streamed)
        assert streamed[1][0] == streamed[1][1]
        assert ctx.spectral_pass_stats()[0] == 2 and fresh.spectral_pass_stats() == (0, 0, 0, 0)
    finally:
        ref.close()


# ---- 4. three AOVs, one of them closest-filtered ---------------------------------------------------------------------------
def test_three_aovs_with_a_closest_filtered_one(orc, gpu_ctx_factory):
    from test_gpu_probe_tl_chroma import KINDS
    (W, H), M = ls.FRAMES[1], ls.M
    p, model, table, keep = common.po_setup(W, H, samples_override=24, lambda_bw=ls.LAMBDA_BW)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02, n_extra=2)
    n = int(visits.n)
    lam = np.asarray(ls.PALETTE)[np.random.default_rng(0x3A0F).integers(0, len(ls.PALETTE), n)]
    ref = sp.oracle_run(orc, p, table, visits, lam, n_aovs=len(KINDS), kinds=KINDS)
    try:
        ctx = gpu_ctx_factory()
        ctx.set_params(p)
        ctx.set_lens(table)
        ctx.upload_visits(visits)
        _frame(ctx, len(KINDS), KINDS)
        ctx.set_visit_lambdas(lam)
        c = _pass(ctx)
        _same_counters(c, ref.counters())
        assert c.streamed == 0 and c.accepted_draws > 0
        check_logs(ctx, ref)
        check_frame(ctx, ref, n_aovs=len(KINDS), kinds=KINDS)
        st = ctx.spectral_pass_stats()
        assert st[0] >= 1 and st[1] > 0 and st[2] == _abi.DRAWS_PATH_COMPILED_IN
    finally:
        ref.close()


# ---- 5. chunks and sub-batches ---------------------------------------------------------------------------------------------
def test_chunks_and_sub_batches_give_the_same_pass(orc, gpu_ctx_factory, monkeypatch):
    case = ("plain", "samples-64", "random")
    kind, name, assignment = case
    ref = sp.oracle_frame(orc, case)
    want = common.sort_log(ref.log())
    s = ls.setup(kind, name)
    retries = max(int(s["p"].vignetting_retries), 0)
    per_item = 4 * s["samples"] + 3 * retries + 32           # enqueue_chunk_draws' bound for one item
    logs = []
    for chunks, pool in (("1", None), ("4", None), ("1", str(20 * per_item))):
        monkeypatch.setenv("LENTIL_CHUNKS", chunks)           # (read when the context is created)
        if pool is None:
            monkeypatch.delenv("LENTIL_MAX_POOL_UNITS", raising=False)
        else:
            monkeypatch.setenv("LENTIL_MAX_POOL_UNITS", pool)
        ctx, _ = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
        _frame(ctx)
        ctx.set_visit_lambdas(sp.column(case))
        c = _pass(ctx)
        _same_counters(c, ref.counters())
        if pool is not None:
            assert c.redistributed_visits > 3 * 20            # several sub-batches of 20 items, run through finish_rounds
        logs.append(_log(ctx))
        check_frame(ctx, ref)
        assert ctx.spectral_pass_stats()[1] > 0
    for got in logs:
        assert got.shape == want.shape and np.array_equal(got, want)


# ---- 6. no tries -----------------------------------------------------------------------------------------------------------
def test_negative_retries_draw_nothing(orc, gpu_ctx_factory, monkeypatch):
    kind, name = "plain", "retries15"
    s = ls.setup(kind, name)
    p = type(s["p"]).from_buffer_copy(s["p"])
    p.vignetting_retries = -1
    lam = ls.lambdas(kind, name)
    ref = sp.oracle_run(orc, p, s["table"], s["visits"], lam)
    try:
        rc = ref.counters()
        assert rc.accepted_draws == 0 and rc.redistributed_visits > 0 and rc.attempted_draws == 5 * s["samples"] * rc.redistributed_visits
        ctx, _ = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
        ctx.set_params(p)
        _frame(ctx)
        ctx.set_visit_lambdas(lam)
        c = _pass(ctx)
        _same_counters(c, rc)
        assert ctx.draw_log().shape[0] == 0 and c.streamed == 0
        check_frame(ctx, ref)
    finally:
        ref.close()


# ---- 7. the column in device memory ----------------------------------------------------------------------------------------
def test_a_bound_device_column_is_the_uploaded_one(orc, gpu_ctx_factory, monkeypatch):
    import torch
    case = ("plain", "samples-65", "blocks")
    kind, name, assignment = case
    ref = sp.oracle_frame(orc, case)
    lam = sp.column(case)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    _frame(ctx)
    ctx.set_visit_lambdas(lam)
    c = _pass(ctx)
    host_log = _log(ctx)
    t_lam = torch.from_numpy(lam.copy()).to("cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    for bad in (lam, t_lam.cpu(), t_lam.float(), torch.stack([t_lam, t_lam], 1)[:, 0]):
        with pytest.raises(ValueError, match="lambdas"):          # numpy as device memory, not on the GPU, fp32, strided
            ctx.set_visit_lambdas(bad, device=True)
    with pytest.raises(ValueError, match="lambdas"):
        ctx.set_visit_lambdas(t_lam)                              # a tensor as host memory
    ctx.set_visit_lambdas(t_lam, device=True)
    cd = _pass(ctx)
    _same_counters(cd, c)
    _same_counters(cd, ref.counters())
    assert np.array_equal(_log(ctx), host_log) and np.array_equal(host_log, common.sort_log(ref.log()))
    check_frame(ctx, ref)
    assert ctx.spectral_pass_stats()[0] == 2
    # bound, not copied: the pass reads what the tensor holds now
    t_lam.zero_()
    torch.cuda.synchronize()
    _pass(ctx)
    assert np.array_equal(_log(ctx), ls.oracle_pass(orc, kind, name, 0.0)["log"])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(orc, gpu_ctx_factory, monkeypatch):
    case = ("plain", "samples-65", "random")
    kind, name, assignment = case
    ref = sp.oracle_frame(orc, case)
    want = common.sort_log(ref.log())
    lam = sp.column(case)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    _frame(ctx)
    n = s["n"]

    def still_passes():
        ctx.set_visit_lambdas(lam)
        c = _pass(ctx)
        _same_counters(c, ref.counters())
        assert np.array_equal(_log(ctx), want)

    still_passes()
    # a column of another length than the stream
    ctx.set_visit_lambdas(lam[:-1])
    ctx.clear_frame()
    rc, msg = _code(ctx.redistribute)
    assert rc == _abi.ERR_INVALID and str(n - 1) in msg and str(n) in msg
    still_passes()
    # a new stream makes the column stale -- the same visits again, for that matter
    ctx.upload_visits(s["visits"])
    ctx.clear_frame()
    rc, msg = _code(ctx.redistribute)
    assert rc == _abi.ERR_INVALID and "stream" in msg
    still_passes()
    ctx.upload_visits(s["visits"])
    ctx.set_visit_lambdas(None)                                   # switched off: the scalar pass
    _pass(ctx)
    assert np.array_equal(_log(ctx), ls.oracle_pass(orc, kind, name, 0.0)["log"])
    still_passes()
    # polynomial optics with abb_chromatic != 0
    pch = type(s["p"]).from_buffer_copy(s["p"])
    pch.abb_chromatic = 0.5
    ctx.set_params(pch)
    ctx.clear_frame()
    rc, msg = _code(ctx.redistribute)
    assert rc == _abi.ERR_UNSUPPORTED and "abb_chromatic" in msg
    ctx.set_params(s["p"])
    still_passes()
    # unknown flags
    assert ctx.lib.lentil_hip_set_visit_lambdas(ctx.h, lam.ctypes.data, n, 2) == _abi.ERR_INVALID
    still_passes()
    assert ctx.spectral_pass_stats()[0] == 6


# ---- 9. the thin lens ------------------------------------------------------------------------------------------------------
def test_the_thin_lens_ignores_the_column(orc, gpu_ctx_factory, monkeypatch):
    kind, name = "plain", "tl-plain"
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    _frame(ctx)
    c0 = _pass(ctx)
    scalar = _log(ctx)
    assert scalar.shape[0] > 0 and np.array_equal(scalar, ls.oracle_pass(orc, kind, name, 0.0)["log"])
    for lam in (ls.lambdas(kind, name), np.full(s["n"], 123.0)):
        ctx.set_visit_lambdas(lam)
        c = _pass(ctx)
        _same_counters(c, c0)
        assert np.array_equal(_log(ctx), scalar)
        assert ctx.spectral_pass_stats() == (0, 0, 0, 0)
    # ... but its length is checked
    ctx.set_visit_lambdas(np.zeros(s["n"] + 1))
    ctx.clear_frame()
    rc, msg = _code(ctx.redistribute)
    assert rc == _abi.ERR_INVALID and str(s["n"] + 1) in msg
