"""A visit range's plan and its accepted draws on the GPU (lentil_hip_plan_visits, lentil_hip_list_draws,
csrc/lentil_list_draws.h) against the oracle's single-threaded pass over the same stream (tests/list_draw_cases.py) and
against lentil_hip_trace_points, which tests/test_gpu_trace_points.py pins to the oracle.  tests/test_list_draw_cases.py
holds the cases to what they are there for.
"""
import ctypes as C

import numpy as np
import pytest

import common
import list_draw_cases as lc
from pota_amd import _abi, capi

pytestmark = pytest.mark.gpu

GUARD = 64          # records behind out[capacity] that must stay as they were


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ctx(make, monkeypatch, name, frame=False):
    s = lc.setup(name)
    if s["path"] == _abi.DRAWS_PATH_INTERPRETER and s["lens_mode"] is None:
        # a table that is not compiled in: no compiling thread for kernels these calls never run (read at context creation)
        monkeypatch.setenv("LENTIL_LENS_JIT", "0")
    ctx = make()
    ctx.set_params(s["p"])
    if s["table"] is not None:
        ctx.set_lens(s["table"])
    if s["bokeh"]:
        import bokeh_tables
        ctx.set_bokeh(bokeh_tables.tables(s["bokeh"]))
    if s["lens_mode"] is not None:
        ctx.set_lens_mode(s["lens_mode"])
    if s["keys"] is not None:
        ctx.set_camera_motion(s["keys"])
    if frame:
        ctx.alloc_frame(1)
    ctx.upload_visits(s["visits"])
    return ctx, s


def _sorted(rec):
    return rec[np.lexsort((rec["attempt"], rec["visit"]))]


def _as_log(rec):
    r = _sorted(rec)
    return np.stack([r["visit"], r["attempt"], r["pixel"]], 1).astype(np.uint32).reshape(-1, 3)


def _same_records(a, b):
    a, b = _sorted(a), _sorted(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the list and the plan against the oracle's pass, the positions against trace_points -------------------------------------
@pytest.mark.parametrize("name", lc.ALL)
def test_list_plan_and_positions(orc, gpu_ctx_factory, monkeypatch, name):
    want = lc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    assert ctx.list_draws_path() == _abi.DRAWS_PATH_THIN_LENS                      # no call yet
    plan, totals = ctx.plan_visits()
    rec, n_draws, attempts = ctx.list_draws(lam=s["lam"])
    print(name, "totals", totals, "draws", n_draws, "attempts", attempts)
    assert ctx.list_draws_path() == s["path"]

    # plan parity: the oracle's counters, and the bound the list is sized with
    assert plan.dtype == _abi.VisitPlan and plan.shape == (s["n"],)
    flagged = (plan["flags"] & _abi.PLAN_REDISTRIBUTE) != 0
    assert totals[0] == want["visits"] == s["n"] and totals[1] == want["redistributed"] == int(flagged.sum())
    assert totals[2] == int(plan["samples"][flagged].astype(np.int64).sum()) >= n_draws
    assert not (plan["flags"] & ~np.uint32(_abi.PLAN_REDISTRIBUTE)).any()
    if s["samples"]:
        assert (plan["samples"] == s["samples"]).all()                             # computed for every visit
    assert not plan["add_energy"][~flagged].any()

    # list parity: record for record the oracle's draw log
    assert rec.dtype == _abi.Draw and rec.shape == (n_draws,)
    assert n_draws == want["accepted"] and attempts == want["attempted"]
    got = _as_log(rec)
    assert got.shape == want["log"].shape and np.array_equal(got, want["log"])
    if name == "retries-1":
        assert n_draws == 0 and attempts == 5 * s["samples"] * want["redistributed"]
        return
    assert flagged[rec["visit"]].all()
    p = s["p"]
    fl = np.floor(rec["xy"]).astype(np.int64)
    assert np.array_equal(fl[:, 0] + fl[:, 1] * int(p.xres), rec["pixel"].astype(np.int64))

    # position parity: xy and tries are what trace_points returns for (plan.cs, plan.pixel, attempt)
    r = _sorted(rec)
    vis, first, count = np.unique(r["visit"], return_index=True, return_counts=True)
    k = int(r["attempt"].max()) + 1
    tp = ctx.trace_points(np.ascontiguousarray(plan["cs"][vis]), np.ascontiguousarray(plan["pixel"][vis]), k, lam=s["lam"], want_tries=True)
    row = np.repeat(np.arange(vis.size), count)
    assert np.array_equal(tp["pixel"][row, r["attempt"]], r["pixel"])
    assert _same_bits(tp["xy"][row, r["attempt"]], r["xy"])
    assert np.array_equal(tp["tries"][row, r["attempt"]], r["tries"])
    if s["camera"] == "tl":
        assert not r["tries"].any()
    # ... and every attempt below a visit's last record that is not in the list did not land
    landed = np.zeros(tp["pixel"].shape, bool)
    landed[row, r["attempt"]] = True
    upto = np.arange(k)[None, :] <= r["attempt"][first + count - 1][:, None]
    assert (tp["pixel"][upto & ~landed] >= _abi.POINT_OUTSIDE).all()


def test_formula_draw_counts(orc, gpu_ctx_factory, monkeypatch):
    """plan.samples of the formula case's highlights are the oracle's draw counts, below and above a slab"""
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, "formula")
    plan, totals = ctx.plan_visits()
    vis, samples = lc.formula_samples(orc, "formula")
    assert np.array_equal(plan["samples"][vis].astype(np.int64), samples)
    flagged = (plan["flags"] & _abi.PLAN_REDISTRIBUTE) != 0
    assert (plan["samples"][flagged] < 64).any() and (plan["samples"][flagged] > 64).any()


# ---- 2. a film of the caller's own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.OWN_FILM_CASES)
def test_own_film(orc, gpu_ctx_factory, monkeypatch, name):
    """the recipe of INTEGRATION.md 3f on the host, from plan + list alone: (rgba + add_energy) * weight at `pixel` per record,
    rgba * weight at its own pixel per visit that stays; the weights likewise -- against the oracle's exact sums, 1e-5"""
    want = lc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, totals = ctx.plan_visits()
    rec, n_draws, attempts = ctx.list_draws(capacity=totals[2])
    assert n_draws == rec.shape[0] > 0
    w, h = int(s["p"].xres), int(s["p"].yres)                                     # (the frame with its filter margin)
    rgba = s["cols"]["rgba"].astype(np.float64)
    buf, wgt = np.zeros((w * h, 4)), np.zeros(w * h)
    flagged = (plan["flags"] & _abi.PLAN_REDISTRIBUTE) != 0
    stay = np.nonzero(~flagged)[0]
    own = (plan["pixel"][stay] & 0xFFFF).astype(np.int64) + (plan["pixel"][stay] >> 16).astype(np.int64) * w
    wt = plan["weight"][stay].astype(np.float64)
    np.add.at(buf, own, rgba[stay] * wt[:, None])
    np.add.at(wgt, own, wt)
    v = rec["visit"]
    wt = plan["weight"][v].astype(np.float64)
    np.add.at(buf, rec["pixel"].astype(np.int64), (rgba[v] + plan["add_energy"][v].astype(np.float64)[:, None]) * wt[:, None])
    np.add.at(wgt, rec["pixel"].astype(np.int64), wt)
    rb, rw = want["buffer64"], want["weight64"]
    assert np.array_equal(buf != 0, rb != 0) and np.array_equal(wgt != 0, rw != 0)
    err = max(common.rel_err(buf[rb != 0], rb[rb != 0]), common.rel_err(wgt[rw != 0], rw[rw != 0]))
    print(name, "own film against the oracle's exact sums:", err)
    assert err < 1e-5
    if name == "add-energy":
        assert (plan["add_energy"][flagged] > 0).any()


# ---- 3. independence -------------------------------------------------------------------------------------------------------------------
def test_ranges_forms_and_capacity(orc, gpu_ctx_factory, monkeypatch):
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, "samples-65")
    want = lc.oracle_pass(orc, "samples-65")
    plan, totals = ctx.plan_visits()
    whole, n_draws, attempts = ctx.list_draws()
    assert n_draws == want["accepted"] and np.array_equal(_as_log(whole), want["log"])

    # two visit ranges split at an odd index: the union is the list, the counts add up
    cut = s["n"] // 2 + 77
    assert cut % 2 == 1 and cut % 64
    a, na, ta = ctx.list_draws(0, cut)
    b, nb, tb = ctx.list_draws(cut, s["n"] - cut)
    assert na + nb == n_draws and ta + tb == attempts and na and nb
    assert (a["visit"] < cut).all() and (b["visit"] >= cut).all()
    assert _same_records(np.concatenate([a, b]), whole)
    pa, tota = ctx.plan_visits(0, cut)
    pb, totb = ctx.plan_visits(cut)
    assert np.concatenate([pa, pb]).tobytes() == plan.tobytes()
    assert tuple(x + y for x, y in zip(tota, totb)) == totals

    # device pointers
    dplan, dtot = ctx.plan_visits(device=True)
    assert dplan.is_cuda and dtot == totals
    assert dplan.cpu().numpy().view(_abi.VisitPlan).reshape(-1).tobytes() == plan.tobytes()
    eplan, none = ctx.plan_visits(device=True, totals=False)                       # only enqueued
    assert none is None
    ctx.sync()
    assert eplan.cpu().numpy().tobytes() == plan.tobytes()
    drec, dn, dt = ctx.list_draws(capacity=totals[2], device=True)
    assert drec.is_cuda and (dn, dt) == (n_draws, attempts)
    assert _same_records(drec.cpu().numpy().view(_abi.Draw).reshape(-1)[:dn], whole)

    # capacity: one record short -- the full count, nothing behind out[capacity], then the full list
    cap = n_draws - 1
    out = np.full((cap + GUARD) * 32, 0xA5, np.uint8).view(_abi.Draw)
    assert out.shape == (cap + GUARD,)
    nd, att = C.c_uint64(), C.c_uint64()
    req = _abi.DrawList()
    req.first_visit, req.n_visits, req.capacity, req.out = 0, s["n"], cap, out.ctypes.data
    req.n_draws, req.attempts = C.pointer(nd), C.pointer(att)
    assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.OK
    assert (nd.value, att.value) == (n_draws, attempts)
    assert (out[cap:].view(np.uint8) == 0xA5).all()
    head = _as_log(out[:cap])                                                     # some n_draws - 1 records of the list
    assert np.unique(_key(head)).size == cap and np.isin(_key(head), _key(want["log"])).all()
    assert np.array_equal(want["log"][np.searchsorted(_key(want["log"]), _key(head))], head)
    import torch
    dev = torch.full((cap + GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    req.out, req.flags = dev.data_ptr(), _abi.DRAWS_DEVICE_POINTERS
    assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.OK and nd.value == n_draws
    host = dev.cpu().numpy()
    assert (host[cap:] == 0xA5).all() and np.unique(_as_log(host[:cap].view(_abi.Draw).reshape(-1)), axis=0).shape[0] == cap
    again, n2, t2 = ctx.list_draws(capacity=n_draws)
    assert n2 == n_draws and _same_records(again, whole)


def _key(log):
    return log[:, 0].astype(np.uint64) << np.uint64(32) | log[:, 1].astype(np.uint64)


def test_a_list_between_clear_and_pass_changes_nothing(orc, gpu_ctx_factory, monkeypatch):
    """list_draws and plan_visits between clear_frame and redistribute: download_records of the pass that follows is that of a
    context that never made the calls.  Every pixel no draw reaches holds its own visits' sums, added in a fixed order: bit for
    bit.  The draws are added with atomics in an order no two runs share, with or without the calls: those pixels at the
    project's 1e-5 bar, and the draw log and the counters entry for entry."""
    want = lc.oracle_pass(orc, "retries3")

    def run(ask):
        ctx, s = _ctx(gpu_ctx_factory, monkeypatch, "retries3", frame=True)
        ctx.set_draw_log(1 << 20)
        got = None
        for _ in range(2):                     # (the second pass is sized from the first)
            ctx.clear_frame()
            if ask:
                got = ctx.plan_visits(), ctx.list_draws()
            ctx.redistribute()
            ctx.resolve()
        c = ctx.counters()
        return (common.sort_log(ctx.draw_log()), ctx.download_records(),
                (c.visits, c.redistributed_visits, c.attempted_draws, c.accepted_draws), got)

    log_a, rec_a, ctr_a, got = run(True)
    log_b, rec_b, ctr_b, _ = run(False)
    assert log_a.shape[0] > 0 and np.array_equal(log_a, log_b) and np.array_equal(log_a, want["log"]) and ctr_a == ctr_b
    assert rec_a.shape == rec_b.shape and rec_a.shape[1] >= 5
    drawn = np.zeros(rec_a.shape[0], bool)
    drawn[log_a[:, 2]] = True
    assert drawn.any() and not drawn.all() and _same_bits(rec_a[~drawn], rec_b[~drawn])
    assert np.array_equal(rec_a != 0, rec_b != 0)
    assert common.rel_err(rec_a[rec_b != 0], rec_b[rec_b != 0]) < 1e-5
    (plan, totals), (rec, n_draws, attempts) = got
    assert np.array_equal(_as_log(rec), log_a) and (totals[0], totals[1], attempts, n_draws) == ctr_a


# ---- 4. paths and refusals ---------------------------------------------------------------------------------------------------------------
def test_paths(gpu_ctx_factory, monkeypatch):
    got = []
    for name in lc.LENS_CASES + ("tl-plain",):
        ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
        ctx.list_draws(0, 640)
        got.append(ctx.list_draws_path())
    assert got == [2, 2, 1, 1, 0]
    # one context, the lens mode switched between two calls: the same list
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, "lens-double-gauss")
    a = ctx.list_draws()[0]
    ctx.set_lens_mode(1)
    b = ctx.list_draws()[0]
    assert ctx.list_draws_path() == _abi.DRAWS_PATH_INTERPRETER and a.shape[0] > 0 and _same_records(a, b)


def test_refusals(gpu_ctx_factory, monkeypatch):
    def code(fn):
        with pytest.raises(capi.LentilError) as e:
            fn()
        return e.value.code, str(e.value)

    bare = gpu_ctx_factory()
    assert code(lambda: bare.list_draws(0, 1, capacity=4))[0] == _abi.ERR_INVALID              # no parameters
    s = lc.setup("retries15")
    bare.set_params(s["p"])
    assert code(lambda: bare.plan_visits(0, 1))[0] == _abi.ERR_INVALID                          # no visits
    bare.upload_visits(s["visits"])
    assert code(lambda: bare.list_draws(0, 1, capacity=4))[0] == _abi.ERR_INVALID              # polynomial optics, no lens

    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, "retries15")
    n = s["n"]
    assert code(lambda: ctx.list_draws(n - 10, 11, capacity=16))[0] == _abi.ERR_INVALID        # a range beyond the stream
    assert code(lambda: ctx.list_draws(n + 1, 0, capacity=16))[0] == _abi.ERR_INVALID
    assert code(lambda: ctx.plan_visits(n - 10, 11))[0] == _abi.ERR_INVALID
    nd = C.c_uint64(7)
    req = _abi.DrawList()
    req.first_visit, req.n_visits, req.capacity, req.out, req.n_draws = 0, n, 16, None, C.pointer(nd)
    assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.ERR_INVALID               # out NULL with capacity > 0
    req.capacity = 0
    assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.OK and nd.value > 0       # counting alone is a call
    req.n_draws = None
    assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.ERR_INVALID               # n_draws NULL
    assert ctx.lib.lentil_hip_list_draws(ctx.h, None) == _abi.ERR_INVALID
    # n_visits == 0: an empty list, zero totals, nothing launched
    rec, n_draws, attempts = ctx.list_draws(5, 0)
    assert rec.shape == (0,) and (n_draws, attempts) == (0, 0)
    plan, totals = ctx.plan_visits(n, 0)
    assert plan.shape == (0,) and totals == (0, 0, 0)
    # the two chromatic modes
    pc = type(s["p"]).from_buffer_copy(s["p"])
    pc.abb_chromatic = 0.5
    ctx.set_params(pc)
    rc, msg = code(lambda: ctx.list_draws())
    assert rc == _abi.ERR_UNSUPPORTED and "abb_chromatic" in msg and "three" in msg
    assert ctx.plan_visits()[1][0] == n                                                          # the plan has no such limit
    ctx.set_params(s["p"])
    assert ctx.list_draws()[1] > 0                                                               # the context stays usable
    tl, st = _ctx(gpu_ctx_factory, monkeypatch, "tl-plain")
    pt = type(st["p"]).from_buffer_copy(st["p"])
    pt.abb_chromatic = 0.6
    tl.set_params(pt)
    rc, msg = code(lambda: tl.list_draws(capacity=16))
    assert rc == _abi.ERR_UNSUPPORTED and "abb_chromatic" in msg and "xor128" in msg
    pi, model, table_i, keep_i = common.po_setup(48, 32, bokeh_enable_image=1)
    ctx.set_params(pi)
    assert code(lambda: ctx.list_draws(capacity=16))[0] == _abi.ERR_INVALID                     # bokeh_enable_image, no tables
