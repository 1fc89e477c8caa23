"""The accepted draws of a visit range per colour channel on the GPU (lentil_hip_list_draws with LENTIL_DRAWS_CHANNELS,
list_draws_chroma_kernel in csrc/lentil_list_draws.h: polynomial optics with abb_chromatic != 0) against the oracle's
single-threaded pass over the same stream (tests/list_draw_chroma_cases.py), against lentil_hip_trace_points at the channels'
wavelengths and against the GPU pass's own draw log.  tests/test_list_draw_chroma_cases.py holds the cases to what they are
there for.
"""
import ctypes as C

import numpy as np
import pytest

import common
import list_draw_cases as lc
import list_draw_chroma_cases as cc
from pota_amd import _abi, capi

pytestmark = pytest.mark.gpu

GUARD = 64          # records behind out[capacity] that must stay as they were


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ctx(make, s, frame=False):
    ctx = make()
    ctx.set_params(s["p"])
    if s["table"] is not None:
        ctx.set_lens(s["table"])
    if s["bokeh"]:
        import bokeh_tables
        ctx.set_bokeh(bokeh_tables.tables(s["bokeh"]))
    if s["lens_mode"] is not None:
        ctx.set_lens_mode(s["lens_mode"])
    if frame:
        ctx.alloc_frame(1)
    ctx.upload_visits(s["visits"])
    return ctx


def _sorted(rec):
    return rec[np.lexsort((rec["attempt"], rec["visit"]))]


def _as_log(rec):
    r = _sorted(rec)
    return np.stack([r["visit"], r["attempt"], r["pixel"]], 1).astype(np.uint32).reshape(-1, 3)


def _same_records(a, b):
    a, b = _sorted(a), _sorted(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _key(log):
    return log[:, 0].astype(np.uint64) << np.uint64(32) | log[:, 1].astype(np.uint64)


def _code(fn):
    with pytest.raises(capi.LentilError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- 1. the list against the oracle's pass, the positions against trace_points ---------------------------------------------------------
@pytest.mark.parametrize("name", cc.ALL)
def test_list_against_the_oracle(orc, gpu_ctx_factory, name):
    want, s = cc.oracle_pass(orc, name), cc.setup(name)
    ctx = _ctx(gpu_ctx_factory, s)
    plan, totals = ctx.plan_visits()
    rec, n_draws, attempts = ctx.list_draws(channels=True)
    print(name, "totals", totals, "records", n_draws, "attempts", attempts)
    assert ctx.list_draws_path() == s["path"]
    assert rec.dtype == _abi.Draw and rec.shape == (n_draws,)
    assert totals[1] == want["redistributed"]
    assert n_draws == want["accepted"] and attempts == want["attempted"]
    assert n_draws <= 11 * totals[2]
    got = _as_log(rec)
    assert got.shape == want["log"].shape and np.array_equal(got, want["log"])
    if name == "retries-1":
        assert n_draws == 0 and attempts == 5 * 16 * want["redistributed"]
        return
    fl = np.floor(rec["xy"]).astype(np.int64)
    assert np.array_equal(fl[:, 0] + fl[:, 1] * int(s["p"].xres), rec["pixel"].astype(np.int64))
    if name in ("pos-16", "short-r3"):
        assert n_draws > totals[2]                                                 # totals[2] is no bound here


@pytest.mark.parametrize("name", cc.POSITION_CASES)
def test_positions_are_trace_points_at_the_channels_wavelengths(gpu_ctx_factory, name):
    """pixel, xy and tries of channel c's records are what trace_points returns for (plan.cs, plan.pixel, n) at
    draw_channels(p).lambda[c], bit for bit -- and an executed attempt's channel that is not in the list did not land"""
    s = cc.setup(name)
    ctx = _ctx(gpu_ctx_factory, s)
    plan, totals = ctx.plan_visits()
    rec = _sorted(ctx.list_draws(channels=True)[0])
    n_ch, lam, w = capi.draw_channels(s["p"])
    assert n_ch == 3 and rec.shape[0] > 0
    n = (rec["attempt"] & cc.ATTEMPT_MASK).astype(np.int64)
    ch = (rec["attempt"] >> cc.CHANNEL_SHIFT).astype(np.int64)
    vis, inv = np.unique(rec["visit"], return_inverse=True)
    k = int(n.max()) + 1
    last = np.zeros(vis.size, np.int64)
    np.maximum.at(last, inv, n)
    for c in range(3):
        tp = ctx.trace_points(np.ascontiguousarray(plan["cs"][vis]), np.ascontiguousarray(plan["pixel"][vis]), k, lam=float(lam[c]), want_tries=True)
        m = ch == c
        assert m.any()
        assert np.array_equal(tp["pixel"][inv[m], n[m]], rec["pixel"][m])
        assert _same_bits(tp["xy"][inv[m], n[m]], rec["xy"][m])
        assert np.array_equal(tp["tries"][inv[m], n[m]], rec["tries"][m])
        landed = np.zeros(tp["pixel"].shape, bool)
        landed[inv[m], n[m]] = True
        upto = np.arange(k)[None, :] <= last[:, None]
        assert (tp["pixel"][upto & ~landed] >= _abi.POINT_OUTSIDE).all()


# ---- 2. a film of the caller's own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.OWN_FILM_CASES)
def test_own_film_per_channel(orc, gpu_ctx_factory, name):
    """the recipe of INTEGRATION.md 3f on the host, from plan + list + draw_channels alone: per record of channel c,
    (rgba[k] + add_energy) * weight * rgb_weight[c][k] to colour component k, (alpha + add_energy) * weight to alpha, weight to
    the weight, at `pixel`; rgba * weight at its own pixel per visit that stays -- against the oracle's exact sums, 1e-5"""
    want, s = cc.oracle_pass(orc, name), cc.setup(name)
    ctx = _ctx(gpu_ctx_factory, s)
    plan, totals = ctx.plan_visits()
    rec, n_draws, attempts = ctx.list_draws(channels=True)
    assert n_draws == rec.shape[0] > 0
    n_ch, lam, rgb_weight = capi.draw_channels(s["p"])
    w, h = int(s["p"].xres), int(s["p"].yres)
    rgba = s["cols"]["rgba"].astype(np.float64)
    buf, wgt = np.zeros((w * h, 4)), np.zeros(w * h)
    flagged = (plan["flags"] & _abi.PLAN_REDISTRIBUTE) != 0
    stay = np.nonzero(~flagged)[0]
    own = (plan["pixel"][stay] & 0xFFFF).astype(np.int64) + (plan["pixel"][stay] >> 16).astype(np.int64) * w
    wt = plan["weight"][stay].astype(np.float64)
    np.add.at(buf, own, rgba[stay] * wt[:, None])
    np.add.at(wgt, own, wt)
    v = rec["visit"]
    ch = (rec["attempt"] >> cc.CHANNEL_SHIFT).astype(np.int64)
    wt = plan["weight"][v].astype(np.float64)
    factor = np.concatenate([rgb_weight.astype(np.float64)[ch], np.ones((v.size, 1))], axis=1)      # alpha takes 1
    pix = rec["pixel"].astype(np.int64)
    np.add.at(buf, pix, (rgba[v] + plan["add_energy"][v].astype(np.float64)[:, None]) * wt[:, None] * factor)
    np.add.at(wgt, pix, wt)
    rb, rw = want["buffer64"], want["weight64"]
    for k in range(4):
        assert np.array_equal(buf[:, k] != 0, rb[:, k] != 0), k
    assert np.array_equal(wgt != 0, rw != 0)
    err = max(common.rel_err(buf[rb != 0], rb[rb != 0]), common.rel_err(wgt[rw != 0], rw[rw != 0]))
    print(name, "own film against the oracle's exact sums:", err)
    assert err < 1e-5
    differ = any(not np.array_equal(rb[:, 0] != 0, rb[:, k] != 0) for k in (1, 2))
    assert differ == (s["p"].abb_chromatic > 0)                                    # channel c reaches component c alone
    if name == "add-energy":
        assert (plan["add_energy"][flagged] > 0).any()


# ---- 3. the pass agrees ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pos-16", "short-r0"])
def test_the_pass_draws_the_same_list(gpu_ctx_factory, name):
    s = cc.setup(name)
    ctx = _ctx(gpu_ctx_factory, s, frame=True)
    ctx.set_draw_log(1 << 20)
    rec, n_draws, attempts = ctx.list_draws(channels=True)
    ctx.clear_frame()
    ctx.redistribute()
    ctx.resolve()
    c = ctx.counters()
    log = common.sort_log(ctx.draw_log())
    assert log.shape[0] > 0 and np.array_equal(_as_log(rec), log)
    assert (c.accepted_draws, c.attempted_draws) == (n_draws, attempts)


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
def test_ranges_forms_and_capacity(orc, gpu_ctx_factory):
    want, s = cc.oracle_pass(orc, "samples-65"), cc.setup("samples-65")
    ctx = _ctx(gpu_ctx_factory, s)
    whole, n_draws, attempts = ctx.list_draws(channels=True)                       # no capacity: still the whole list
    assert n_draws == want["accepted"] == whole.shape[0] and np.array_equal(_as_log(whole), want["log"])
    assert n_draws > ctx.plan_visits()[1][2]

    # two visit ranges split at an odd index: the union is the list, the counts add up
    cut = s["n"] // 2 + 77
    assert cut % 2 == 1 and cut % 64
    a, na, ta = ctx.list_draws(0, cut, channels=True)
    b, nb, tb = ctx.list_draws(cut, s["n"] - cut, channels=True)
    assert na + nb == n_draws and ta + tb == attempts and na and nb
    assert (a["visit"] < cut).all() and (b["visit"] >= cut).all()
    assert _same_records(np.concatenate([a, b]), whole)

    # device pointers
    drec, dn, dt = ctx.list_draws(capacity=n_draws, device=True, channels=True)
    assert drec.is_cuda and (dn, dt) == (n_draws, attempts)
    assert _same_records(drec.cpu().numpy().view(_abi.Draw).reshape(-1)[:dn], whole)

    # capacity: one record short -- the full count, nothing behind out[capacity]
    cap = n_draws - 1
    out = np.full((cap + GUARD) * 32, 0xA5, np.uint8).view(_abi.Draw)
    nd, att = C.c_uint64(), C.c_uint64()
    req = _abi.DrawList()
    req.first_visit, req.n_visits, req.capacity, req.out, req.flags = 0, s["n"], cap, out.ctypes.data, _abi.DRAWS_CHANNELS
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
    req.out, req.flags = dev.data_ptr(), _abi.DRAWS_DEVICE_POINTERS | _abi.DRAWS_CHANNELS
    assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.OK and nd.value == n_draws
    host = dev.cpu().numpy()
    assert (host[cap:] == 0xA5).all() and np.unique(_as_log(host[:cap].view(_abi.Draw).reshape(-1)), axis=0).shape[0] == cap

    # the lens mode switched between two calls: the same list on the other path
    assert ctx.list_draws_path() == _abi.DRAWS_PATH_COMPILED_IN
    ctx.set_lens_mode(1)
    other = ctx.list_draws(channels=True)[0]
    assert ctx.list_draws_path() == _abi.DRAWS_PATH_INTERPRETER and _same_records(other, whole)


# ---- 5. what the flag means --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["retries3", "tl-plain"])
def test_the_flag_leaves_the_plain_list_as_it_is(gpu_ctx_factory, name):
    s = lc.setup(name)
    ctx = _ctx(gpu_ctx_factory, s)
    plain, n0, t0 = ctx.list_draws()
    flagged, n1, t1 = ctx.list_draws(channels=True)
    assert n0 > 0 and (n0, t0) == (n1, t1) and _same_records(plain, flagged)
    assert int(flagged["attempt"].max()) < (1 << cc.CHANNEL_SHIFT)
    assert ctx.list_draws_path() == s["path"]


def test_refusals(gpu_ctx_factory):
    s = cc.setup("pos-16")
    ctx = _ctx(gpu_ctx_factory, s)
    good = ctx.list_draws(channels=True)[1]
    assert good > 0
    # without the flag the refusal stands as it is
    rc, msg = _code(lambda: ctx.list_draws())
    assert rc == _abi.ERR_UNSUPPORTED and "abb_chromatic" in msg and "three" in msg
    assert ctx.list_draws(channels=True)[1] == good
    # with the probed flag: not built, whether there is a probe or not
    rc, msg = _code(lambda: ctx.list_draws(channels=True, probed=True))
    assert rc == _abi.ERR_UNSUPPORTED and "LENTIL_DRAWS_PROBED" in msg and "abb_chromatic" in msg
    assert ctx.list_draws(channels=True)[1] == good
    # the wavelengths are the mode's own
    rc, msg = _code(lambda: ctx.list_draws(channels=True, lam=0.45))
    assert rc == _abi.ERR_INVALID and "lambda" in msg
    assert ctx.list_draws(channels=True)[1] == good
    # the channel bits need 5 * samples + vignetting_retries < 2^30
    pr = type(s["p"]).from_buffer_copy(s["p"])
    pr.vignetting_retries = (1 << 30) - 5 * 16
    ctx.set_params(pr)
    rc, msg = _code(lambda: ctx.list_draws(0, 64, capacity=16, channels=True))
    assert rc == _abi.ERR_UNSUPPORTED and "2^30" in msg
    ctx.set_params(s["p"])
    assert ctx.list_draws(channels=True)[1] == good
    # the thin lens with abb_chromatic > 0 stays refused, flag or not
    st = lc.setup("tl-plain")
    tl = _ctx(gpu_ctx_factory, st)
    pt = type(st["p"]).from_buffer_copy(st["p"])
    pt.abb_chromatic = 0.6
    tl.set_params(pt)
    rc, msg = _code(lambda: tl.list_draws(capacity=16, channels=True))
    assert rc == _abi.ERR_UNSUPPORTED and "abb_chromatic" in msg and "xor128" in msg
    tl.set_params(st["p"])
    assert tl.list_draws(channels=True)[1] > 0


def test_white_channels_at_another_wavelength(gpu_ctx_factory):
    """abb_chromatic < 0: `lambda` replaces lambda_bw for all three channels, as in the plain list -- the records are the plain
    list's of the same stream at that wavelength, three times"""
    s = cc.setup("neg-16")
    ctx = _ctx(gpu_ctx_factory, s)
    rec = _sorted(ctx.list_draws(channels=True, lam=lc.LAM_BLUE)[0])
    base = _sorted(ctx.list_draws(channels=True)[0])
    assert rec.shape[0] > 0 and rec.shape[0] % 3 == 0 and not _same_records(rec, base)
    n = rec["attempt"] & cc.ATTEMPT_MASK
    vis, inv = np.unique(rec["visit"], return_inverse=True)
    plan = ctx.plan_visits()[0]
    tp = ctx.trace_points(np.ascontiguousarray(plan["cs"][vis]), np.ascontiguousarray(plan["pixel"][vis]), int(n.max()) + 1, lam=lc.LAM_BLUE)
    assert np.array_equal(tp["pixel"][inv, n], rec["pixel"]) and _same_bits(tp["xy"][inv, n], rec["xy"])
