"""lentil_hip_list_draws with LENTIL_DRAWS_PROBED (csrc/lentil_list_draws.h: list_draws_probed_kernel and the turns around
it) against the oracle's single-threaded pass under the same probe (tests/list_draw_probe_cases.py), against
lentil_hip_trace_points, and -- where the camera stands still at the origin, in centimetres, with polynomial optics -- against
an exact model walked here: the per-seed lens outcome from trace_points, the per-seed occlusion from the test's own segment
through orc_sphere_occluder, the reference's loop over the two.  tests/test_list_draw_probe_cases.py holds the cases to
"the sphere bites".
"""
import collections
import ctypes as C

import numpy as np
import pytest

import list_draw_probe_cases as pc
import oracle_lib
from pota_amd import _abi, capi
from test_gpu_list_draws import GUARD, _as_log, _same_bits, _same_records, _sorted

pytestmark = pytest.mark.gpu


def _ctx(make, monkeypatch, name, frame=False):
    s = pc.setup(name)
    if s["path"] == _abi.DRAWS_PATH_INTERPRETER and s["lens_mode"] is None:
        monkeypatch.setenv("LENTIL_LENS_JIT", "0")      # (no compiling thread for kernels these calls never run)
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


def _host_probe(ctx, orc, s):
    ctx.set_occlusion_probe(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data, s["c2w"])


def _device_probe(ctx, s):
    ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), s["sphere"].ctypes.data, s["c2w"])


def _code(fn):
    with pytest.raises(capi.LentilError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- 1. the list against the oracle's pass under the probe, host and device callback; the positions against trace_points ------
@pytest.mark.parametrize("name", pc.ALL)
def test_probed_list_is_the_oracles(orc, gpu_ctx_factory, monkeypatch, name):
    want = pc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, totals = ctx.plan_visits()
    _host_probe(ctx, orc, s)
    before = ctx.probe_stats()
    rec, n_draws, attempts = ctx.list_draws(lam=s["lam"], probed=True)
    after = ctx.probe_stats()
    print(name, "totals", totals, "draws", n_draws, "attempts", attempts, "asked / occluded / turns", tuple(a - b for a, b in zip(after, before)))
    assert ctx.list_draws_path() == s["path"]
    assert rec.dtype == _abi.Draw and rec.shape == (n_draws,)
    assert n_draws == want["accepted"] and attempts == want["attempted"] and totals[2] >= n_draws
    got = _as_log(rec)
    assert got.shape == want["log"].shape and np.array_equal(got, want["log"])

    # the device callback: the same list, byte for byte
    _device_probe(ctx, s)
    dbefore, lbefore = ctx.probe_stats(), ctx.probe_device_stats()
    drec, dn, dattempts = ctx.list_draws(lam=s["lam"], probed=True)
    dafter, lafter = ctx.probe_stats(), ctx.probe_device_stats()
    assert (dn, dattempts) == (n_draws, attempts) and _same_records(rec, drec)
    # ... asked the same segments in the same number of turns: the statistics grow alike, the lists are counted
    assert tuple(a - b for a, b in zip(dafter, dbefore)) == tuple(a - b for a, b in zip(after, before))
    assert lafter[0] - lbefore[0] == after[2] - before[2] and lafter[2] == lbefore[2]
    if name == "retries-1":
        assert n_draws == 0 and after == before and attempts == 5 * s["samples"] * want["redistributed"]
        return
    assert after[0] > before[0] and 0 < after[1] - before[1] < after[0] - before[0] and after[2] > before[2]
    # the oracle asks about every try it reaches and every time it reaches it, the library only about those that got through
    # the lens, once (what exactly it asks: test_exact_model_and_the_segments_asked)
    assert after[0] - before[0] <= want["segments"].shape[0]

    # position parity: the record is the try at seed attempt + tries, which gets through the lens at once
    r = _sorted(rec)
    cs, pix = np.ascontiguousarray(plan["cs"][r["visit"]]), np.ascontiguousarray(plan["pixel"][r["visit"]])
    seed = (r["attempt"] + r["tries"].astype(np.uint32)).astype(np.uint32)
    tp = ctx.trace_points(cs, pix, 1, first_attempt=seed, lam=s["lam"], want_tries=True)
    assert not tp["tries"].any() and np.array_equal(tp["pixel"][:, 0], r["pixel"]) and _same_bits(tp["xy"][:, 0], r["xy"])
    fl = np.floor(r["xy"]).astype(np.int64)
    assert np.array_equal(fl[:, 0] + fl[:, 1] * int(s["p"].xres), r["pixel"].astype(np.int64))
    # ... and an occluded try only adds to the vignetted ones before it
    free = ctx.trace_points(cs, pix, 1, first_attempt=np.ascontiguousarray(r["attempt"]), lam=s["lam"], want_tries=True)
    assert (r["tries"] >= free["tries"][:, 0]).all()
    if s["camera"] == "tl":
        assert not r["tries"].any()
    elif name in ("retries3", "retries15", "samples-130"):          # (where some visit is occluded in part)
        assert (r["tries"] > free["tries"][:, 0]).any()


# ---- 2. the exact model, and what the callback is asked --------------------------------------------------------------------------
def _model(orc, ctx, s, plan):
    """the reference's loop over per-seed facts -> (records [(visit, attempt, pixel, tries)], attempts, segments asked as a
    Counter of 24-byte strings, the occluded among them)"""
    p = s["p"]
    retries = int(p.vignetting_retries)
    red = np.nonzero(plan["flags"] & _abi.PLAN_REDISTRIBUTE)[0]
    samples = plan["samples"][red].astype(np.int64)
    k = int(samples.max()) * 5 + retries + 1
    # the lens: seed m of a visit gets through where trace_points makes no further try at attempt m
    tp = ctx.trace_points(np.ascontiguousarray(plan["cs"][red]), np.ascontiguousarray(plan["pixel"][red]), k, want_tries=True)
    passes = tp["tries"] == 0
    if retries == 0:
        passes &= tp["pixel"] != _abi.POINT_VIGNETTED
    # the scene: the segment from the sample's world position to the aperture point (identity camera, centimetres)
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    seg = np.zeros((red.size, k, 6), np.float32)
    seg[:, :, :3] = s["cols"]["pos_z"][red, None, :3]
    ap = (C.c_double * 2)()
    for i, v in enumerate(red):
        px, py = int(plan["pixel"][v] & 0xFFFF), int(plan["pixel"][v] >> 16)
        for m in range(k):
            orc.orc_po_aperture_sample(C.byref(p), ob, (px * py + px) & 0xFFFFFFFF, m, ap)
            seg[i, m, 3] = np.float32(-ap[0] * 0.1)
            seg[i, m, 4] = np.float32(-ap[1] * 0.1)
    seg += np.float32(0.0)                                        # (-0 -> +0, as the matrix product's sums leave it)
    if ob:
        orc.orc_bokeh_destroy(ob)
    occ = np.zeros(red.size * k, np.uint8)
    flat = np.ascontiguousarray(seg.reshape(-1, 6))
    orc.orc_sphere_occluder(C.c_void_p(s["sphere"].ctypes.data), C.c_uint64(flat.shape[0]), C.c_void_p(flat.ctypes.data), C.c_void_p(occ.ctypes.data))
    occ = occ.reshape(red.size, k).astype(bool)
    records, attempts, asked, n_occ = [], 0, collections.Counter(), 0
    for i, v in enumerate(red):
        n, a, accepted, mine = int(samples[i]), 0, 0, set()
        while accepted < n and a < 5 * n:
            tries, hit = 0, -1
            while tries <= retries:
                m = a + tries
                if passes[i, m]:
                    mine.add(m)
                    if not occ[i, m]:
                        hit = m
                        break
                tries += 1
            if hit >= 0 and tp["pixel"][i, hit] < _abi.POINT_OUTSIDE:
                records.append((v, a, int(tp["pixel"][i, hit]), tries))
                accepted += 1
            a += 1
        attempts += a
        for m in mine:
            asked[seg[i, m].tobytes()] += 1
            n_occ += int(occ[i, m])
    return records, attempts, asked, n_occ


@pytest.mark.parametrize("name", pc.MODEL)
def test_exact_model_and_the_segments_asked(orc, gpu_ctx_factory, monkeypatch, name):
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, totals = ctx.plan_visits()
    records, m_attempts, m_asked, m_occ = _model(orc, ctx, s, plan)
    watch = pc.Recorder(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data)
    ctx.set_occlusion_probe(watch.address, None, None)
    before = ctx.probe_stats()
    rec, n_draws, attempts = ctx.list_draws(probed=True)
    after = ctx.probe_stats()
    r = _sorted(rec)
    got = list(zip(r["visit"].tolist(), r["attempt"].tolist(), r["pixel"].tolist(), r["tries"].tolist()))
    assert got == [tuple(int(x) for x in t) for t in records] and attempts == m_attempts
    # the segments: exactly the model's, none twice (a visit's seeds with enable_dof = 0 coincide: as many as there are seeds)
    seg = watch.segments() + np.float32(0.0)
    asked = collections.Counter(row.tobytes() for row in seg)
    assert asked == m_asked
    if int(s["p"].enable_dof) and not int(s["p"].bokeh_enable_image):      # (an aperture image's samples repeat, too)
        assert max(asked.values()) == 1
    pos = {row.tobytes() for row in s["cols"]["pos_z"][:, :3].view(np.uint32)}
    assert all(row.tobytes() in pos for row in np.unique(watch.segments()[:, :3].view(np.uint32), axis=0))
    # the statistics grow by exactly what the callback saw
    assert tuple(a - b for a, b in zip(after, before)) == (sum(watch.calls), int(watch.answers().astype(bool).sum()), len(watch.calls))
    assert int(watch.answers().astype(bool).sum()) == m_occ and all(watch.calls)
    print(name, "turns", len(watch.calls), "lists", watch.calls)


# ---- 3. ranges, capacity, device pointers -------------------------------------------------------------------------------------------
def test_ranges_capacity_and_device_pointers(orc, gpu_ctx_factory, monkeypatch):
    name = "samples-65"
    want = pc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    watch = pc.Recorder(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data)
    ctx.set_occlusion_probe(watch.address, None, None)
    whole, n_draws, attempts = ctx.list_draws(probed=True)
    assert n_draws == want["accepted"] and np.array_equal(_as_log(whole), want["log"])
    asked_whole = collections.Counter(row.tobytes() for row in watch.segments())
    n_whole = len(watch._seg)

    # three uneven ranges: the union is the list, the counts add up, the same segments are asked
    c1, c2 = s["n"] // 5 + 13, s["n"] // 2 + 77
    assert c1 % 64 and c2 % 64
    parts = [ctx.list_draws(a, b - a, probed=True) for a, b in ((0, c1), (c1, c2), (c2, s["n"]))]
    assert sum(q[1] for q in parts) == n_draws and sum(q[2] for q in parts) == attempts and all(q[1] for q in parts)
    assert (parts[0][0]["visit"] < c1).all() and (parts[1][0]["visit"] >= c1).all() and (parts[1][0]["visit"] < c2).all()
    assert _same_records(np.concatenate([q[0] for q in parts]), whole)
    asked_parts = collections.Counter(np.frombuffer(b"".join(watch._seg[n_whole:]), np.float32).reshape(-1, 6)[i].tobytes()
                                      for i in range(sum(watch.calls[n_whole:])))
    assert asked_parts == asked_whole and max(asked_whole.values()) == 1

    # capacity: small, and none -- the full count, nothing behind out[capacity]
    _host_probe(ctx, orc, s)
    for cap in (37, 0):
        out = np.full((cap + GUARD) * 32, 0xA5, np.uint8).view(_abi.Draw)
        nd, att = C.c_uint64(), C.c_uint64()
        req = _abi.DrawList()
        req.first_visit, req.n_visits, req.capacity, req.out, req.flags = 0, s["n"], cap, out.ctypes.data if cap else None, _abi.DRAWS_PROBED
        req.n_draws, req.attempts = C.pointer(nd), C.pointer(att)
        assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.OK
        assert (nd.value, att.value) == (n_draws, attempts)
        assert (out[cap:].view(np.uint8) == 0xA5).all()
        head = _as_log(out[:cap])
        key = lambda log: log[:, 0].astype(np.uint64) << np.uint64(32) | log[:, 1].astype(np.uint64)     # noqa: E731
        assert np.unique(key(head)).size == cap and np.isin(key(head), key(want["log"])).all()
        assert np.array_equal(want["log"][np.searchsorted(key(want["log"]), key(head))], head)

    # device pointers with the flag, under the device callback, with room and without
    import torch
    _device_probe(ctx, s)
    drec, dn, dt = ctx.list_draws(device=True, probed=True)
    assert drec.is_cuda and (dn, dt) == (n_draws, attempts)
    assert _same_records(drec.cpu().numpy().view(_abi.Draw).reshape(-1)[:dn], whole)
    cap = 37
    dev = torch.full((cap + GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    nd = C.c_uint64()
    req = _abi.DrawList()
    req.first_visit, req.n_visits, req.capacity, req.out = 0, s["n"], cap, dev.data_ptr()
    req.flags, req.n_draws = _abi.DRAWS_PROBED | _abi.DRAWS_DEVICE_POINTERS, C.pointer(nd)
    assert ctx.lib.lentil_hip_list_draws(ctx.h, C.byref(req)) == _abi.OK and nd.value == n_draws
    host = dev.cpu().numpy()
    assert (host[cap:] == 0xA5).all() and np.unique(_as_log(host[:cap].view(_abi.Draw).reshape(-1)), axis=0).shape[0] == cap


# ---- 4. the flag and the probe, one without the other; a callback that fails -------------------------------------------------------
def test_flag_without_probe_and_probe_without_flag(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    free = pc.oracle_pass(orc, name, probed=False)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plain, n_plain, t_plain = ctx.list_draws()
    assert np.array_equal(_as_log(plain), free["log"]) and (n_plain, t_plain) == (free["accepted"], free["attempted"])
    rc, msg = _code(lambda: ctx.list_draws(probed=True))
    assert rc == _abi.ERR_INVALID and "probe" in msg
    for put in (lambda: _host_probe(ctx, orc, s), lambda: _device_probe(ctx, s)):
        put()
        before = ctx.probe_stats()
        rec, n, t = ctx.list_draws()                               # a probe without the flag: the unprobed list, bit for bit
        assert (n, t) == (n_plain, t_plain) and _same_records(rec, plain) and ctx.probe_stats() == before
    ctx.set_occlusion_probe_device(None)
    assert _code(lambda: ctx.list_draws(probed=True))[0] == _abi.ERR_INVALID
    # the existing refusals come first and stay what they were
    pch = type(s["p"]).from_buffer_copy(s["p"])
    pch.abb_chromatic = 0.5
    ctx.set_params(pch)
    _host_probe(ctx, orc, s)
    assert _code(lambda: ctx.list_draws(probed=True))[0] == _abi.ERR_UNSUPPORTED
    ctx.set_params(s["p"])
    assert _code(lambda: ctx.list_draws(s["n"] - 10, 11, capacity=16, probed=True))[0] == _abi.ERR_INVALID
    rec, n, t = ctx.list_draws(5, 0, probed=True)
    assert rec.shape == (0,) and (n, t) == (0, 0)


def test_a_device_callback_that_fails_fails_the_call_and_the_context_stays_usable(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    want = pc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), None)      # user == NULL: returns 1, enqueues nothing
    rc, msg = _code(lambda: ctx.list_draws(probed=True))
    assert rc == _abi.ERR_INVALID and "returned 1" in msg
    _device_probe(ctx, s)
    rec, n, t = ctx.list_draws(probed=True)
    assert np.array_equal(_as_log(rec), want["log"]) and (n, t) == (want["accepted"], want["attempted"])


# ---- 5. the passes around a probed list ---------------------------------------------------------------------------------------------
def test_a_probed_list_between_two_passes_changes_neither(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    want = pc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name, frame=True)
    ctx.set_draw_log(1 << 20)
    _host_probe(ctx, orc, s)
    stalls = capi.process_stats()[1]

    def run():
        ctx.clear_frame(); ctx.redistribute(); ctx.resolve(); ctx.sync()
        c = ctx.counters()
        import common
        return common.sort_log(ctx.draw_log()), ctx.download_records(), (c.visits, c.redistributed_visits, c.attempted_draws, c.accepted_draws)

    log_a, rec_a, ctr_a = run()
    got, n, t = ctx.list_draws(probed=True)
    assert ctx.counters().accepted_draws == ctr_a[3]                # (the counter block is the pass's)
    log_b, rec_b, ctr_b = run()
    assert np.array_equal(log_a, want["log"]) and np.array_equal(log_a, log_b) and ctr_a == ctr_b
    assert np.array_equal(_as_log(got), log_a) and (n, t) == (ctr_a[3], ctr_a[2])
    drawn = np.zeros(rec_a.shape[0], bool)
    drawn[log_a[:, 2]] = True
    assert drawn.any() and not drawn.all() and _same_bits(rec_a[~drawn], rec_b[~drawn])
    assert np.array_equal(rec_a != 0, rec_b != 0)
    import common
    assert common.rel_err(rec_a[rec_b != 0], rec_b[rec_b != 0]) < 1e-5
    assert capi.process_stats()[1] == stalls                        # the list took no part in a streamed pass's turns
