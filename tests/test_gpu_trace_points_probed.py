"""lentil_hip_trace_points_probed (csrc/lentil_trace_points.h: trace_points_probed_kernel, trace_points_probed_spectral_kernel
and the turns around them) against the oracle's single-threaded pass under the same probe, against the unprobed
lentil_hip_trace_points, against lentil_hip_list_draws(LENTIL_DRAWS_PROBED), and against an exact model of the reference's try
loop (tests/trace_point_probe_cases.py; tests/test_trace_point_probe_cases.py holds its five small cases to the oracle and to
"the sphere bites").

Measured on an MI355X, the counts test_exact_model_and_the_segments_asked prints (turns: calls of the callback; lists: their
lengths) are in DESIGN.md 4.7.
"""
import collections
import ctypes as C

import numpy as np
import pytest

import common
import list_draw_probe_cases as pc
import oracle_lib
import trace_point_probe_cases as tpc
from pota_amd import _abi, capi
from test_gpu_list_draws import _as_log, _same_bits, _same_records, _sorted
from test_gpu_list_draws_probed import _code, _ctx, _device_probe, _host_probe

pytestmark = pytest.mark.gpu

VIGNETTED, OUTSIDE = tpc.VIGNETTED, tpc.OUTSIDE
KEYS = ("pixel", "xy", "sensor", "tries")


def _probed(ctx, b, k=None, rows=None, **kw):
    """the probed call over a batch of tpc.batch (rows: a subset of its points), everything asked for"""
    pick = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(a[rows]))
    kw.setdefault("time", pick(b["time"]))
    kw.setdefault("exempt", pick(b["exempt"]))
    return ctx.trace_points_probed(pick(b["cs"]), pick(b["pixel"]), b["k"] if k is None else k, pick(b["origin"]), want_sensor=True, **kw)


def _same(a, b, cols=None):
    """two result dicts, bit for bit (cols: of b, the columns a has)"""
    return all(_same_bits(np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key] if cols is None else b[key][:, cols])) for key in KEYS)


def _delta(after, before):
    return tuple(int(x) - int(y) for x, y in zip(after, before))


def _batch(ctx, name):
    plan, _ = ctx.plan_visits()
    return plan, tpc.batch(name, plan)


def _check_against_log(want, b, got):
    """the oracle's probed log: every record's query has its pixel; below the attempts made nothing else lands in the frame"""
    made, landed = tpc.made_from_log(want["log"], b["visits"], b["samples"])
    logged = landed != VIGNETTED
    assert int(logged.sum()) == want["log"].shape[0] == want["accepted"] and int(made.sum()) == want["attempted"]
    assert np.array_equal(got["pixel"][logged], landed[logged])
    below = np.arange(b["k"])[None, :] < made[:, None]
    assert (logged <= below).all() and (got["pixel"][below & ~logged] >= OUTSIDE).all()
    return logged


# ---- 1. every case against the oracle's pass, the unprobed call and the probed list; host callback, then device callback ------------
@pytest.mark.parametrize("name", pc.ALL)
def test_probed_points_are_the_oracles(orc, gpu_ctx_factory, monkeypatch, name):
    want = pc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, b = _batch(ctx, name)
    if s["model"] and s["samples"] > 0:                     # the columns give what the plan gives
        c = tpc.batch(name)
        assert all(np.array_equal(b[key], c[key]) for key in ("visits", "pixel", "samples")) and _same_bits(b["cs"] + np.float32(0), c["cs"] + np.float32(0))
    assert b["visits"].size == want["redistributed"]
    cs, pix, k = b["cs"], b["pixel"], b["k"]
    _host_probe(ctx, orc, s)
    before = ctx.probe_stats()
    got = _probed(ctx, b, lam=s["lam"])
    after = ctx.probe_stats()
    print(name, "points", cs.shape[0], "k", k, "asked / occluded / turns", _delta(after, before))
    assert ctx.trace_points_path() == s["path"]
    free = ctx.trace_points(cs, pix, k, lam=s["lam"], want_sensor=True, want_tries=True)

    # the device callback: the same arrays byte for byte, the same growth of the statistics
    _device_probe(ctx, s)
    dbefore, lbefore = ctx.probe_stats(), ctx.probe_device_stats()
    dgot = _probed(ctx, b, lam=s["lam"])
    dafter, lafter = ctx.probe_stats(), ctx.probe_device_stats()
    assert _same(dgot, got) and _delta(dafter, dbefore) == _delta(after, before)
    assert lafter[0] - lbefore[0] == after[2] - before[2]

    if name == "retries-1":
        assert (got["pixel"] == VIGNETTED).all() and not got["tries"].any() and after == before and want["accepted"] == 0
        return
    assert after[0] > before[0] and 0 < after[1] - before[1] < after[0] - before[0]
    assert 0 < after[2] - before[2] <= max(int(s["p"].vignetting_retries), 0) + 1
    logged = _check_against_log(want, b, got)
    if name == "skydome":
        assert 0 < int(b["exempt"].sum()) < b["exempt"].size and np.array_equal(np.nonzero(b["exempt"])[0], np.nonzero(np.isin(b["visits"], s["skydome"]))[0])

    # a query that got through is the unprobed call at the passing seed, which gets through at once
    at = np.nonzero(got["pixel"] != VIGNETTED)
    seed = (at[1] + got["tries"][at]).astype(np.uint32)
    one = ctx.trace_points(np.ascontiguousarray(cs[at[0]]), np.ascontiguousarray(pix[at[0]]), 1, first_attempt=seed, lam=s["lam"],
                           want_sensor=True, want_tries=True)
    assert not one["tries"].any() and all(_same_bits(one[key][:, 0], got[key][at]) for key in ("pixel", "xy", "sensor"))
    # an occluded try only adds to the vignetted ones before it
    assert (got["tries"] >= free["tries"]).all()
    untouched = got["tries"] == free["tries"]
    if s["camera"] == "tl":
        assert not got["tries"].any()
    else:
        assert all(_same_bits(got[key][untouched], free[key][untouched]) for key in KEYS)
        if name in ("retries3", "retries15", "samples-130"):
            assert (got["tries"] > free["tries"]).any()

    # the logged attempts: tries and xy are the probed list's records, bit for bit
    _host_probe(ctx, orc, s)
    rec, n_draws, _ = ctx.list_draws(lam=s["lam"], probed=True)
    r = _sorted(rec)
    assert np.array_equal(_as_log(rec), want["log"])
    i, m = np.searchsorted(b["visits"], r["visit"]), r["attempt"]
    assert logged[i, m].all() and np.array_equal(got["tries"][i, m], r["tries"]) and _same_bits(got["xy"][i, m], r["xy"])


# ---- 2. the exact model, and what the callback is asked --------------------------------------------------------------------------
def _gpu_model(orc, ctx, s, b, k, first=0, lens_ctx=None):
    """walk() over the lens outcome of every seed from the unprobed call (a seed gets through where no further try is made at
    it) and the sphere's answer about the test's own segment -> walk()'s dict with seg and occ"""
    retries = int(s["p"].vignetting_retries)
    seeds = k + max(retries, 0)
    fa = None if not first else np.full(b["cs"].shape[0], first, np.uint32)
    tp = (lens_ctx or ctx).trace_points(b["cs"], b["pixel"], seeds, first_attempt=fa, want_tries=True)
    passes = tp["tries"] == 0
    if retries == 0 or lens_ctx is not None:
        passes &= tp["pixel"] != VIGNETTED
    seg, occ = tpc.segments(orc, s, b, seeds, first)
    w = tpc.walk(passes, occ, k, retries)
    w.update(seg=seg, occ=occ)
    return w


@pytest.mark.parametrize("name", pc.MODEL)
def test_exact_model_and_the_segments_asked(orc, gpu_ctx_factory, monkeypatch, name):
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, b = _batch(ctx, name)
    retries = int(s["p"].vignetting_retries)
    w = tpc.oracle_model(orc, name) if name in tpc.ORACLE_MODEL else _gpu_model(orc, ctx, s, b, b["k"])
    watch = pc.Recorder(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data)
    ctx.set_occlusion_probe(watch.address, None, None)
    before = ctx.probe_stats()
    got = _probed(ctx, b)
    after = ctx.probe_stats()
    # tries and pass / fail of every query, beyond the attempts the pass makes too
    assert np.array_equal(got["tries"], w["tries"]) and np.array_equal(got["pixel"] != VIGNETTED, w["hit"] >= 0)
    # the segments: exactly the model's as a multiset of 24-byte rows
    asked = collections.Counter(row.tobytes() for row in watch.segments() + np.float32(0.0))
    assert asked == tpc.asked_counter(w["seg"], w["asked"])
    if int(s["p"].enable_dof) and not int(s["p"].bokeh_enable_image):
        # none twice -- but for two seeds of one point that draw the same aperture point: with 650 seeds per point the inputs
        # have such a pair (samples-130: seeds 230 and 641 of one point), two (point, seed) pairs with one segment
        same = collections.Counter(row.tobytes() for row in w["seg"].reshape(-1, 6))
        assert all(n == 1 for row, n in asked.items() if same[row] == 1) and all(n <= same[row] for row, n in asked.items())
    assert 0 < len(watch.calls) <= retries + 1 and all(watch.calls)
    occluded = int(watch.answers().astype(bool).sum())
    assert _delta(after, before) == (sum(watch.calls), occluded, len(watch.calls))
    assert occluded == int((w["asked"] & w["occ"]).sum())
    print(name, "points", b["cs"].shape[0], "k", b["k"], "turns", len(watch.calls), "lists", watch.calls)


# ---- 3. shapes: attempts around a slab, one point, first attempts, splits ---------------------------------------------------------
def test_shapes_first_attempts_and_splits(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, b = _batch(ctx, name)
    n = b["cs"].shape[0]
    _host_probe(ctx, orc, s)
    whole = _probed(ctx, b, k=130)
    free = ctx.trace_points(b["cs"], b["pixel"], 130, want_tries=True)
    assert (whole["tries"] > free["tries"]).any()
    for k in (1, 63, 64, 65):
        assert _same(_probed(ctx, b, k=k), whole, slice(0, k)), k
    # one point
    one = _probed(ctx, b, k=130, rows=slice(5, 6))
    assert all(_same_bits(one[key], whole[key][5:6]) for key in KEYS)
    # first attempts: uniform ones are shifted columns, differing ones are the uniform runs' rows
    choice = np.array([0, 7, 64, 1000], np.uint32)
    mixed_first = np.ascontiguousarray(choice[np.arange(n) % 4])
    mixed = _probed(ctx, b, k=20, first_attempt=mixed_first)
    for f in choice:
        uni = _probed(ctx, b, k=20, first_attempt=np.full(n, f, np.uint32))
        if f + 20 <= 130:
            assert _same(uni, whole, slice(int(f), int(f) + 20)), f
        rows = mixed_first == f
        assert rows.any() and all(_same_bits(mixed[key][rows], uni[key][rows]) for key in KEYS), f
    # the last seeds of the 32-bit range: no wrap, host pointers accept them, the model's results at those seeds
    k, retries = 8, int(s["p"].vignetting_retries)
    top = (1 << 32) - 1 - (k + retries)
    p0 = type(s["p"]).from_buffer_copy(s["p"])
    p0.vignetting_retries = 0                                 # (one try per seed, so that the unprobed call reaches the last seed)
    lens_ctx = gpu_ctx_factory()
    lens_ctx.set_params(p0)
    lens_ctx.set_lens(s["table"])
    w = _gpu_model(orc, ctx, s, b, k, first=top, lens_ctx=lens_ctx)
    high = _probed(ctx, b, k=k, first_attempt=np.full(n, top, np.uint32))
    assert np.array_equal(high["tries"], w["tries"]) and np.array_equal(high["pixel"] != VIGNETTED, w["hit"] >= 0) and (w["hit"] >= 0).any()
    assert (w["asked"] & w["occ"]).any()
    rc, msg = _code(lambda: _probed(ctx, b, k=k, first_attempt=np.full(n, top + 1, np.uint32)))
    assert rc == _abi.ERR_INVALID and "32 bits" in msg
    # split by points into three calls, and by attempts into two
    c1, c2 = n // 5 + 3, n // 2 + 7
    parts = [_probed(ctx, b, k=130, rows=slice(lo, hi)) for lo, hi in ((0, c1), (c1, c2), (c2, n))]
    assert all(_same_bits(np.concatenate([q[key] for q in parts]), whole[key]) for key in KEYS)
    head = _probed(ctx, b, k=50)
    tail = _probed(ctx, b, k=80, first_attempt=np.full(n, 50, np.uint32))
    assert _same(head, whole, slice(0, 50)) and _same(tail, whole, slice(50, 130))


# ---- 4. pointers and context state ---------------------------------------------------------------------------------------------
def test_device_pointers_and_exempt_points(orc, gpu_ctx_factory, monkeypatch):
    import torch
    name = "samples-65"
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, b = _batch(ctx, name)
    n, k = b["cs"].shape[0], b["k"]
    _device_probe(ctx, s)
    host = _probed(ctx, b)
    dev = "cuda:%d" % ctx.device
    put = lambda a: torch.from_numpy(np.array(a)).to(dev)      # noqa: E731
    first = np.zeros(n, np.uint32)
    torch.cuda.synchronize()
    got = ctx.trace_points_probed(put(b["cs"]), put(b["pixel"].view(np.int32)), k, put(b["origin"]), first_attempt=put(first.view(np.int32)),
                                  time=put(b["time"]), exempt=put(b["exempt"]), want_sensor=True)
    assert all(t.is_cuda for t in got.values())
    back = {key: t.cpu().numpy() for key, t in got.items()}
    back["pixel"] = back["pixel"].view(np.uint32)
    assert _same(back, host) and (host["pixel"] < OUTSIDE).any()
    # every point exempt: the unprobed arrays, and nobody is asked -- under either callback
    free = ctx.trace_points(b["cs"], b["pixel"], k, want_sensor=True, want_tries=True)
    assert not _same(host, free)
    for setp in (lambda: _device_probe(ctx, s), lambda: _host_probe(ctx, orc, s)):
        setp()
        before, lbefore = ctx.probe_stats(), ctx.probe_device_stats()
        assert _same(_probed(ctx, b, exempt=np.ones(n, np.uint8)), free)
        assert ctx.probe_stats() == before and ctx.probe_device_stats()[0] == lbefore[0]
    # no point exempt by a NULL pointer is no point exempt by zeros
    assert _same(_probed(ctx, b, exempt=None, time=None), host)


def test_skydome_points_by_the_rule_match_the_oracles_log(orc, gpu_ctx_factory, monkeypatch):
    name = "skydome"
    want = pc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, b = _batch(ctx, name)
    _host_probe(ctx, orc, s)
    got = _probed(ctx, b)
    _check_against_log(want, b, got)
    # the exempt points are the unprobed call's; with nobody exempt the sphere takes some of their draws
    free = ctx.trace_points(b["cs"], b["pixel"], b["k"], want_sensor=True, want_tries=True)
    ex = b["exempt"] != 0
    assert ex.any() and all(_same_bits(got[key][ex], free[key][ex]) for key in KEYS)
    bare = _probed(ctx, b, exempt=None)
    assert (bare["tries"][ex] > free["tries"][ex]).any() and all(_same_bits(bare[key][~ex], got[key][~ex]) for key in KEYS)


# ---- 5. a wavelength per point ---------------------------------------------------------------------------------------------------
def test_a_wavelength_per_point(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, b = _batch(ctx, name)
    n = b["cs"].shape[0]
    _host_probe(ctx, orc, s)
    scalar = _probed(ctx, b)
    assert _same(_probed(ctx, b, lambdas=np.zeros(n)), scalar) and ctx.trace_points_path() == s["path"]
    lams = np.array([0.45, 0.55, 0.65, 0.0])
    lambdas = np.ascontiguousarray(lams[np.arange(n) % 4])
    got = _probed(ctx, b, lambdas=lambdas, lam=0.61)            # (lam is ignored beside lambdas)
    for j, lam in enumerate(lams):
        rows = np.nonzero(np.arange(n) % 4 == j)[0]
        sub = _probed(ctx, b, rows=rows, lam=float(lam))
        assert all(_same_bits(got[key][rows], sub[key]) for key in KEYS), lam
    blue = _probed(ctx, b, lam=0.45)
    assert not _same_bits(blue["xy"], scalar["xy"])            # (the wavelength matters)
    # the same through device pointers, under the device callback
    import torch
    _device_probe(ctx, s)
    dev = "cuda:%d" % ctx.device
    put = lambda a: torch.from_numpy(np.array(a)).to(dev)      # noqa: E731
    torch.cuda.synchronize()
    dgot = ctx.trace_points_probed(put(b["cs"]), put(b["pixel"].view(np.int32)), b["k"], put(b["origin"]), time=put(b["time"]),
                                   exempt=put(b["exempt"]), lambdas=put(lambdas), want_sensor=True)
    back = {key: t.cpu().numpy() for key, t in dgot.items()}
    back["pixel"] = back["pixel"].view(np.uint32)
    assert _same(back, got)


def test_the_interpreter_and_the_thin_lens_with_wavelengths(orc, gpu_ctx_factory, monkeypatch):
    for name in ("lens-interpreter", "tl-plain"):
        ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
        plan, b = _batch(ctx, name)
        n = b["cs"].shape[0]
        _host_probe(ctx, orc, s)
        scalar = _probed(ctx, b)
        lambdas = np.ascontiguousarray(np.array([0.45, 0.65])[np.arange(n) % 2])
        got = _probed(ctx, b, lambdas=lambdas)
        assert ctx.trace_points_path() == s["path"]
        if s["camera"] == "tl":
            assert _same(got, scalar)                            # the thin lens reads no wavelength
        else:
            for j, lam in enumerate((0.45, 0.65)):
                rows = np.nonzero(np.arange(n) % 2 == j)[0]
                sub = _probed(ctx, b, rows=rows, lam=lam)
                assert all(_same_bits(got[key][rows], sub[key]) for key in KEYS)


# ---- 6. buffers that grow --------------------------------------------------------------------------------------------------------
def test_a_capped_first_turn_grows_its_buffers(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    runs = []
    for cap in (None, "1024"):
        if cap:
            monkeypatch.setenv("LENTIL_POINTS_PROBE_CAP", cap)      # (read when the context is made)
        ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
        plan, b = _batch(ctx, name)
        watch = pc.Recorder(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data)
        ctx.set_occlusion_probe(watch.address, None, None)
        before = ctx.probe_stats()
        got = _probed(ctx, b)
        assert _delta(ctx.probe_stats(), before) == (sum(watch.calls), int(watch.answers().astype(bool).sum()), len(watch.calls))
        runs.append((got, collections.Counter(row.tobytes() for row in watch.segments()), list(watch.calls)))
        if cap:
            _device_probe(ctx, s)
            assert _same(_probed(ctx, b), got)
    (free_got, free_asked, free_calls), (cap_got, cap_asked, cap_calls) = runs
    print("uncapped lists", free_calls, "capped lists", cap_calls)
    assert _same(cap_got, free_got) and cap_asked == free_asked and max(free_asked.values()) == 1
    assert len(cap_calls) > len(free_calls) and cap_calls[0] == 1024 and max(free_calls) > 1024 and all(cap_calls)


# ---- 7. refusals and neighbours --------------------------------------------------------------------------------------------------
def test_refusals(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name)
    plan, b = _batch(ctx, name)
    rc, msg = _code(lambda: _probed(ctx, b))
    assert rc == _abi.ERR_INVALID and "probe" in msg
    _host_probe(ctx, orc, s)
    want = _probed(ctx, b)
    # origin missing: the struct itself, and its required member
    n, k = b["cs"].shape[0], 4
    out = np.empty((n, k), np.uint32)
    req = _abi.PointBatch()
    req.n_points, req.attempts, req.cs, req.pixel, req.out_pixel = n, k, b["cs"].ctypes.data, b["pixel"].ctypes.data, out.ctypes.data
    assert ctx.lib.lentil_hip_trace_points_probed(ctx.h, C.byref(req), None) == _abi.ERR_INVALID
    assert ctx.lib.lentil_hip_trace_points_probed(ctx.h, C.byref(req), C.byref(_abi.PointProbe())) == _abi.ERR_INVALID
    req.n_points = 0                                          # no points: nothing is launched, nothing is needed
    assert ctx.lib.lentil_hip_trace_points_probed(ctx.h, C.byref(req), None) == _abi.OK
    req.n_points, req.attempts = n, 0
    assert ctx.lib.lentil_hip_trace_points_probed(ctx.h, C.byref(req), None) == _abi.ERR_INVALID
    # polynomial optics with abb_chromatic != 0 stays refused
    pch = type(s["p"]).from_buffer_copy(s["p"])
    pch.abb_chromatic = 0.5
    ctx.set_params(pch)
    rc, msg = _code(lambda: _probed(ctx, b))
    assert rc == _abi.ERR_UNSUPPORTED and "abb_chromatic" in msg
    ctx.set_params(s["p"])
    # a device callback that fails fails the call; the context stays usable
    ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), None)      # user == NULL: returns 1, enqueues nothing
    rc, msg = _code(lambda: _probed(ctx, b))
    assert rc == _abi.ERR_INVALID and "returned 1" in msg
    _device_probe(ctx, s)
    assert _same(_probed(ctx, b), want)


def test_a_probed_batch_changes_neither_its_neighbours_nor_the_passes(orc, gpu_ctx_factory, monkeypatch):
    name = "retries3"
    want = pc.oracle_pass(orc, name)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, name, frame=True)
    plan, b = _batch(ctx, name)
    ctx.set_draw_log(1 << 20)
    _host_probe(ctx, orc, s)
    stalls = capi.process_stats()[1]

    def run():
        ctx.clear_frame(); ctx.redistribute(); ctx.resolve(); ctx.sync()
        c = ctx.counters()
        return common.sort_log(ctx.draw_log()), ctx.download_records(), (c.visits, c.redistributed_visits, c.attempted_draws, c.accepted_draws)

    def neighbours():
        free = ctx.trace_points(b["cs"], b["pixel"], b["k"], want_sensor=True, want_tries=True)
        return free, ctx.list_draws(probed=True)

    log_a, rec_a, ctr_a = run()
    free_a, list_a = neighbours()
    got = _probed(ctx, b)
    assert ctx.counters().accepted_draws == ctr_a[3]                # (the counter block is the pass's)
    free_b, list_b = neighbours()
    log_b, rec_b, ctr_b = run()
    assert _same(free_a, free_b) and _same_records(list_a[0], list_b[0]) and list_a[1:] == list_b[1:]
    assert np.array_equal(log_a, want["log"]) and np.array_equal(log_a, log_b) and ctr_a == ctr_b
    _check_against_log(want, b, got)
    drawn = np.zeros(rec_a.shape[0], bool)
    drawn[log_a[:, 2]] = True
    assert drawn.any() and not drawn.all() and _same_bits(rec_a[~drawn], rec_b[~drawn])
    assert np.array_equal(rec_a != 0, rec_b != 0) and common.rel_err(rec_a[rec_b != 0], rec_b[rec_b != 0]) < 1e-5
    assert capi.process_stats()[1] == stalls                        # the batch took no part in a streamed pass's turns
