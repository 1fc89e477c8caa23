"""lentil_hip_list_draws_spectral on the GPU (csrc/lentil_list_draws.h: list_draws_spectral_kernel and
list_draws_probed_spectral_kernel) against the oracle's single-threaded passes, one per wavelength
(tests/list_draw_spectral_cases.py), and against the scalar call, bit for bit: there is no tolerance anywhere.
tests/test_list_draw_spectral_cases.py holds the cases to lists that depend on the wavelength.

What a record holds besides the oracle's log -- tries and xy -- is taken from orc_trace_ray_bw_po at the visit's wavelength
and the sensor -> pixel mapping of tests/trace_point_cases.py, as the sibling tests take it from trace_points: of an unprobed
list for (plan.cs, plan.pixel, attempt); of a probed list for the seed attempt + tries, which gets through the lens at once,
and an occluded try only adds to the vignetted ones before it (the exact tries of a probed list are the scalar call's, below).
"""
import collections
import ctypes as C

import numpy as np
import pytest

import list_draw_cases as lc
import list_draw_probe_cases as pc
import list_draw_spectral_cases as ls
import oracle_lib
from pota_amd import _abi, capi
from test_gpu_list_draws import GUARD, _as_log, _key, _same_bits, _same_records, _sorted

pytestmark = pytest.mark.gpu


def _ctx(make, monkeypatch, kind, name, jit=False):
    s = ls.setup(kind, name)
    if s["path"] == _abi.DRAWS_PATH_INTERPRETER and s["lens_mode"] is None and not jit:
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
    ctx.upload_visits(s["visits"])
    return ctx, s


def _host_probe(ctx, orc, s):
    ctx.set_occlusion_probe(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data, s["c2w"])


def _device_probe(ctx, s):
    ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), s["sphere"].ctypes.data, s["c2w"])


def _watch(ctx, orc, s):
    w = pc.Recorder(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data)
    ctx.set_occlusion_probe(w.address, None, s["c2w"])
    return w


def _code(fn):
    with pytest.raises(capi.LentilError) as e:
        fn()
    return e.value.code, str(e.value)


def _attempts(plan, log, first=0, n=None):
    """the attempts the visits first ... first + n - 1 made, from the plan and the expected log"""
    n = plan.shape[0] - first if n is None else n
    red = np.nonzero(plan["flags"] & _abi.PLAN_REDISTRIBUTE)[0]
    red = red[(red >= first) & (red < first + n)]
    return int(ls.attempts_per_visit(log, red, plan["samples"][red]).sum())


def _in_range(a, first, n):
    """the rows of a log, or the records of a list, whose visit lies in first ... first + n - 1"""
    v = a["visit"] if a.dtype == _abi.Draw else a[:, 0]
    return a[(v >= first) & (v < first + n)]


# ---- 1. against the oracle, per case: one pass per wavelength, of each the visits that carry it ------------------------------
@pytest.mark.parametrize("kind,name", ls.ALL, ids=ls.IDS)
def test_the_list_is_the_oracles_visit_by_visit(orc, gpu_ctx_factory, monkeypatch, kind, name):
    lam = ls.lambdas(kind, name)
    want = ls.expected_log(orc, kind, name, lam)
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    probed = kind == "probed"
    plan, totals = ctx.plan_visits()
    want_attempts = _attempts(plan, want)
    if probed:
        _host_probe(ctx, orc, s)
    before = ctx.probe_stats()
    rec, n_draws, attempts = ctx.list_draws(lam=123.0, lambdas=lam, probed=probed)          # (lam is ignored)
    after = ctx.probe_stats()
    print(kind, name, "totals", totals, "draws", n_draws, "attempts", attempts, "want", want.shape[0], want_attempts)
    assert ctx.list_draws_path() == s["path"]
    assert rec.dtype == _abi.Draw and rec.shape == (n_draws,) and totals[2] >= n_draws
    assert n_draws == want.shape[0] > 0 and attempts == want_attempts
    got = _as_log(rec)
    assert got.shape == want.shape and np.array_equal(got, want)
    r = _sorted(rec)
    fl = np.floor(r["xy"]).astype(np.int64)
    assert np.array_equal(fl[:, 0] + fl[:, 1] * int(s["p"].xres), r["pixel"].astype(np.int64))

    if probed:
        # the device callback: the same list byte for byte, the same segments in the same number of turns
        assert after[0] > before[0] and after[2] > before[2]
        _device_probe(ctx, s)
        dbefore = ctx.probe_stats()
        drec, dn, dattempts = ctx.list_draws(lambdas=lam, probed=True)
        dafter = ctx.probe_stats()
        assert (dn, dattempts) == (n_draws, attempts) and _same_records(rec, drec)
        assert tuple(a - b for a, b in zip(dafter, dbefore)) == tuple(a - b for a, b in zip(after, before))
    else:
        assert after == before

    # tries and xy: the oracle's backward trace at the visit's wavelength
    if s["camera"] == "tl":
        assert not r["tries"].any()
        scalar = ctx.list_draws(probed=probed)
        assert (scalar[1], scalar[2]) == (n_draws, attempts) and _same_records(scalar[0], rec)
        return
    cs, pix = plan["cs"][r["visit"]], plan["pixel"][r["visit"]]
    free = ls.trace_records(orc, s, cs, pix, r["visit"], r["attempt"], lam)
    if not probed:
        t = free
        assert np.array_equal(t["tries"], r["tries"])
    else:
        t = ls.trace_records(orc, s, cs, pix, r["visit"], r["attempt"] + r["tries"].astype(np.uint32), lam)
        assert not t["tries"].any() and (r["tries"] >= free["tries"]).all()
    assert t["ok"].all() and np.array_equal(t["pixel"], r["pixel"]) and _same_bits(t["xy"], r["xy"])


# ---- 2. against the scalar call ------------------------------------------------------------------------------------------------------
SCALAR_CASES = [("plain", "samples-65"), ("plain", "lens-interpreter"), ("probed", "retries3"), ("probed", "lens-anamorphic")]


@pytest.mark.parametrize("kind,name", SCALAR_CASES, ids=["%s/%s" % k for k in SCALAR_CASES])
def test_a_constant_wavelength_is_the_scalar_call(orc, gpu_ctx_factory, monkeypatch, kind, name):
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    probed = kind == "probed"
    if probed:
        _host_probe(ctx, orc, s)
    lists = []
    for lam in (ls.LAM_BLUE, 0.0, 0.5712345678901234):
        a = ctx.list_draws(lambdas=np.full(s["n"], lam), lam=ls.LAM_RED, probed=probed)
        b = ctx.list_draws(lam=lam, probed=probed)
        assert (a[1], a[2]) == (b[1], b[2]) and a[1] > 0 and _same_records(a[0], b[0])
        lists.append(b[0])
    assert not _same_records(lists[0], lists[1])                                        # (the wavelength shows)
    # 0 is params.lambda_bw, entry by entry
    by_name = ctx.list_draws(lambdas=np.full(s["n"], ls.LAMBDA_BW), probed=probed)
    assert _same_records(by_name[0], lists[1])
    mixed = ls.lambdas(kind, name)
    full = np.where(mixed == 0.0, ls.LAMBDA_BW, mixed)
    a, b = ctx.list_draws(lambdas=mixed, probed=probed), ctx.list_draws(lambdas=full, probed=probed)
    assert (a[1], a[2]) == (b[1], b[2]) and _same_records(a[0], b[0])


@pytest.mark.parametrize("kind,name", SCALAR_CASES, ids=["%s/%s" % k for k in SCALAR_CASES])
def test_blocks_are_three_scalar_calls(orc, gpu_ctx_factory, monkeypatch, kind, name):
    """a wavelength constant over three sub-ranges whose cut points are no multiples of 64: the union of three scalar calls --
    records and attempts; probed, also the set of segments asked, none twice, and the statistics' sums"""
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    probed = kind == "probed"
    n = s["n"]
    c1, c2 = ls.cuts(n)
    blocks = ls.lambdas(kind, name, "blocks")
    watch = _watch(ctx, orc, s) if probed else None
    before = ctx.probe_stats()
    rec, n_draws, attempts = ctx.list_draws(lambdas=blocks, probed=probed)
    mid = ctx.probe_stats()
    n_lists = len(watch._seg) if probed else 0
    parts = [ctx.list_draws(a, b - a, lam=lam, probed=probed) for (a, b), lam in zip(((0, c1), (c1, c2), (c2, n)), ls.BLOCKS)]
    after = ctx.probe_stats()
    assert all(q[1] for q in parts) and sum(q[1] for q in parts) == n_draws and sum(q[2] for q in parts) == attempts
    assert _same_records(np.concatenate([q[0] for q in parts]), rec)
    # ... and it is what the oracle lists
    assert np.array_equal(_as_log(rec), ls.expected_log(orc, kind, name, blocks))
    if probed:
        seg = watch.segments()
        k = sum(watch.calls[:n_lists])
        whole = collections.Counter(row.tobytes() for row in seg[:k])
        thirds = collections.Counter(row.tobytes() for row in seg[k:])
        assert whole == thirds and len(whole) > 0
        if int(s["p"].enable_dof) and not int(s["p"].bokeh_enable_image):
            assert max(whole.values()) == 1
        d1, d2 = tuple(a - b for a, b in zip(mid, before)), tuple(a - b for a, b in zip(after, mid))
        assert d1[0] == d2[0] == k and d1[1] == d2[1] > 0
    else:
        assert after == before


# ---- 3. ranges and the grid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("plain", "samples-65"), ("probed", "samples-65")], ids=["plain", "probed"])
def test_ranges_take_their_wavelengths_by_the_range(orc, gpu_ctx_factory, monkeypatch, kind, name):
    """first_visit no multiple of 64, an end inside a group: the whole list filtered to the range -- which a kernel that
    indexes lambdas by the stream does not give.  And the list as a set under a grid of one block: the grid is sized from the
    range (a wave per 64 visits, four waves per block), so a range of at most 256 visits is walked by one block."""
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    probed = kind == "probed"
    if probed:
        _host_probe(ctx, orc, s)
    lam = ls.lambdas(kind, name)
    want = ls.expected_log(orc, kind, name, lam)
    plan, totals = ctx.plan_visits()
    whole, n_draws, attempts = ctx.list_draws(lambdas=lam, probed=probed)
    assert np.array_equal(_as_log(whole), want)
    n = s["n"]
    for first, count in ((77, 1000), (n // 2 + 21, n // 3 + 5), (n - 333, 333)):       # (the last one ends with the stream)
        assert first % 64 and ((first + count) % 64 or first + count == n)
        rec, nd, att = ctx.list_draws(first, count, lambdas=lam[first:first + count], probed=probed)
        mine = _in_range(whole, first, count)
        assert nd == mine.shape[0] > 0 and _same_records(rec, mine)
        assert att == _attempts(plan, _in_range(want, first, count), first, count)
        # the same range with the stream's first wavelengths instead: another list
        other = ctx.list_draws(first, count, lambdas=lam[:count], probed=probed)[0]
        assert not _same_records(other, mine)
    # one block per call: ranges of 256 visits and less, from an odd start
    starts = list(range(0, n, 251))
    parts = [ctx.list_draws(a, min(251, n - a), lambdas=lam[a:a + 251], probed=probed) for a in starts]
    assert sum(q[1] for q in parts) == n_draws and sum(q[2] for q in parts) == attempts
    assert _same_records(np.concatenate([q[0] for q in parts]), whole)


# ---- 4. forms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("plain", "samples-65"), ("probed", "samples-65")], ids=["plain", "probed"])
def test_device_pointers_counting_call_and_capacity(orc, gpu_ctx_factory, monkeypatch, kind, name):
    import torch
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    probed = kind == "probed"
    flags = _abi.DRAWS_PROBED if probed else 0
    if probed:
        _device_probe(ctx, s)
    lam = ls.lambdas(kind, name)
    want = ls.expected_log(orc, kind, name, lam)
    whole, n_draws, attempts = ctx.list_draws(lambdas=lam, probed=probed)
    assert np.array_equal(_as_log(whole), want)
    n = s["n"]

    # device=True: the records stay on the GPU, the wavelengths are a tensor there
    t_lam = torch.from_numpy(lam.copy()).cuda()
    drec, dn, dt = ctx.list_draws(device=True, lambdas=t_lam, probed=probed)
    assert drec.is_cuda and (dn, dt) == (n_draws, attempts)
    assert _same_records(drec.cpu().numpy().view(_abi.Draw).reshape(-1)[:dn], whole)
    for bad in (lam, t_lam.cpu(), t_lam.float(), t_lam[:-1], torch.stack([t_lam, t_lam], 1)[:, 0]):
        with pytest.raises(ValueError, match="lambdas"):      # numpy beside tensors, not on the GPU, fp32, too short, strided
            ctx.list_draws(device=True, lambdas=bad, probed=probed)
    with pytest.raises(ValueError, match="lambdas"):
        ctx.list_draws(lambdas=t_lam, probed=probed)          # a tensor beside numpy

    # a counting call, then the real one with exactly that room
    nd, att = C.c_uint64(), C.c_uint64()
    req = _abi.DrawList()
    req.first_visit, req.n_visits, req.capacity, req.out, req.flags = 0, n, 0, None, flags
    req.n_draws, req.attempts = C.pointer(nd), C.pointer(att)
    assert ctx.lib.lentil_hip_list_draws_spectral(ctx.h, C.byref(req), lam.ctypes.data) == _abi.OK
    assert (nd.value, att.value) == (n_draws, attempts)
    again, n2, t2 = ctx.list_draws(capacity=nd.value, lambdas=lam, probed=probed)
    assert (n2, t2) == (n_draws, attempts) and _same_records(again, whole)

    # a capacity below n_draws: the full count, nothing behind out[capacity], some `capacity` records of the list
    cap = n_draws - 1 if not probed else 37
    out = np.full((cap + GUARD) * 32, 0xA5, np.uint8).view(_abi.Draw)
    req.capacity, req.out = cap, out.ctypes.data
    assert ctx.lib.lentil_hip_list_draws_spectral(ctx.h, C.byref(req), lam.ctypes.data) == _abi.OK
    assert (nd.value, att.value) == (n_draws, attempts)
    assert (out[cap:].view(np.uint8) == 0xA5).all()
    head = _as_log(out[:cap])
    assert np.unique(_key(head)).size == cap and np.isin(_key(head), _key(want)).all()
    assert np.array_equal(want[np.searchsorted(_key(want), _key(head))], head)
    dev = torch.full((cap + GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    req.out, req.flags = dev.data_ptr(), flags | _abi.DRAWS_DEVICE_POINTERS
    assert ctx.lib.lentil_hip_list_draws_spectral(ctx.h, C.byref(req), t_lam.data_ptr()) == _abi.OK and nd.value == n_draws
    host = dev.cpu().numpy()
    assert (host[cap:] == 0xA5).all() and np.unique(_as_log(host[:cap].view(_abi.Draw).reshape(-1)), axis=0).shape[0] == cap


def test_a_table_compiled_at_run_time_is_served_by_the_interpreter(orc, gpu_ctx_factory, monkeypatch):
    kind, name = "plain", "lens-anamorphic"
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name, jit=True)
    assert not ctx.lens_is_compiled()
    ctx.lens_jit_wait(600.0)                                  # (seconds from the cache on disk)
    assert ctx.lens_jit_status()[0] == 2, ctx.lens_jit_status()
    lam = ls.lambdas(kind, name)
    rec, n_draws, attempts = ctx.list_draws(lambdas=lam)
    assert ctx.list_draws_path() == _abi.DRAWS_PATH_INTERPRETER
    assert np.array_equal(_as_log(rec), ls.expected_log(orc, kind, name, lam))


# ---- 5. the thin lens ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "probed"])
def test_the_thin_lens_ignores_the_wavelengths(orc, gpu_ctx_factory, monkeypatch, kind):
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, "tl-plain")
    probed = kind == "probed"
    if probed:
        _host_probe(ctx, orc, s)
    n = s["n"]
    want, n_draws, attempts = ctx.list_draws(probed=probed)
    assert n_draws > 0 and np.array_equal(_as_log(want), ls.oracle_pass(orc, kind, "tl-plain", 0.0)["log"])
    for lam in (ls.lambdas(kind, "tl-plain"), np.full(n, 123.0)):
        rec, nd, att = ctx.list_draws(lambdas=lam, probed=probed)
        assert ctx.list_draws_path() == _abi.DRAWS_PATH_THIN_LENS
        assert (nd, att) == (n_draws, attempts) and _same_records(rec, want)
    out = np.zeros(n_draws, _abi.Draw)                        # lambdas NULL
    nd, att = C.c_uint64(), C.c_uint64()
    req = _abi.DrawList()
    req.first_visit, req.n_visits, req.capacity, req.out, req.flags = 0, n, n_draws, out.ctypes.data, _abi.DRAWS_PROBED if probed else 0
    req.n_draws, req.attempts = C.pointer(nd), C.pointer(att)
    assert ctx.lib.lentil_hip_list_draws_spectral(ctx.h, C.byref(req), None) == _abi.OK
    assert (nd.value, att.value) == (n_draws, attempts) and _same_records(out, want)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_listing(orc, gpu_ctx_factory, monkeypatch):
    kind, name = "probed", "retries3"
    ctx, s = _ctx(gpu_ctx_factory, monkeypatch, kind, name)
    n = s["n"]
    lam = ls.lambdas(kind, name)
    free, n_free, t_free = ctx.list_draws(lambdas=lam)

    def still_lists():
        rec, nd, att = ctx.list_draws(lambdas=lam)
        assert (nd, att) == (n_free, t_free) and nd > 0 and _same_records(rec, free)

    def raw(n_visits, lambdas, capacity=0, out=None, n_draws=True, flags=0, first=0):
        nd = C.c_uint64(7)
        req = _abi.DrawList()
        req.first_visit, req.n_visits, req.capacity, req.out, req.flags = first, n_visits, capacity, out, flags
        req.n_draws = C.pointer(nd) if n_draws else None
        return ctx.lib.lentil_hip_list_draws_spectral(ctx.h, C.byref(req), lambdas), nd.value

    # lambdas NULL with polynomial optics
    assert raw(n, None)[0] == _abi.ERR_INVALID
    still_lists()
    assert raw(0, None) == (_abi.OK, 0)                                                          # n_visits == 0, whatever the pointer
    # where the scalar call refuses
    assert raw(n, lam.ctypes.data, capacity=16)[0] == _abi.ERR_INVALID                            # out NULL with capacity > 0
    assert raw(n, lam.ctypes.data, n_draws=False)[0] == _abi.ERR_INVALID                          # n_draws NULL
    assert raw(11, lam.ctypes.data, first=n - 10)[0] == _abi.ERR_INVALID                          # a range beyond the stream
    assert ctx.lib.lentil_hip_list_draws_spectral(ctx.h, None, lam.ctypes.data) == _abi.ERR_INVALID
    still_lists()
    # probed without a probe
    rc, msg = _code(lambda: ctx.list_draws(lambdas=lam, probed=True))
    assert rc == _abi.ERR_INVALID and "probe" in msg
    still_lists()
    # abb_chromatic != 0: the chromatic list has no wavelength per visit, with the flag or without
    for c in (0.5, -0.5):
        pch = type(s["p"]).from_buffer_copy(s["p"])
        pch.abb_chromatic = c
        ctx.set_params(pch)
        for channels in (False, True):
            rc, msg = _code(lambda: ctx.list_draws(0, n, capacity=16, lambdas=lam, channels=channels))
            assert rc == _abi.ERR_UNSUPPORTED and "abb_chromatic" in msg
        assert ctx.list_draws(0, n, channels=True)[1] > 0                                         # (the scalar call serves the mode)
        ctx.set_params(s["p"])
        still_lists()
    # the flag changes nothing where the plain list serves the mode
    rec, nd, att = ctx.list_draws(lambdas=lam, channels=True)
    assert (nd, att) == (n_free, t_free) and _same_records(rec, free)
    # under the probe the context lists what the oracle lists
    _host_probe(ctx, orc, s)
    rec, nd, att = ctx.list_draws(lambdas=lam, probed=True)
    assert np.array_equal(_as_log(rec), ls.expected_log(orc, kind, name, lam))


# ---- 7. the scalar calls are what they were -----------------------------------------------------------------------------------------
def test_the_scalar_calls_around_a_spectral_one(orc, gpu_ctx_factory, monkeypatch):
    """one plain and one probed case of the existing tables, through lentil_hip_list_draws, before and after a spectral call on
    the same context: their oracle lists"""
    for table, name, probed in ((lc, "lambda", False), (pc, "retries3", True)):
        s = table.setup(name)
        want = table.oracle_pass(orc, name)
        ctx = gpu_ctx_factory()
        ctx.set_params(s["p"])
        ctx.set_lens(s["table"])
        ctx.upload_visits(s["visits"])
        if probed:
            _host_probe(ctx, orc, s)
        lam = np.asarray(ls.PALETTE)[np.arange(s["n"]) % 4]
        seen = []
        for turn in range(2):
            rec, n_draws, attempts = ctx.list_draws(lam=s["lam"], probed=probed)
            assert (n_draws, attempts) == (want["accepted"], want["attempted"]) and np.array_equal(_as_log(rec), want["log"])
            seen.append(rec)
            if turn == 0:
                other = ctx.list_draws(lambdas=lam, probed=probed)
                assert other[1] > 0 and not _same_records(other[0], rec)
        assert _same_records(seen[0], seen[1])
