"""Scene points traced backward through the lens in batches on the GPU (lentil_hip_trace_points,
csrc/lentil_trace_points.h) against the oracle.

Polynomial optics: every query of every case of tests/trace_point_cases.py against orc_trace_ray_bw_po -- which queries
are vignetted, the try counts and the sensor positions bit for bit -- and against the oracle's sensor -> pixel mapping
restated in fp64 (trace_point_cases.pixel_mapping), bit for bit.  Both cameras: against the draw log of the oracle's own
pass.  tests/test_trace_point_cases.py holds the cases to the classes of queries they are there for.
"""
import ctypes as C

import numpy as np
import pytest

import common
import trace_point_cases as tc
from pota_amd import _abi, capi

pytestmark = pytest.mark.gpu

QUIET = np.uint64(1) << np.uint64(51)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _quiet_nans(a):
    return bool(np.isnan(a).all() and ((_bits(a) & QUIET) != 0).all())


def _po_ctx(make, s):
    ctx = make()
    ctx.set_params(s["p"])
    ctx.set_lens(s["table"])
    if s["bokeh"]:
        import bokeh_tables
        ctx.set_bokeh(bokeh_tables.tables(s["bokeh"]))
    if s["lens_mode"] is not None:
        ctx.set_lens_mode(s["lens_mode"])
    return ctx


def _trace(ctx, s, **kw):
    kw.setdefault("want_sensor", True)
    kw.setdefault("want_tries", True)
    return ctx.trace_points(s["cs"], s["pixel"], s["k"], first_attempt=s["first"], lam=s["lam"], **kw)


def _check_po(got, want, p):
    ok = want["ok"]
    assert got["pixel"].dtype == np.uint32 and got["pixel"].shape == ok.shape
    assert np.array_equal(got["pixel"] == tc.VIGNETTED, ~ok)                       # vignetted exactly where the oracle returns 0
    assert np.array_equal(got["tries"][ok], want["tries"][ok])
    assert _same_bits(got["sensor"][ok], want["sensor"][ok])
    assert _same_bits(got["xy"][ok], want["xy"][ok])
    bad = np.nonzero(got["pixel"] != want["pixel"])
    assert bad[0].size == 0, (bad[0][:8], got["pixel"][bad][:8], want["pixel"][bad][:8])
    assert _quiet_nans(got["xy"][~ok]) and _quiet_nans(got["sensor"][~ok])
    if (~ok).any():                                                                # every try was made and failed
        assert np.array_equal(got["tries"][~ok], want["tries"][~ok])
        assert (got["tries"][~ok] == max(int(p.vignetting_retries) + 1, 0)).all()


# ---- 1. polynomial optics against the oracle, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.PO_CASES)
def test_po_points_bitwise(orc, gpu_ctx_factory, monkeypatch, name):
    s, want = tc.setup(name), tc.oracle_po(orc, name)
    if s["path"] == _abi.POINTS_PATH_INTERPRETER and s["lens_mode"] is None:
        # A table that is not compiled in: set_lens would hand it to a compiling thread (csrc/lentil_lens_jit.h) whose kernels
        # this call never runs -- a minute of CPUs for nothing, and a process that ends meanwhile ends with hiprtc still at work
        # in that thread.  (Read when the context is created.)
        monkeypatch.setenv("LENTIL_LENS_JIT", "0")
    ctx = _po_ctx(gpu_ctx_factory, s)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_THIN_LENS                   # no call yet
    got = _trace(ctx, s)
    print(name, tc.classes(want))
    assert ctx.trace_points_path() == s["path"]
    _check_po(got, want, s["p"])


def test_compiled_in_and_interpreter_agree(orc, gpu_ctx_factory):
    """one context, the lens mode switched between two calls: the same bits, paths 2 and 1"""
    s = tc.setup("po-flat")
    ctx = _po_ctx(gpu_ctx_factory, s)
    a = _trace(ctx, s)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_COMPILED_IN
    ctx.set_lens_mode(1)
    b = _trace(ctx, s)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_INTERPRETER
    for key in ("pixel", "xy", "sensor", "tries"):
        assert _same_bits(a[key], b[key]), key
    _check_po(b, tc.oracle_po(orc, "po-flat"), s["p"])


# ---- 2. agreement with the pass -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.PASS_CASES))
def test_points_agree_with_the_pass(orc, gpu_ctx_factory, name):
    """every attempt 0 ... the last logged one of every visit in the oracle's draw log: (visit, m) is in the log <=> the
    query lands in the frame, on the logged pixel; every other attempt in that range is one of the two codes"""
    r = tc.pass_case(orc, name)
    p = r["p"]
    ctx = gpu_ctx_factory()
    ctx.set_params(p)
    if r["table"] is not None:
        ctx.set_lens(r["table"])
    got = ctx.trace_points(r["cs"], r["pixel"], r["k"], want_tries=True)
    assert ctx.trace_points_path() == (_abi.POINTS_PATH_COMPILED_IN if r["table"] is not None else _abi.POINTS_PATH_THIN_LENS)
    upto = np.arange(r["k"])[None, :] <= r["last"][:, None]
    logged = upto & (r["landed"] != tc.VIGNETTED)
    inside = got["pixel"] < tc.OUTSIDE
    print(name, tc.pass_counts(r), "codes in range:", int((upto & (got["pixel"] == tc.VIGNETTED)).sum()), "vignetted,",
          int((upto & (got["pixel"] == tc.OUTSIDE)).sum()), "outside")
    assert np.array_equal(inside & upto, logged)
    assert np.array_equal(got["pixel"][logged], r["landed"][logged])
    assert np.isin(got["pixel"][upto & ~logged], (tc.VIGNETTED, tc.OUTSIDE)).all()
    # the coordinates go with the codes: NaNs where vignetted, the pixel's own where inside, beyond the frame where outside
    xy, pix = got["xy"], got["pixel"]
    assert _quiet_nans(xy[pix == tc.VIGNETTED])
    fl = np.floor(xy[inside]).astype(np.int64)
    assert np.array_equal(fl[:, 0] + fl[:, 1] * int(p.xres), pix[inside].astype(np.int64))
    out = xy[pix == tc.OUTSIDE]
    if name == "pass-tl-plain":                 # (nothing vignettes a plain thin lens: every absent attempt fell outside)
        assert out.shape[0] > 0 and not (upto & (pix == tc.VIGNETTED)).any()
    assert (np.isnan(out).any(1) | (out[:, 0] < 0) | (out[:, 0] >= p.xres) | (out[:, 1] < 0) | (out[:, 1] >= p.yres)).all()
    if r["table"] is None:
        assert not got["tries"].any()                                              # the thin lens makes one try per attempt
        assert _same_bits(xy[inside], xy[inside].astype(np.float32).astype(np.float64))   # fp32 values widened


# ---- 3. forms of the call -----------------------------------------------------------------------------------------------------
def test_forms_of_the_call(orc, gpu_ctx_factory):
    import torch
    s, want = tc.setup("po-slabs-k130"), tc.oracle_po(orc, "po-slabs-k130")
    ctx = _po_ctx(gpu_ctx_factory, s)
    whole = _trace(ctx, s)
    _check_po(whole, want, s["p"])
    n, k = s["cs"].shape[0], s["k"]
    keys = ("pixel", "xy", "sensor", "tries")

    # device pointers: torch tensors in and out, nothing waited for by the call
    t_cs = torch.from_numpy(s["cs"].copy()).cuda()
    t_px = torch.from_numpy(s["pixel"].view(np.int32).copy()).cuda()
    t_fa = torch.from_numpy(s["first"].view(np.int32).copy()).cuda()
    dev = ctx.trace_points(t_cs, t_px, k, first_attempt=t_fa, lam=s["lam"], want_sensor=True, want_tries=True)
    assert all(dev[key].is_cuda for key in keys) and tuple(dev["xy"].shape) == (n, k, 2)
    ctx.sync()
    assert np.array_equal(dev["pixel"].cpu().numpy().view(np.uint32), whole["pixel"])
    for key in keys[1:]:
        assert _same_bits(dev[key].cpu().numpy(), whole[key]), key
    with pytest.raises(ValueError):
        ctx.trace_points(torch.from_numpy(s["cs"].copy()), t_px, k)                # not on the context's GPU
    with pytest.raises(ValueError):
        ctx.trace_points(torch.empty((3, n), dtype=torch.float32, device="cuda").t(), t_px, k)     # not contiguous

    # split by points
    h = n // 3
    parts = [ctx.trace_points(s["cs"][a:b], s["pixel"][a:b], k, first_attempt=s["first"][a:b], lam=s["lam"], want_sensor=True, want_tries=True)
             for a, b in ((0, h), (h, n))]
    for key in keys:
        assert _same_bits(np.concatenate([q[key] for q in parts], 0), whole[key]), key

    # split by attempts: the second call starts K / 2 attempts later
    half = k // 2
    first2 = (s["first"] + np.uint32(half)).astype(np.uint32)
    parts = [ctx.trace_points(s["cs"], s["pixel"], half, first_attempt=s["first"], lam=s["lam"], want_sensor=True, want_tries=True),
             ctx.trace_points(s["cs"], s["pixel"], k - half, first_attempt=first2, lam=s["lam"], want_sensor=True, want_tries=True)]
    for key in keys:
        assert _same_bits(np.concatenate([q[key] for q in parts], 1), whole[key]), key

    # optional outputs left out change nothing in out_pixel
    bare = ctx.trace_points(s["cs"], s["pixel"], k, first_attempt=s["first"], lam=s["lam"], want_xy=False)
    assert sorted(bare) == ["pixel"] and np.array_equal(bare["pixel"], whole["pixel"])
    only_tries = ctx.trace_points(s["cs"], s["pixel"], k, first_attempt=s["first"], lam=s["lam"], want_xy=False, want_tries=True)
    assert np.array_equal(only_tries["pixel"], whole["pixel"]) and np.array_equal(only_tries["tries"], whole["tries"])


def test_no_points_launch_nothing(gpu_ctx_factory):
    s = tc.setup("po-slabs-k65")
    ctx = _po_ctx(gpu_ctx_factory, s)
    got = ctx.trace_points(s["cs"][:0], s["pixel"][:0], 65, want_sensor=True, want_tries=True)
    assert got["pixel"].shape == (0, 65) and got["xy"].shape == (0, 65, 2) and got["tries"].shape == (0, 65)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_THIN_LENS                   # still "no call yet": nothing ran
    batch = _abi.PointBatch()                                                      # ... whatever the pointers are
    batch.n_points, batch.attempts = 0, 3
    assert ctx.lib.lentil_hip_trace_points(ctx.h, C.byref(batch)) == _abi.OK


# ---- 4. invalid calls -----------------------------------------------------------------------------------------------------------
def test_invalid_calls(orc, gpu_ctx_factory):
    s, want = tc.setup("po-slabs-k63"), tc.oracle_po(orc, "po-slabs-k63")
    cs, pixel, first, k = s["cs"], s["pixel"], s["first"], s["k"]
    ctx = gpu_ctx_factory()

    def code(fn):
        with pytest.raises(capi.LentilError) as e:
            fn()
        return e.value.code

    assert code(lambda: ctx.trace_points(cs, pixel, k)) == _abi.ERR_INVALID                       # no parameters
    ctx.set_params(s["p"])
    assert code(lambda: ctx.trace_points(cs, pixel, k)) == _abi.ERR_INVALID                       # polynomial optics, no lens
    ctx.set_lens(s["table"])
    assert ctx.lib.lentil_hip_trace_points(ctx.h, None) == _abi.ERR_INVALID
    assert code(lambda: ctx.trace_points(cs, pixel, 0)) == _abi.ERR_INVALID                       # attempts == 0
    out = np.zeros((4, 2), np.uint32)

    def raw(n_points, attempts, a, b, c, fa=None):
        batch = _abi.PointBatch()
        batch.n_points, batch.attempts, batch.cs, batch.pixel, batch.out_pixel, batch.first_attempt = n_points, attempts, a, b, c, fa
        return ctx.lib.lentil_hip_trace_points(ctx.h, C.byref(batch))

    ptrs = (cs.ctypes.data, pixel.ctypes.data, out.ctypes.data)
    assert raw(4, 2, *ptrs) == _abi.OK
    for missing in range(3):                                                                       # cs / pixel / out_pixel NULL
        assert raw(4, 2, *[None if i == missing else q for i, q in enumerate(ptrs)]) == _abi.ERR_INVALID
    assert raw(1 << 20, 1 << 12, *ptrs) == _abi.ERR_INVALID                                        # n_points * attempts == 2^32
    assert raw(1 << 33, 1, *ptrs) == _abi.ERR_INVALID
    # the seeds of a point's tries must fit 32 bits: first_attempt + attempts + max(vignetting_retries, 0)
    retries = int(s["p"].vignetting_retries)
    assert retries == 15
    fa = np.zeros(4, np.uint32)
    fa[2] = 0xFFFFFFFF - 2 - retries + 1
    assert raw(4, 2, *ptrs, fa=fa.ctypes.data) == _abi.ERR_INVALID
    fa[2] -= 1
    assert raw(4, 2, *ptrs, fa=fa.ctypes.data) == _abi.OK
    assert code(lambda: ctx.trace_points(cs, pixel, k, first_attempt=np.full(cs.shape[0], 0xFFFFFFF0, np.uint32))) == _abi.ERR_INVALID
    pi, model, table_i, keep_i = common.po_setup(96, 64, bokeh_enable_image=1)
    ctx.set_params(pi)
    assert code(lambda: ctx.trace_points(cs, pixel, k)) == _abi.ERR_INVALID                       # bokeh_enable_image, no tables
    # the context stays usable
    ctx.set_params(s["p"])
    _check_po(_trace(ctx, s), want, s["p"])
    # a thin lens needs no lens table
    tl = gpu_ctx_factory()
    tl.set_params(common.tl_setup(96, 64))
    assert tl.trace_points(cs, pixel, 2)["pixel"].shape == (cs.shape[0], 2)
    assert tl.trace_points_path() == _abi.POINTS_PATH_THIN_LENS


# ---- 5. no interference with a pass -------------------------------------------------------------------------------------------------
def test_points_between_two_passes(orc, gpu_ctx_factory):
    """a batch between two passes of a context: the second pass's draw log is the one of a context that never made the call,
    entry for entry, and so is its frame -- at the 1e-5 bar every comparison of draws' sums is made at (the draws are added
    with atomics, in an order no two runs share)"""
    s, want = tc.setup("po-slabs-k65"), tc.oracle_po(orc, "po-slabs-k65")
    W, H, M = 96, 64, 9
    p, model, table, keep = common.po_setup(W, H, samples_override=16)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)

    def context():
        ctx = gpu_ctx_factory()
        ctx.set_params(p)
        ctx.set_lens(table)
        ctx.alloc_frame(1)
        ctx.set_draw_log(1 << 20)
        ctx.upload_visits(visits)
        return ctx

    def frame(ctx):
        ctx.clear_frame()
        ctx.redistribute()
        ctx.resolve()

    a, b = context(), context()
    frame(a)
    got = a.trace_points(s["cs"], s["pixel"], s["k"], first_attempt=s["first"], want_sensor=True, want_tries=True)
    frame(a)
    frame(b)
    frame(b)
    log_a, log_b = common.sort_log(a.draw_log()), common.sort_log(b.draw_log())
    assert log_a.shape[0] > 0 and np.array_equal(log_a, log_b)
    (buf_a, w_a), (buf_b, w_b) = a.download_accum(0), b.download_accum(0)
    assert np.array_equal(buf_a != 0, buf_b != 0) and np.array_equal(w_a != 0, w_b != 0)
    assert common.rel_err(buf_a[buf_b != 0], buf_b[buf_b != 0]) < 1e-5 and common.rel_err(w_a[w_b != 0], w_b[w_b != 0]) < 1e-5
    ca, cb = a.counters(), b.counters()
    assert (ca.attempted_draws, ca.accepted_draws, ca.redistributed_visits) == (cb.attempted_draws, cb.accepted_draws, cb.redistributed_visits)
    _check_po(got, want, s["p"])                 # (the frame's parameters are the case's but for samples_override, which no query reads)
