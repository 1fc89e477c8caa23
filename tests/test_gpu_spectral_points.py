"""Scene points traced backward with a wavelength per point on the GPU (lentil_hip_trace_points_spectral,
trace_points_spectral_kernel of csrc/lentil_trace_points.h) against the oracle and against the scalar call, bit for bit:
there is no tolerance anywhere.  tests/spectral_cases.py has the cases, tests/test_spectral_cases.py holds them to queries
whose results and retries depend on the wavelength.
"""
import ctypes as C

import numpy as np
import pytest

import common
import lens_tables as lt
import spectral_cases as sc
import trace_point_cases as tc
from pota_amd import _abi, capi
from test_gpu_trace_points import _check_po, _same_bits

pytestmark = pytest.mark.gpu

KEYS = ("pixel", "xy", "sensor", "tries")


def _ctx(make, s):
    ctx = make()
    ctx.set_params(s["p"])
    ctx.set_lens(s["table"])
    if s.get("lens_mode") is not None:
        ctx.set_lens_mode(s["lens_mode"])
    return ctx


def _trace(ctx, s, **kw):
    kw.setdefault("lambdas", s["lambdas"])
    return ctx.trace_points(s["cs"], s["pixel"], s["k"], first_attempt=s["first"], want_sensor=True, want_tries=True, **kw)


def _assert_same(a, b):
    for key in KEYS:
        assert _same_bits(a[key], b[key]), key


# ---- (a) against the oracle, per query with the point's wavelength -------------------------------------------------------------
@pytest.mark.parametrize("name", sc.POINT_CASES)
def test_spectral_points_bitwise(orc, gpu_ctx_factory, name):
    s, want = sc.point_setup(orc, name), sc.oracle_point_case(orc, name)
    ctx = _ctx(gpu_ctx_factory, s)
    got = _trace(ctx, s, lam=123.0)                                                # (lam is ignored)
    assert ctx.trace_points_path() == s["path"]
    _check_po(got, want, s["p"])


# ---- (b) equal wavelengths: the scalar call; 0: lambda_bw ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dg/k65", "dg-interpreter/k65"])
def test_equal_wavelengths_are_the_scalar_call(orc, gpu_ctx_factory, name):
    s = sc.point_setup(orc, name)
    ctx = _ctx(gpu_ctx_factory, s)
    n = s["cs"].shape[0]
    for lam in (sc.LAM_RED, 0.5712345678901234):
        _assert_same(_trace(ctx, s, lambdas=np.full(n, lam)), _trace(ctx, s, lambdas=None, lam=lam))
    by_default = _trace(ctx, s, lambdas=None, lam=0.0)                              # params.lambda_bw
    _assert_same(_trace(ctx, s, lambdas=np.zeros(n)), by_default)
    _assert_same(_trace(ctx, s, lambdas=np.full(n, float(s["p"].lambda_bw))), by_default)
    # ... entry by entry: zeros among other wavelengths
    mixed = s["lambdas"].copy()
    mixed[::2] = 0.0
    full = np.where(mixed == 0.0, float(s["p"].lambda_bw), mixed)
    _assert_same(_trace(ctx, s, lambdas=mixed), _trace(ctx, s, lambdas=full))
    _check_po(_trace(ctx, s, lambdas=mixed), sc.trace_queries(orc, s["p"], s["table"], s["cs"], s["px"], s["py"], s["first"], s["k"], mixed), s["p"])


# ---- (c) more slabs than the grid has waves: a wave restages for another point --------------------------------------------------
def _grid_waves():
    """the waves of the largest grid lentil_hip_trace_points launches: eight blocks of four waves per compute unit"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4


@pytest.mark.parametrize("shape", ["5000x1", "700x65", "two-grids-x1"])
@pytest.mark.parametrize("lens_mode", [None, 1])
def test_a_palette_of_three_across_many_slabs(orc, gpu_ctx_factory, shape, lens_mode):
    """wavelengths from a palette of three in an order that changes from point to point, against three scalar calls over the
    same points and, on every 50th point, the oracle.  "two-grids-x1" has more than twice as many slabs as the grid has
    waves, whatever the device: every wave walks on to at least two other points."""
    n, k = (2 * _grid_waves() + 777, 1) if shape == "two-grids-x1" else tuple(int(v) for v in shape.split("x"))
    p, model, table, keep = common.po_setup(*sc.FRAME)
    cs, px, py, first = sc.draw_points(p, n, 31)
    pixel = tc.pack_pixel(px, py)
    which = np.random.default_rng(32).integers(0, 3, n)
    which[:6] = (0, 1, 2, 2, 0, 1)
    lambdas = np.asarray(sc.LAM_PALETTE)[which]
    assert (which[1:] != which[:-1]).mean() > 0.5
    ctx = _ctx(gpu_ctx_factory, dict(p=p, table=table, lens_mode=lens_mode))
    kw = dict(first_attempt=first, want_sensor=True, want_tries=True)
    got = ctx.trace_points(cs, pixel, k, lambdas=lambdas, **kw)
    assert ctx.trace_points_path() == (_abi.POINTS_PATH_COMPILED_IN if lens_mode is None else _abi.POINTS_PATH_INTERPRETER)
    scalar = [ctx.trace_points(cs, pixel, k, lam=lam, **kw) for lam in sc.LAM_PALETTE]
    assert not _same_bits(scalar[0]["sensor"], scalar[2]["sensor"])
    for key in KEYS:
        sel = which.reshape((n, 1) + (1,) * (scalar[0][key].ndim - 2))
        want = np.choose(sel, [q[key] for q in scalar])
        assert _same_bits(got[key], want), key
    if lens_mode is None:
        step = slice(0, n, 50)
        want = sc.trace_queries(orc, p, table, cs[step], px[step], py[step], first[step], k, lambdas[step])
        _check_po({key: got[key][step] for key in KEYS}, want, p)


# ---- (d) wavelength exponents up to 15 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lambda-powers", "all-fifteen"])
def test_generated_tables(orc, gpu_ctx_factory, monkeypatch, name):
    """no shipped term reads beyond lambda_pow[2]: only these tables show a wrong higher power"""
    monkeypatch.setenv("LENTIL_LENS_JIT", "0")          # (read when the context is created; see tests/test_gpu_lens_tables.py)
    p, model, table, keep = lt.setup(name)
    n, k = 256, 4
    cs, px, py, first = sc.draw_points(p, n, 0x7A1, frame=(lt.W, lt.H))
    lambdas = sc.float32_lambdas(n, 41)
    want = sc.trace_queries(orc, p, table, cs, px, py, first, k, lambdas)
    assert int((want["pixel"] < tc.OUTSIDE).sum()) > n
    ctx = _ctx(gpu_ctx_factory, dict(p=p, table=table))
    got = ctx.trace_points(cs, tc.pack_pixel(px, py), k, first_attempt=first, want_sensor=True, want_tries=True, lambdas=lambdas)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_INTERPRETER
    _check_po(got, want, p)


# ---- (e) paths -----------------------------------------------------------------------------------------------------------------------------
def test_compiled_in_and_interpreter_agree(orc, gpu_ctx_factory):
    """one context, the lens mode switched between two calls: the same bits, paths 2 and 1"""
    s, want = sc.point_setup(orc, "petzval/k130"), sc.oracle_point_case(orc, "petzval/k130")
    ctx = _ctx(gpu_ctx_factory, s)
    a = _trace(ctx, s)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_COMPILED_IN
    ctx.set_lens_mode(1)
    b = _trace(ctx, s)
    assert ctx.trace_points_path() == _abi.POINTS_PATH_INTERPRETER
    _assert_same(a, b)
    _check_po(b, want, s["p"])


# ---- (f) device pointers ---------------------------------------------------------------------------------------------------------------
def test_device_pointers(orc, gpu_ctx_factory):
    import torch
    s, want = sc.point_setup(orc, "dg/k130"), sc.oracle_point_case(orc, "dg/k130")
    ctx = _ctx(gpu_ctx_factory, s)
    n, k = s["cs"].shape[0], s["k"]
    t_cs = torch.from_numpy(s["cs"].copy()).cuda()
    t_px = torch.from_numpy(s["pixel"].view(np.int32).copy()).cuda()
    t_fa = torch.from_numpy(s["first"].view(np.int32).copy()).cuda()
    t_lam = torch.from_numpy(s["lambdas"].copy()).cuda()
    dev = ctx.trace_points(t_cs, t_px, k, first_attempt=t_fa, want_sensor=True, want_tries=True, lambdas=t_lam)
    assert all(dev[key].is_cuda for key in KEYS) and tuple(dev["xy"].shape) == (n, k, 2)
    ctx.sync()
    got = {key: dev[key].cpu().numpy() for key in KEYS}
    got["pixel"] = got["pixel"].view(np.uint32)
    _check_po(got, want, s["p"])
    for bad in (s["lambdas"], t_lam.cpu(), t_lam.float(), t_lam[:-1], torch.stack([t_lam, t_lam], 1)[:, 0]):
        with pytest.raises(ValueError, match="lambdas"):      # numpy beside tensors, not on the GPU, fp32, too short, strided
            ctx.trace_points(t_cs, t_px, k, first_attempt=t_fa, lambdas=bad)
    with pytest.raises(ValueError, match="lambdas"):
        ctx.trace_points(s["cs"], s["pixel"], k, lambdas=t_lam)      # a tensor beside numpy


# ---- (g) thin lens -------------------------------------------------------------------------------------------------------------------------
def test_thin_lens_ignores_the_wavelengths(orc, gpu_ctx_factory):
    s = sc.point_setup(orc, "dg/k65")
    cs, pixel, k = s["cs"], s["pixel"], s["k"]
    n = cs.shape[0]
    ctx = gpu_ctx_factory()
    ctx.set_params(common.tl_setup(*sc.FRAME))
    want = ctx.trace_points(cs, pixel, k, want_sensor=True, want_tries=True)
    assert int((want["pixel"] < tc.OUTSIDE).sum()) > 0
    got = ctx.trace_points(cs, pixel, k, want_sensor=True, want_tries=True, lambdas=s["lambdas"])
    assert ctx.trace_points_path() == _abi.POINTS_PATH_THIN_LENS
    _assert_same(got, want)
    out = np.zeros((n, k), np.uint32)                                              # lambdas NULL
    b = _abi.PointBatch()
    b.n_points, b.attempts, b.cs, b.pixel, b.out_pixel = n, k, cs.ctypes.data, pixel.ctypes.data, out.ctypes.data
    assert ctx.lib.lentil_hip_trace_points_spectral(ctx.h, C.byref(b), None) == _abi.OK
    assert np.array_equal(out, want["pixel"])


# ---- (h) refusals ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_calls(orc, gpu_ctx_factory):
    s, want = sc.point_setup(orc, "dg/k64"), sc.oracle_point_case(orc, "dg/k64")
    cs, pixel, k, lam = s["cs"], s["pixel"], s["k"], s["lambdas"]
    n = cs.shape[0]
    ctx = gpu_ctx_factory()

    def code(fn):
        with pytest.raises(capi.LentilError) as e:
            fn()
        return e.value.code

    assert code(lambda: ctx.trace_points(cs, pixel, k, lambdas=lam)) == _abi.ERR_INVALID         # no parameters
    ctx.set_params(s["p"])
    assert code(lambda: ctx.trace_points(cs, pixel, k, lambdas=lam)) == _abi.ERR_INVALID         # polynomial optics, no lens
    ctx.set_lens(s["table"])
    assert ctx.lib.lentil_hip_trace_points_spectral(ctx.h, None, lam.ctypes.data) == _abi.ERR_INVALID
    assert code(lambda: ctx.trace_points(cs, pixel, 0, lambdas=lam)) == _abi.ERR_INVALID         # attempts == 0
    assert ctx.trace_points(cs[:0], pixel[:0], k, lambdas=lam[:0])["pixel"].shape == (0, k)      # n_points == 0: nothing launched
    assert ctx.trace_points_path() == _abi.POINTS_PATH_THIN_LENS                                  # ("no call yet")
    out = np.zeros((n, 2), np.uint32)

    def raw(n_points, attempts, a, b, c, lambdas, fa=None):
        batch = _abi.PointBatch()
        batch.n_points, batch.attempts, batch.cs, batch.pixel, batch.out_pixel, batch.first_attempt = n_points, attempts, a, b, c, fa
        return ctx.lib.lentil_hip_trace_points_spectral(ctx.h, C.byref(batch), lambdas)

    ptrs = (cs.ctypes.data, pixel.ctypes.data, out.ctypes.data)
    assert raw(n, 2, *ptrs, lam.ctypes.data) == _abi.OK
    assert np.array_equal(out, want["pixel"][:, :2])
    assert raw(n, 2, *ptrs, None) == _abi.ERR_INVALID                                             # lambdas NULL, polynomial optics
    assert raw(0, 2, None, None, None, None) == _abi.OK                                           # n_points == 0, whatever the pointers
    for missing in range(3):                                                                      # cs / pixel / out_pixel NULL
        assert raw(n, 2, *[None if i == missing else q for i, q in enumerate(ptrs)], lam.ctypes.data) == _abi.ERR_INVALID
    assert raw(1 << 20, 1 << 12, *ptrs, lam.ctypes.data) == _abi.ERR_INVALID                      # n_points * attempts == 2^32
    fa = np.zeros(n, np.uint32)
    fa[2] = 0xFFFFFFFF - 2 - int(s["p"].vignetting_retries) + 1
    assert raw(n, 2, *ptrs, lam.ctypes.data, fa=fa.ctypes.data) == _abi.ERR_INVALID               # the seeds must fit 32 bits
    pi, model, table_i, keep_i = common.po_setup(*sc.FRAME, bokeh_enable_image=1)
    ctx.set_params(pi)
    assert code(lambda: ctx.trace_points(cs, pixel, k, lambdas=lam)) == _abi.ERR_INVALID         # bokeh_enable_image, no tables
    # the context still serves both calls
    ctx.set_params(s["p"])
    _check_po(_trace(ctx, s), want, s["p"])
    scalar = ctx.trace_points(cs[:1], pixel[:1], k, lam=float(lam[0]), want_sensor=True, want_tries=True)
    _check_po(scalar, {key: v[:1] for key, v in want.items()}, s["p"])
