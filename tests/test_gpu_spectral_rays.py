"""Camera rays with a wavelength per ray on the GPU (lentil_hip_camera_rays_spectral, camera_rays_spectral_kernel of
csrc/lentil_camera_rays.h) against the oracle and against the scalar call, word for word: every comparison is of bit
patterns, there is no tolerance anywhere.  tests/spectral_cases.py has the cases, tests/test_spectral_cases.py holds them
to rays whose results and retries depend on the wavelength.
"""
import ctypes as C

import numpy as np
import pytest

import common
import lens_tables as lt
import spectral_cases as sc
from pota_amd import _abi, capi
from test_gpu_camera_rays import _inputs, _same_bits, oracle_rays

pytestmark = pytest.mark.gpu

SEED = sc.SEED
DG = "double_gauss_50mm/disk"


def _ctx(make, s, tables=None):
    ctx = make()
    ctx.set_params(s["p"])
    ctx.set_lens(s["table"])
    if tables is not None:
        ctx.set_bokeh(tables)
    return ctx


def _assert_rays(got, got_tries, want, want_tries):
    assert np.array_equal(got_tries, want_tries)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:2]], want[bad[:2]])


# ---- (a) against the oracle, per ray with that ray's wavelength ---------------------------------------------------------------
@pytest.mark.parametrize("name", sc.RAY_CASES)
def test_spectral_rays_bitwise(orc, gpu_ctx_factory, name):
    s = sc.ray_setup(name)
    want, want_tries = sc.oracle_ray_case(orc, name)
    ctx = _ctx(gpu_ctx_factory, s, sc.ray_tables(orc, name))
    got, got_tries = ctx.camera_rays(s["inp"], seed=SEED, want_tries=True, lambdas=s["lambdas"], lam=123.0)      # (lam is ignored)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER
    _assert_rays(got, got_tries, want, want_tries)


# ---- (b) all wavelengths equal: the scalar call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("differentials", [True, False])
def test_equal_wavelengths_are_the_scalar_call(gpu_ctx_factory, differentials):
    s = sc.ray_setup(DG)
    ctx = _ctx(gpu_ctx_factory, s)
    n = s["inp"].shape[0]
    for lam in (sc.LAM_BLUE, 0.5712345678901234):
        want, want_tries = ctx.camera_rays(s["inp"], lam=lam, seed=SEED, differentials=differentials, want_tries=True)
        got, got_tries = ctx.camera_rays(s["inp"], seed=SEED, differentials=differentials, want_tries=True, lambdas=np.full(n, lam))
        assert int((want_tries > 0).sum()) > 0
        _assert_rays(got, got_tries, want, want_tries)
        if not differentials:
            assert not got[:, 9:].view(np.uint32).any()


# ---- (c) two wavelengths interleaved lane by lane ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_even_and_odd_lanes_at_two_wavelengths(gpu_ctx_factory, n):
    s = sc.ray_setup(DG)
    ctx = _ctx(gpu_ctx_factory, s)
    inp = s["inp"][:n]
    blue, blue_tries = ctx.camera_rays(inp, lam=sc.LAM_BLUE, seed=SEED, want_tries=True)
    red, red_tries = ctx.camera_rays(inp, lam=sc.LAM_RED, seed=SEED, want_tries=True)
    odd = (np.arange(n) & 1) == 1
    want, want_tries = np.where(odd[:, None], red, blue), np.where(odd, red_tries, blue_tries)
    got, got_tries = ctx.camera_rays(inp, seed=SEED, want_tries=True, lambdas=np.where(odd, sc.LAM_RED, sc.LAM_BLUE))
    assert got.shape == (n, 21)
    _assert_rays(got, got_tries, want, want_tries)
    if n > 1:
        assert not _same_bits(got, blue) and not _same_bits(got, red)


# ---- (d) split-invariance ----------------------------------------------------------------------------------------------------------
def test_a_spectral_batch_does_not_depend_on_how_it_is_split(orc, gpu_ctx_factory):
    s = sc.ray_setup(DG)
    want, want_tries = sc.oracle_ray_case(orc, DG)
    ctx = _ctx(gpu_ctx_factory, s)
    n, cut = s["inp"].shape[0], 333
    parts = [ctx.camera_rays(s["inp"][a:b], first_ray=a, seed=SEED, want_tries=True, lambdas=s["lambdas"][a:b]) for a, b in ((0, cut), (cut, n))]
    _assert_rays(np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts]), want, want_tries)


# ---- (e) wavelength exponents up to 15 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lambda-powers", "all-fifteen"])
def test_generated_tables(orc, gpu_ctx_factory, monkeypatch, name):
    """no shipped term reads beyond lambda_pow[2]: only these tables show a wrong higher power"""
    monkeypatch.setenv("LENTIL_LENS_JIT", "0")          # (read when the context is created; see tests/test_gpu_lens_tables.py)
    p, model, table, keep = lt.setup(name)
    n = 515
    inp, lambdas = _inputs(n, 9, 1.1, 0.7), sc.ray_lambdas(n, seed=23)
    lens = orc.orc_lens_create(C.byref(table))
    want, want_tries = np.zeros((n, 21), np.float32), np.zeros(n, np.int32)
    try:
        for i in range(n):
            o, t = oracle_rays(orc, p, lens, None, inp[i:i + 1], first_ray=i, lam=float(lambdas[i]), seed=SEED)
            want[i], want_tries[i] = o[0], t[0]
    finally:
        orc.orc_lens_destroy(lens)
    assert int((want[:, 6] != 0).sum()) > n // 4
    ctx = gpu_ctx_factory()
    ctx.set_params(p)
    ctx.set_lens(table)
    got, got_tries = ctx.camera_rays(inp, seed=SEED, want_tries=True, lambdas=lambdas)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER
    _assert_rays(got, got_tries, want, want_tries)


# ---- (f) paths -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ["double_gauss_50mm", "petzval_58mm"])
def test_paths(orc, gpu_ctx_factory, monkeypatch, lens):
    name = lens + "/disk"
    s = sc.ray_setup(name)
    want, want_tries = sc.oracle_ray_case(orc, name)
    kw = dict(seed=SEED, want_tries=True, lambdas=s["lambdas"])
    monkeypatch.delenv("LENTIL_RAYS_COMPILED", raising=False)
    ctx = _ctx(gpu_ctx_factory, s)
    a = ctx.camera_rays(s["inp"], **kw)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER                    # the default
    monkeypatch.setenv("LENTIL_RAYS_COMPILED", "1")
    ctx = _ctx(gpu_ctx_factory, s)
    b = ctx.camera_rays(s["inp"], **kw)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    ctx.set_lens_mode(1)
    c = ctx.camera_rays(s["inp"], **kw)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER
    for got in (a, b, c):
        _assert_rays(got[0], got[1], want, want_tries)


# ---- (g) device pointers ---------------------------------------------------------------------------------------------------------------
def test_device_pointers(orc, gpu_ctx_factory):
    import torch
    s = sc.ray_setup(DG)
    want, want_tries = sc.oracle_ray_case(orc, DG)
    ctx = _ctx(gpu_ctx_factory, s)
    t_in, t_lam = torch.from_numpy(s["inp"].copy()).cuda(), torch.from_numpy(s["lambdas"].copy()).cuda()
    t_out, t_tries = ctx.camera_rays(t_in, seed=SEED, want_tries=True, lambdas=t_lam)
    assert t_out.is_cuda and tuple(t_out.shape) == (s["inp"].shape[0], 21)
    ctx.sync()
    _assert_rays(t_out.cpu().numpy(), t_tries.cpu().numpy(), want, want_tries)
    for bad in (s["lambdas"], t_lam.cpu(), t_lam.float(), t_lam[:-1], torch.stack([t_lam, t_lam], 1)[:, 0]):
        with pytest.raises(ValueError, match="lambdas"):      # numpy beside tensors, not on the GPU, fp32, too short, strided
            ctx.camera_rays(t_in, seed=SEED, lambdas=bad)
    with pytest.raises(ValueError, match="lambdas"):
        ctx.camera_rays(s["inp"], seed=SEED, lambdas=t_lam)  # a tensor beside numpy


# ---- (h) thin lens ------------------------------------------------------------------------------------------------------------------------
def test_thin_lens_ignores_the_wavelengths(gpu_ctx_factory):
    p = common.tl_setup(sc.W, sc.H, optical_vignetting_distance=2.0)
    ctx = gpu_ctx_factory()
    ctx.set_params(p)
    n = 600
    inp = _inputs(n, 10, 1.0, 0.6)
    want, want_tries = ctx.camera_rays(inp, seed=77, exposure=0.5, want_tries=True)
    assert int((want_tries > 0).sum()) > 0
    got, got_tries = ctx.camera_rays(inp, seed=77, exposure=0.5, want_tries=True, lambdas=sc.ray_lambdas(n))
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_THIN_LENS
    _assert_rays(got, got_tries, want, want_tries)
    out, tries = np.zeros((n, 21), np.float32), np.zeros(n, np.int32)        # lambdas NULL
    b = _abi.CameraRayBatch()
    b.n, b.inp, b.out, b.tries, b.exposure, b.rng_seed = n, inp.ctypes.data, out.ctypes.data, tries.ctypes.data, 0.5, 77
    assert ctx.lib.lentil_hip_camera_rays_spectral(ctx.h, C.byref(b), None) == _abi.OK
    _assert_rays(out, tries, want, want_tries)


# ---- (i) refusals ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_calls(orc, gpu_ctx_factory):
    s = sc.ray_setup(DG)
    want, want_tries = sc.oracle_ray_case(orc, DG)
    inp, lam = s["inp"][:4], s["lambdas"][:4]
    ctx = gpu_ctx_factory()

    def code(fn):
        with pytest.raises(capi.LentilError) as e:
            fn()
        return e.value.code

    assert code(lambda: ctx.camera_rays(inp, lambdas=lam)) == _abi.ERR_INVALID                    # no parameters
    ctx.set_params(s["p"])
    assert code(lambda: ctx.camera_rays(inp, lambdas=lam)) == _abi.ERR_INVALID                    # polynomial optics, no lens
    ctx.set_lens(s["table"])
    assert ctx.camera_rays(inp[:0], lambdas=lam[:0]).shape == (0, 21)                             # n == 0: nothing launched
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_THIN_LENS                                     # ("no call yet")
    assert code(lambda: ctx.camera_rays(inp, first_ray=(1 << 32) - 3, lambdas=lam)) == _abi.ERR_INVALID
    out = np.zeros((4, 21), np.float32)

    def raw(n, a, b, lambdas):
        batch = _abi.CameraRayBatch()
        batch.n, batch.inp, batch.out, batch.exposure, batch.rng_seed = n, a, b, 1.0, SEED
        return ctx.lib.lentil_hip_camera_rays_spectral(ctx.h, C.byref(batch), lambdas)

    assert raw(4, inp.ctypes.data, out.ctypes.data, None) == _abi.ERR_INVALID                     # lambdas NULL, polynomial optics
    assert raw(4, None, out.ctypes.data, lam.ctypes.data) == _abi.ERR_INVALID
    assert raw(4, inp.ctypes.data, None, lam.ctypes.data) == _abi.ERR_INVALID
    assert raw(0, None, None, None) == _abi.OK                                                    # n == 0, whatever the pointers
    assert ctx.lib.lentil_hip_camera_rays_spectral(ctx.h, None, lam.ctypes.data) == _abi.ERR_INVALID
    assert raw(4, inp.ctypes.data, out.ctypes.data, lam.ctypes.data) == _abi.OK
    assert _same_bits(out, want[:4])
    pi, model, table_i, keep_i = common.po_setup(sc.W, sc.H, bokeh_enable_image=1)
    ctx.set_params(pi)
    assert code(lambda: ctx.camera_rays(inp, lambdas=lam)) == _abi.ERR_INVALID                    # bokeh_enable_image, no tables
    # the context still serves a scalar call
    ctx.set_params(s["p"])
    scalar = ctx.camera_rays(s["inp"][:1], lam=float(s["lambdas"][0]), seed=SEED)
    assert _same_bits(scalar, want[:1])


# ---- (j) between two streamed passes -----------------------------------------------------------------------------------------------------
def test_spectral_rays_between_two_streamed_passes(orc, gpu_ctx_factory):
    """tests/test_gpu_camera_rays.py::test_rays_between_two_streamed_passes with the spectral call in between: the next pass
    still streams and its frame is the one it is without the batch -- the draw log entry for entry, the sums at the 1e-5 bar
    every comparison of draws' sums is made at (they are added with atomics, in an order no two runs share); no stall is
    counted"""
    s = sc.ray_setup(DG)
    want, want_tries = sc.oracle_ray_case(orc, DG)
    M, S = 9, 128
    p, model, table, keep = common.po_setup(sc.W, sc.H, samples_override=S)
    visits, cols = common.make_stream(p, sc.W, sc.H, M, f_hi=2.0 ** -12)
    ctx = gpu_ctx_factory()
    ctx.set_params(p)
    ctx.set_lens(table)
    ctx.alloc_frame(1)
    ctx.set_draw_log(1 << 22)
    ctx.upload_visits(visits)

    def frame():
        ctx.clear_frame()
        ctx.redistribute()
        ctx.resolve()

    before = capi.process_stats()
    for _ in range(3):                       # the context's first passes size its buffers (not streamed, then streamed)
        frame()
    assert int(ctx.counters().streamed) == 1
    buf0, w0 = ctx.download_accum(0)
    log0 = common.sort_log(ctx.draw_log())
    frame()
    rays = ctx.camera_rays(s["inp"], seed=SEED, lambdas=s["lambdas"])           # lands behind the pass in flight
    frame()
    assert int(ctx.counters().streamed) == 1
    buf1, w1 = ctx.download_accum(0)
    assert np.array_equal(common.sort_log(ctx.draw_log()), log0)
    assert common.rel_err(buf1[buf0 != 0], buf0[buf0 != 0]) < 1e-5 and common.rel_err(w1[w0 != 0], w0[w0 != 0]) < 1e-5
    assert np.array_equal(buf1 != 0, buf0 != 0)
    assert _same_bits(rays, want)
    after = capi.process_stats()
    assert after[1] - before[1] == 0, capi.process_stall_notes()
