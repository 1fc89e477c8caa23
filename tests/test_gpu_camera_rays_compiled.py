"""Forward camera rays through the lens's straight-line code (csrc/lentil_camera_rays.h, camera_rays_kernel<GenLens<..>>):
the compiled-in lenses (path 2), a lens compiled at run time (path 3) and the table interpreter they replace (path 1) give
the oracle's rays, word for word and try for try -- the comparison of tests/test_gpu_camera_rays.py::test_po_rays_bitwise,
whose helpers are used here.  The focus search's compiled-in instantiations keep the sequential loop's winner.
The compiled paths are taken by a context created under LENTIL_RAYS_COMPILED=1 (the library's default is the interpreter
until the two have been measured against each other): every test here runs under it unless it says otherwise.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import common
from pota_amd import _abi, capi, hostlib
from test_gpu_camera_rays import LAM, PO_SETUPS, _bokeh_tables, _ctx, _inputs, _same_bits, oracle_rays

pytestmark = pytest.mark.gpu

W, H = 640, 360
COMPILED = ["double_gauss_50mm", "petzval_58mm"]
N_IN, N_OUT = 4096 + 37 - 256, 256       # 4 133 rays: the last block is partial and one of its waves is partly past the end
SEED = 0x1234


@pytest.fixture(autouse=True)
def _rays_compiled(monkeypatch):
    monkeypatch.setenv("LENTIL_RAYS_COMPILED", "1")          # (read when a context is created)


def _batch():
    """uniform over the sensor, then N_OUT rays far outside the image circle (every try of theirs vignettes)"""
    inside = _inputs(N_IN, 31, 1.0, H / W)
    rng = np.random.default_rng(32)
    ang = rng.uniform(0.0, 2.0 * np.pi, N_OUT)
    rad = rng.uniform(2.5, 3.0, N_OUT)
    outside = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0.5, 2.0, N_OUT), rng.uniform(0.5, 2.0, N_OUT),
                        rng.random(N_OUT), rng.random(N_OUT)], 1).astype(np.float32)
    return np.concatenate([inside, outside])


def _check(got, got_tries, want, want_tries):
    assert np.array_equal(got_tries, want_tries)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.fixture(scope="module", params=COMPILED)
def ref(request, orc):
    """one batch per compiled-in lens and the oracle's rays for it, computed once"""
    p, model, table, keep = common.po_setup(W, H, lens=request.param)
    lens = orc.orc_lens_create(C.byref(table))
    inp = _batch()
    want, want_tries = oracle_rays(orc, p, lens, None, inp, seed=SEED)
    orc.orc_lens_destroy(lens)
    assert int((want_tries[:N_IN] > 0).sum()) > 0 and int((want[:N_IN, 6] != 0).sum()) > N_IN // 2
    assert (want_tries[N_IN:] == p.vignetting_retries + 1).all() and not want[N_IN:, 6].any()     # outside: every try vignetted
    return request.param, p, table, keep, inp, want, want_tries


# ---- a: the new path runs and matches the oracle ------------------------------------------------------------------------------
def test_compiled_in_lens_runs_its_own_kernel_and_matches_the_oracle(ref, gpu_ctx_factory):
    name, p, table, keep, inp, want, want_tries = ref
    ctx = _ctx(gpu_ctx_factory, p, table)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_THIN_LENS           # no call yet
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    _check(got, tries, want, want_tries)


# ---- b: the forced interpreter -----------------------------------------------------------------------------------------------
def test_lens_mode_1_forces_the_interpreter(ref, gpu_ctx_factory):
    name, p, table, keep, inp, want, want_tries = ref
    ctx = _ctx(gpu_ctx_factory, p, table)
    ctx.set_lens_mode(1)
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER
    _check(got, tries, want, want_tries)
    ctx.set_lens_mode(0)
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    _check(got, tries, want, want_tries)


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import common
from pota_amd import capi
name, src, dst = sys.argv[1:4]
p, model, table, keep = common.po_setup(%d, %d, lens=name)
ctx = capi.Context(0); ctx.set_params(p); ctx.set_lens(table)
got, tries = ctx.camera_rays(np.load(src), lam=%r, seed=%d, want_tries=True)
np.savez(dst, got=got, tries=tries, path=ctx.camera_rays_path())
ctx.close()
"""


def test_rays_compiled_0_in_the_environment_forces_the_interpreter(ref, tmp_path):
    name, p, table, keep, inp, want, want_tries = ref
    src, dst = str(tmp_path / "in.npy"), str(tmp_path / "out.npz")
    np.save(src, inp)
    code = CHILD % (common.ROOT, os.path.join(common.ROOT, "tests"), W, H, LAM, SEED)
    env = dict(os.environ, LENTIL_RAYS_COMPILED="0")
    subprocess.run([sys.executable, "-c", code, name, src, dst], env=env, check=True, timeout=300)
    res = np.load(dst)
    assert int(res["path"]) == _abi.RAYS_PATH_INTERPRETER
    _check(res["got"], res["tries"], want, want_tries)


def test_without_the_switch_the_interpreter_runs(ref, gpu_ctx_factory, monkeypatch):
    name, p, table, keep, inp, want, want_tries = ref
    monkeypatch.delenv("LENTIL_RAYS_COMPILED")
    ctx = _ctx(gpu_ctx_factory, p, table)
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER
    _check(got, tries, want, want_tries)


# ---- c: setups ---------------------------------------------------------------------------------------------------------------
# blades 0 and 5, a bokeh image, enable_dof = 0, retries 0; "disk" is the camera's defaults: cm units, 15 retries
@pytest.mark.parametrize("setup", ["disk", "blades5", "image", "no_dof", "retries0"])
@pytest.mark.parametrize("lens_name", COMPILED)
def test_setups(orc, gpu_ctx_factory, lens_name, setup):
    kw = PO_SETUPS[setup]
    p, model, table, keep = common.po_setup(W, H, lens=lens_name, **kw)
    if setup == "disk":
        assert p.unitModel == _abi.UNIT_CM and p.vignetting_retries == 15 and p.bokeh_aperture_blades == 0
    tables, ob = _bokeh_tables(orc) if kw.get("bokeh_enable_image") else (None, None)
    lens = orc.orc_lens_create(C.byref(table))
    try:
        inp = _inputs(1024, 9, 1.1, 0.7)
        want, want_tries = oracle_rays(orc, p, lens, ob, inp, seed=SEED)
        if p.enable_dof:
            assert int((want_tries > 0).sum()) > 0, "no ray of this case retries"
        ctx = _ctx(gpu_ctx_factory, p, table, tables)
        got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
        assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    finally:
        orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    _check(got, tries, want, want_tries)


# ---- d: small batches, no differentials, splitting -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_batches(ref, gpu_ctx_factory, n):
    name, p, table, keep, inp, want, want_tries = ref
    ctx = _ctx(gpu_ctx_factory, p, table)
    got, tries = ctx.camera_rays(inp[:n], lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    assert got.shape == (n, 21)
    _check(got, tries, want[:n], want_tries[:n])


def test_no_differentials(ref, gpu_ctx_factory):
    name, p, table, keep, inp, want, want_tries = ref
    ctx = _ctx(gpu_ctx_factory, p, table)
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, differentials=False, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    assert _same_bits(got[:, :9], want[:, :9]) and np.array_equal(tries, want_tries)
    assert not got[:, 9:].view(np.uint32).any()


def test_a_batch_split_in_two_calls_equals_one_call(ref, gpu_ctx_factory):
    name, p, table, keep, inp, want, want_tries = ref
    ctx = _ctx(gpu_ctx_factory, p, table)
    cut = 2049                       # inside a wave of the whole batch
    a = ctx.camera_rays(inp[:cut], first_ray=0, lam=LAM, seed=SEED, want_tries=True)
    b = ctx.camera_rays(inp[cut:], first_ray=cut, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    _check(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), want, want_tries)


# ---- e: a lens compiled at run time ---------------------------------------------------------------------------------------------
def test_run_time_lens(orc, gpu_ctx_factory, monkeypatch):
    """anamorphic_petzval_58mm: cylindrical outer pupil, no kernel of it in the library"""
    p, model, table, keep = common.po_setup(W, H, lens="anamorphic_petzval_58mm")
    lens = orc.orc_lens_create(C.byref(table))
    inp = _inputs(1024, 9, 1.1, 0.7)
    want, want_tries = oracle_rays(orc, p, lens, None, inp, seed=SEED)
    orc.orc_lens_destroy(lens)
    assert int((want_tries > 0).sum()) > 0
    ctx = _ctx(gpu_ctx_factory, p, table)
    assert not ctx.lens_is_compiled()
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() in (_abi.RAYS_PATH_INTERPRETER, _abi.RAYS_PATH_RUN_TIME)
    _check(got, tries, want, want_tries)
    ctx.lens_jit_wait(600.0)
    assert ctx.lens_jit_status()[0] == 2
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_RUN_TIME
    _check(got, tries, want, want_tries)
    ctx.set_lens_mode(1)
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER
    _check(got, tries, want, want_tries)
    monkeypatch.setenv("LENTIL_LENS_JIT", "0")          # (read when a context is created)
    off = _ctx(gpu_ctx_factory, p, table)
    assert off.lens_jit_status()[0] == 0
    got, tries = off.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    assert off.camera_rays_path() == _abi.RAYS_PATH_INTERPRETER
    _check(got, tries, want, want_tries)


# ---- f: stream order --------------------------------------------------------------------------------------------------------------
def test_rays_between_two_streamed_passes(orc, gpu_ctx_factory):
    """as tests/test_gpu_camera_rays.py::test_rays_between_two_streamed_passes (its frame, its lens), through the compiled-in
    kernel"""
    M, S = 9, 128
    p, model, table, keep = common.po_setup(W, H, samples_override=S)
    lens = orc.orc_lens_create(C.byref(table))
    inp = _inputs(1024, 21, 1.1, 0.7)
    want, want_tries = oracle_rays(orc, p, lens, None, inp, seed=SEED)
    orc.orc_lens_destroy(lens)
    visits, cols = common.make_stream(p, W, H, M, f_hi=2.0 ** -12)
    ctx = _ctx(gpu_ctx_factory, p, table)
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
    assert int(ctx.counters().streamed) == 1
    rays, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)           # lands behind the pass in flight
    assert ctx.camera_rays_path() == _abi.RAYS_PATH_COMPILED_IN
    frame()
    assert int(ctx.counters().streamed) == 1
    buf1, w1 = ctx.download_accum(0)
    assert np.array_equal(common.sort_log(ctx.draw_log()), log0)
    assert common.rel_err(buf1[buf0 != 0], buf0[buf0 != 0]) < 1e-5 and common.rel_err(w1[w0 != 0], w0[w0 != 0]) < 1e-5
    assert np.array_equal(buf1 != 0, buf0 != 0)
    _check(rays, tries, want, want_tries)
    after = capi.process_stats()
    assert after[1] - before[1] == 0, capi.process_stall_notes()


# ---- g: focus search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_name", COMPILED)
def test_focus_search_keeps_the_sequential_winner(gpu_ctx_factory, lens_name):
    p, model, table, keep = common.po_setup(64, 48, lens=lens_name)
    hl = hostlib.HostLens(model.spec)
    try:
        want = [hl.lib.lentil_host_logarithmic_focus_search(hl.h, f, LAM) for f in (300.0, 1500.0, 50000.0)]
    finally:
        hl.close()
    assert len(set(want)) == 3
    ctx = _ctx(gpu_ctx_factory, p, table)
    assert ctx.lens_is_compiled()
    for mode in (0, 1):
        ctx.set_lens_mode(mode)
        got = [ctx.focus_search(f, LAM) for f in (300.0, 1500.0, 50000.0)]
        assert got == want, (lens_name, mode, got, want)
