"""Forward camera rays in batches on the GPU (lentil_hip_camera_rays, csrc/lentil_camera_rays.h) against the oracle.

The yardstick is the oracle's Camera::trace_ray_fw_po / trace_ray_fw_thinlens (src/lentil.h:283-569) composed the way
camera_create_ray composes them (src/lentil_camera.cpp:78-125): three traces that share r1, r2 and ONE xor128 state, float32
finite differences with inv_step = float32(1) / float32(0.001), and the ray's start state computed here, from the oracle's
tea<8>, by the rule the header states.  Every ray of every case is compared, word for word.
"""
import ctypes as C
import os

import numpy as np
import pytest

import common
from pota_amd import _abi, bokeh, capi

pytestmark = pytest.mark.gpu

W, H = 640, 360
N = 2085                   # eight blocks and a partial last wave
LAM = float(np.float32(550.0)) * 0.001

# Thin lens, coma and optical-vignetting cases only: the largest distance, in float32 ulps, a word fed by the device's
# sin / cos / log / exp / powf may lie from the oracle's (glibc's).  MEASURED on the MI355X over the seeded inputs below:
# 0 ulps -- every word of every case came out bit-identical -- so the allowance, twice the measured figure, is 0.
TL_MATH_ULPS = 0


def _bokeh_tables(orc, case=None):
    """(tables, the oracle's OrcBokeh): the reference's example kernel, or a case of tests/bokeh_tables.py"""
    if case is not None:
        import bokeh_tables
        return bokeh_tables.tables(case), bokeh_tables.oracle_bokeh(orc, case)
    tex = np.load(os.path.join(common.ROOT, "tests", "golden", "example_bokeh_kernel_u8.npy")).astype(np.float32) / np.float32(255)
    tables = bokeh.build_tables(tex)
    bt = _abi.BokehTable()
    bt.x, bt.y = tables["x"], tables["y"]
    for k in ("cdfRow", "rowIndices", "cdfColumn", "columnIndices"):
        setattr(bt, k, tables[k].ctypes.data)
    return tables, orc.orc_bokeh_from_tables(C.byref(bt))


def _inputs(n, seed, sx_max, sy_max):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-sx_max, sx_max, n), rng.uniform(-sy_max, sy_max, n), rng.uniform(0.5, 2.0, n),
                     rng.uniform(0.5, 2.0, n), rng.random(n), rng.random(n)], 1).astype(np.float32)


def oracle_rays(orc, p, lens, ob, inp, first_ray=0, lam=LAM, exposure=1.0, seed=0, differentials=True):
    """camera_create_ray over the oracle's forward traces -> ([n, 21] float32, [n] int32 tries of the main trace)"""
    n = inp.shape[0]
    out = np.zeros((n, 21), np.float32)
    tries = np.zeros(n, np.int32)
    step = np.float32(0.001)
    inv_step = np.float32(1.0) / step
    po = p.cameraType == _abi.POLYNOMIAL_OPTICS
    o, d, w = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    tr = C.c_int()
    for i in range(n):
        rid = first_ray + i
        words, x = [], seed
        for _ in range(4):
            x = orc.orc_tea8(rid, x)
            words.append(x)
        st = (C.c_uint32 * 4)(*words)
        if not any(words):
            orc.orc_xor128_init(st)
        sx, sy, dsx, dsy, lx, ly = inp[i]
        r1, r2 = C.c_double(float(lx)), C.c_double(float(ly))

        def trace(tsx, tsy, deriv):
            w[0] = w[1] = w[2] = 1.0
            if po:
                orc.orc_trace_ray_fw_po(C.byref(p), lens, ob, st, lam, float(tsx), float(tsy), C.byref(r1), C.byref(r2), deriv, o, d, w, C.byref(tr))
            else:
                orc.orc_trace_ray_fw_thinlens(C.byref(p), ob, st, float(tsx), float(tsy), C.byref(r1), C.byref(r2), deriv, o, d, w, C.byref(tr))
            return np.array(o[:], np.float32), np.array(d[:], np.float32), np.array(w[:], np.float32), tr.value

        o0, d0, w0, t0 = trace(sx, sy, 0)
        out[i, 0:3], out[i, 3:6], out[i, 6:9] = o0, d0, w0 * np.float32(exposure)
        tries[i] = t0
        if differentials:
            sxd, syd = np.float32(sx + dsx * step), np.float32(sy + dsy * step)
            o1, d1, _, _ = trace(sxd, sy, 1)
            o2, d2, _, _ = trace(sx, syd, 1)
            out[i, 9:12], out[i, 12:15] = (o1 - o0) * inv_step, (o2 - o0) * inv_step
            out[i, 15:18], out[i, 18:21] = (d1 - d0) * inv_step, (d2 - d0) * inv_step
    return out, tries


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _ulps(a, b):
    """largest distance in float32 ulps (0 for identical bit patterns, NaNs included)"""
    ua, ub = np.ascontiguousarray(a).view(np.uint32).astype(np.int64), np.ascontiguousarray(b).view(np.uint32).astype(np.int64)
    ka = np.where(ua & 0x80000000, 0x80000000 - ua, ua)
    kb = np.where(ub & 0x80000000, 0x80000000 - ub, ub)
    dist = np.abs(ka - kb)
    dist[ua == ub] = 0
    return int(dist.max()) if dist.size else 0


def _ctx(make, p, table=None, tables=None):
    ctx = make()
    ctx.set_params(p)
    if table is not None:
        ctx.set_lens(table)
    if tables is not None:
        ctx.set_bokeh(tables)
    return ctx


# ---- polynomial optics: every word bit-identical ----------------------------------------------------------------------------
PO_SETUPS = {
    "disk": dict(),
    "blades5": dict(bokeh_aperture_blades=5),
    "blades6_mm": dict(bokeh_aperture_blades=6, unitModel=_abi.UNIT_MM),
    "image": dict(bokeh_enable_image=1),
    "no_dof": dict(enable_dof=0),
    "retries0": dict(vignetting_retries=0),
}


@pytest.mark.parametrize("setup", sorted(PO_SETUPS))
@pytest.mark.parametrize("lens_name", ["double_gauss_50mm", "petzval_58mm", "anamorphic_petzval_58mm"])
def test_po_rays_bitwise(orc, gpu_ctx_factory, lens_name, setup):
    kw = PO_SETUPS[setup]
    p, model, table, keep = common.po_setup(W, H, lens=lens_name, **kw)
    if lens_name.startswith("anamorphic"):
        assert table.lens_outer_pupil_geometry != _abi.GEOM_SPHERICAL       # the cylindrical outer pupil branch
    tables, ob = _bokeh_tables(orc) if kw.get("bokeh_enable_image") else (None, None)
    lens = orc.orc_lens_create(C.byref(table))
    try:
        inp = _inputs(N, 9, 1.1, 0.7)
        want, want_tries = oracle_rays(orc, p, lens, ob, inp, seed=0x1234)
        if p.enable_dof:
            assert int((want_tries > 0).sum()) > 0, "no ray of this case retries"
        if p.vignetting_retries == 0:
            assert int((want[:, 6] == 0).sum()) > 0, "no ray of this case exhausts its tries"
        ctx = _ctx(gpu_ctx_factory, p, table, tables)
        got, got_tries = ctx.camera_rays(inp, lam=LAM, seed=0x1234, want_tries=True)
    finally:
        orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    print("%s / %s: %d rays, %d retried, %d weight 0, max ulps %d" % (lens_name, setup, N, int((want_tries > 0).sum()),
                                                                      int((want[:, 6] == 0).sum()), _ulps(got, want)))
    assert np.array_equal(got_tries, want_tries)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:2]], want[bad[:2]])


def test_po_rays_with_a_crafted_2049_table(orc, gpu_ctx_factory):
    """tests/bokeh_tables.py's crafted 2049 x 2049 table: a quarter of the rays clamp the row, half of the others the column,
    and the clamped entries are not row / column 0.  (test_po_rays_bitwise's comparison.)"""
    p, model, table, keep = common.po_setup(W, H, bokeh_enable_image=1)
    tables, ob = _bokeh_tables(orc, "clamp2049")
    plain_tables, plain = _bokeh_tables(orc)
    lens = orc.orc_lens_create(C.byref(table))
    try:
        inp = _inputs(N, 9, 1.1, 0.7)
        want, want_tries = oracle_rays(orc, p, lens, ob, inp, seed=0x1234)
        other, _ = oracle_rays(orc, p, lens, plain, inp[:64], seed=0x1234, differentials=False)
        assert not _same_bits(want[:64, 0:9], other[:, 0:9])                 # the table decides the rays
        assert int((want_tries > 0).sum()) > 0, "no ray of this case retries"
        ctx = _ctx(gpu_ctx_factory, p, table, tables)
        got, got_tries = ctx.camera_rays(inp, lam=LAM, seed=0x1234, want_tries=True)
    finally:
        orc.orc_lens_destroy(lens)
        orc.orc_bokeh_destroy(ob)
        orc.orc_bokeh_destroy(plain)
    assert np.array_equal(got_tries, want_tries)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:2]], want[bad[:2]])


# ---- thin lens -------------------------------------------------------------------------------------------------------------------
TL_SETUPS = {
    # name: (parameters, vignetting case, a coma or optical-vignetting case: the only ones TL_MATH_ULPS may ever loosen)
    "ov": (dict(optical_vignetting_distance=2.0), True, True),
    "ov_coma": (dict(optical_vignetting_distance=2.0, abb_coma=0.6), True, True),
    "coma": (dict(abb_coma=0.6), False, True),
    "distortion": (dict(abb_distortion=0.2), False, False),
    "square_ov": (dict(circle_to_square=0.5, optical_vignetting_distance=2.0), True, True),
    "anamorphic": (dict(bokeh_anamorphic=0.6), False, False),
    "blades_ov": (dict(bokeh_aperture_blades=5, optical_vignetting_distance=2.0), True, True),
    "image_ov": (dict(bokeh_enable_image=1, optical_vignetting_distance=2.0), True, True),
    "retries0_ov": (dict(vignetting_retries=0, optical_vignetting_distance=2.0), True, True),
}


@pytest.mark.parametrize("setup", sorted(TL_SETUPS))
def test_thinlens_rays(orc, gpu_ctx_factory, setup):
    kw, vignetting, coma_or_ov = TL_SETUPS[setup]
    p = common.tl_setup(W, H, **kw)
    tables, ob = _bokeh_tables(orc) if kw.get("bokeh_enable_image") else (None, None)
    try:
        inp = _inputs(N, 10, 1.0, 0.6)
        want, want_tries = oracle_rays(orc, p, None, ob, inp, seed=77, exposure=0.5)
        if vignetting:
            assert int((want_tries > 0).sum()) > 0, "no ray of this case retries"
        if p.vignetting_retries == 0:
            assert int((want[:, 6] == 0).sum()) > 0, "no ray of this case exhausts its tries"
        ctx = _ctx(gpu_ctx_factory, p, None, tables)
        got, got_tries = ctx.camera_rays(inp, seed=77, exposure=0.5, want_tries=True)
    finally:
        if ob:
            orc.orc_bokeh_destroy(ob)
    ulps = _ulps(got, want)
    print("thin lens / %s: %d rays, %d retried, %d weight 0, max ulps %d" % (setup, N, int((want_tries > 0).sum()),
                                                                            int((want[:, 6] == 0).sum()), ulps))
    assert np.array_equal(got_tries, want_tries)
    assert _same_bits(got[:, 0:3], want[:, 0:3]) and _same_bits(got[:, 6:15], want[:, 6:15])     # origin, weight, dOdx, dOdy: no libm
    assert ulps <= (TL_MATH_ULPS if coma_or_ov else 0)


def test_thinlens_rays_with_a_crafted_2049_table(orc, gpu_ctx_factory):
    """(test_thinlens_rays' "image_ov" with tests/bokeh_tables.py's crafted 2049 x 2049 table, and its comparison)"""
    p = common.tl_setup(W, H, bokeh_enable_image=1, optical_vignetting_distance=2.0)
    tables, ob = _bokeh_tables(orc, "clamp2049")
    try:
        inp = _inputs(N, 10, 1.0, 0.6)
        want, want_tries = oracle_rays(orc, p, None, ob, inp, seed=77, exposure=0.5)
        assert int((want_tries > 0).sum()) > 0, "no ray of this case retries"
        ctx = _ctx(gpu_ctx_factory, p, None, tables)
        got, got_tries = ctx.camera_rays(inp, seed=77, exposure=0.5, want_tries=True)
    finally:
        orc.orc_bokeh_destroy(ob)
    assert np.array_equal(got_tries, want_tries)
    assert _same_bits(got[:, 0:3], want[:, 0:3]) and _same_bits(got[:, 6:15], want[:, 6:15])     # origin, weight, dOdx, dOdy: no libm
    assert _ulps(got, want) <= TL_MATH_ULPS


# ---- splitting, forms, flags ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dg(orc):
    p, model, table, keep = common.po_setup(W, H)
    lens = orc.orc_lens_create(C.byref(table))
    inp = _inputs(3000, 21, 1.1, 0.7)
    want, want_tries = oracle_rays(orc, p, lens, None, inp, first_ray=0, seed=5)
    orc.orc_lens_destroy(lens)
    assert int((want_tries > 0).sum()) > 0
    return p, table, keep, inp, want, want_tries


def test_a_batch_does_not_depend_on_how_it_is_split(dg, gpu_ctx_factory):
    import torch
    p, table, keep, inp, want, want_tries = dg
    ctx = _ctx(gpu_ctx_factory, p, table)
    whole, tries = ctx.camera_rays(inp, lam=LAM, seed=5, want_tries=True)
    assert _same_bits(whole, want) and np.array_equal(tries, want_tries)
    n = inp.shape[0]
    parts = [ctx.camera_rays(inp[a:b], first_ray=a, lam=LAM, seed=5, want_tries=True) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    assert _same_bits(np.concatenate([q[0] for q in parts]), whole)
    assert np.array_equal(np.concatenate([q[1] for q in parts]), tries)
    # device pointers: torch tensors in and out, nothing waited for by the call
    t_in = torch.from_numpy(inp).cuda()
    t_out, t_tries = ctx.camera_rays(t_in, lam=LAM, seed=5, want_tries=True)
    assert t_out.is_cuda and t_out.shape == (n, 21) and t_tries.dtype == torch.int32
    ctx.sync()
    assert _same_bits(t_out.cpu().numpy(), whole) and np.array_equal(t_tries.cpu().numpy(), tries)
    with pytest.raises(ValueError):          # a copy made here would run on torch's stream, unordered with the context's
        ctx.camera_rays(torch.empty((6, n), dtype=torch.float32, device="cuda").t())
    with pytest.raises(ValueError):
        ctx.camera_rays(torch.from_numpy(inp))          # not on the context's GPU
    # other ids, other retries: the id is what seeds a ray
    moved = ctx.camera_rays(inp, first_ray=1000, lam=LAM, seed=5)
    retried = want_tries > 0
    assert _same_bits(moved[~retried], whole[~retried]) and not _same_bits(moved[retried], whole[retried])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches(dg, gpu_ctx_factory, n):
    p, table, keep, inp, want, want_tries = dg
    ctx = _ctx(gpu_ctx_factory, p, table)
    got, tries = ctx.camera_rays(inp[:n], lam=LAM, seed=5, want_tries=True)
    assert got.shape == (n, 21) and _same_bits(got, want[:n]) and np.array_equal(tries, want_tries[:n])


def test_no_differentials(dg, gpu_ctx_factory):
    p, table, keep, inp, want, want_tries = dg
    ctx = _ctx(gpu_ctx_factory, p, table)
    got, tries = ctx.camera_rays(inp, lam=LAM, seed=5, differentials=False, want_tries=True)
    assert _same_bits(got[:, :9], want[:, :9]) and np.array_equal(tries, want_tries)
    assert not got[:, 9:].view(np.uint32).any()


def test_rays_between_two_streamed_passes(dg, orc, gpu_ctx_factory):
    """a batch between two passes of a context that streams: the next pass still streams and its frame is the one it is
    without the batch in between; no stall is counted"""
    p0, table, keep, inp, want, want_tries = dg
    M, S = 9, 128
    p, model, table, keep2 = common.po_setup(W, H, samples_override=S)
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
    rays = ctx.camera_rays(inp, lam=LAM, seed=5)           # lands behind the pass in flight
    frame()
    assert int(ctx.counters().streamed) == 1
    buf1, w1 = ctx.download_accum(0)
    assert np.array_equal(common.sort_log(ctx.draw_log()), log0)
    assert common.rel_err(buf1[buf0 != 0], buf0[buf0 != 0]) < 1e-5 and common.rel_err(w1[w0 != 0], w0[w0 != 0]) < 1e-5
    assert np.array_equal(buf1 != 0, buf0 != 0)
    assert _same_bits(rays, want)
    after = capi.process_stats()
    assert after[1] - before[1] == 0, capi.process_stall_notes()


def test_invalid_calls(dg, orc, gpu_ctx_factory):
    p, table, keep, inp, want, want_tries = dg
    ctx = gpu_ctx_factory()

    def code(fn):
        with pytest.raises(capi.LentilError) as e:
            fn()
        return e.value.code

    assert code(lambda: ctx.camera_rays(inp[:4])) == _abi.ERR_INVALID                    # no parameters
    ctx.set_params(p)
    assert code(lambda: ctx.camera_rays(inp[:4])) == _abi.ERR_INVALID                    # polynomial optics, no lens
    ctx.set_lens(table)
    assert ctx.camera_rays(inp[:4], lam=LAM, seed=5).shape == (4, 21)
    assert ctx.camera_rays(inp[:0]).shape == (0, 21)                                     # n == 0: nothing launched
    assert code(lambda: ctx.camera_rays(inp[:4], first_ray=(1 << 32) - 3)) == _abi.ERR_INVALID
    assert ctx.camera_rays(inp[:4], first_ray=(1 << 32) - 4).shape == (4, 21)
    out = np.zeros((4, 21), np.float32)
    for a, b in ((None, out.ctypes.data), (inp.ctypes.data, None)):
        batch = _abi.CameraRayBatch()
        batch.n, batch.inp, batch.out, batch.lam, batch.exposure = 4, a, b, LAM, 1.0
        assert ctx.lib.lentil_hip_camera_rays(ctx.h, C.byref(batch)) == _abi.ERR_INVALID
    assert ctx.lib.lentil_hip_camera_rays(ctx.h, None) == _abi.ERR_INVALID
    pi, model, table_i, keep_i = common.po_setup(W, H, bokeh_enable_image=1)
    ctx.set_params(pi)
    assert code(lambda: ctx.camera_rays(inp[:4])) == _abi.ERR_INVALID                    # bokeh_enable_image, no tables
    # a thin lens needs no lens table
    tl = gpu_ctx_factory()
    tl.set_params(common.tl_setup(W, H))
    assert tl.camera_rays(inp[:4]).shape == (4, 21)
