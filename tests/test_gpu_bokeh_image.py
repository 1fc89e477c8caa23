"""The aperture-image sampler (bokeh_sample, pota_amd/csrc/lentil_device.h) in the kernels it is compiled into, against the
oracle, over the tables of tests/bokeh_tables.py (what each is there for: that module; that the cases bite: tests/
test_bokeh_table_cases.py, no GPU).

  the sampler alone        lentil_hip_test_aperture_sample against orc_po_aperture_sample over 20 000 seed pairs, every table, fp64
                           outputs bit for bit: the search, the clamps, the centring, the indices
  through a pass           polynomial optics (compiled lens, table interpreter, run-time kernel) and the thin lens (plain,
                           anamorphic, abb_chromatic > 0), twice on one context -- chunked, then blind or streamed: counters and
                           accepted-draw lists the oracle's, the frame within 1e-5.  Tables on both sides of kMaxBokehRows = 2048:
                           the solve kernels stage cdfRow in LDS up to there and read global memory above.  With blades the image
                           loses in polynomial optics (po_aperture_sample) and wins on the thin lens (thinlens_ray)
  with an occlusion probe  probe_list_kernel / tl_chroma_probe_list_kernel read the tables from global memory
  the context's state      a second image, a table beyond the LDS limit on a live context, refused tables, the image taken away
(Across ranks: tests/test_native_exchange_tl_chroma.py; camera rays: tests/test_gpu_camera_rays.py.)

Out of scope: an all-black image (tests/bokeh_tables.py says why)."""
import ctypes as C

import numpy as np
import pytest

import bokeh_tables
import common
import oracle_lib
from pota_amd import _abi, bokeh, capi
from test_gpu_parity import check_frame, check_logs

pytestmark = pytest.mark.gpu

W, H, M = 48, 40, 9
SAMPLES = 16
F_HI = 0.02
TL_CHROMA_KINDS = [0, 0, 1]         # test_gpu_parity's chromatic thin-lens case: RGBA, a gaussian and a closest extra AOV
SPHERE = (6.0, 2.0, -70.0, 9.0)     # tests/test_gpu_probe.py's: beside the optical axis, between the lens and the far highlights


# ---- the sampler alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bokeh_tables.CASES, ids=[c["name"] for c in bokeh_tables.CASES])
def test_sampler_bit_for_bit(orc, gpu_ctx_factory, case):
    want = bokeh_tables.oracle_samples(orc, case["name"])
    ctx = gpu_ctx_factory()
    ctx.set_params(bokeh_tables.sampler_params())
    ctx.set_bokeh(bokeh_tables.tables(case["name"]))
    a, b = bokeh_tables.seed_pairs()
    got = ctx.test_aperture_sample(a, b)
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    assert bad.size == 0, "%s: %d of %d aperture points differ, first at draw %d: %s against %s" % (
        case["name"], bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]])


# ---- through the pass ----------------------------------------------------------------------------------------------------------
def _camera(camera, lens="double_gauss_50mm", image=1, **kw):
    """(params, lens table or None, keepalive, kinds)"""
    if camera == "po":
        p, model, table, keep = common.po_setup(W, H, lens=lens, samples_override=SAMPLES, bokeh_enable_image=image, **kw)
        return p, table, (model, keep), [0]
    p = common.tl_setup(W, H, samples_override=SAMPLES, bokeh_enable_image=image, **kw)
    return p, None, None, (TL_CHROMA_KINDS if float(p.abb_chromatic) > 0 else [0])


def _stream(p, kinds, w=W, h=H):
    return common.make_stream(p, w, h, M, f_hi=F_HI, n_extra=len(kinds) - 1)


def _oracle(orc, p, table, visits, kinds, ob, probe=None, start=None):
    """(frame, xor128 state at the end or None).  The thin lens with abb_chromatic > 0 draws its channels from one xor128 stream:
    a single-threaded frame that starts at `start`; everything else: common.ThreadedOracle."""
    if p.cameraType != _abi.POLYNOMIAL_OPTICS and float(p.abb_chromatic) > 0:
        ref = oracle_lib.Frame(orc, p, n_aovs=len(kinds), kinds=kinds, keep_log=True)
        if probe is not None:
            ref.set_probe(*probe)
        if start is not None:
            orc.orc_frame_set_xor128(ref.h, (C.c_uint32 * 4)(*start))
        ref.run(None, ob, visits)
        st = (C.c_uint32 * 4)()
        orc.orc_frame_get_xor128(ref.h, st)
        return ref, list(st)
    return common.ThreadedOracle(orc, p, table, visits, 4, n_aovs=len(kinds), kinds=kinds, bokeh=ob, probe=probe), None


def _set_up(ctx, p, table, kinds, tables, lens_mode=0, compiled=True):
    ctx.set_params(p)
    ctx.set_lens_mode(lens_mode)
    if table is not None:
        ctx.set_lens(table)
        assert ctx.lens_is_compiled() == compiled
    ctx.set_bokeh(tables)
    ctx.alloc_frame(len(kinds), kinds)


def _pass(ctx, visits):
    """(as tests/test_gpu_scan_shapes.py's)"""
    ctx.set_draw_log(1 << 20)
    ctx.upload_visits(visits)
    ctx.clear_frame()
    ctx.redistribute()
    ctx.resolve()
    ctx.sync()
    c = ctx.counters()
    assert c.worklist_overflow == 0
    return c


def _same_counters(c, ref):
    rc = ref.counters()
    assert (c.visits, c.redistributed_visits, c.attempted_draws, c.accepted_draws) == (
        rc.visits, rc.redistributed_visits, rc.attempted_draws, rc.accepted_draws)


def _same_pass(ctx, c, ref, kinds):
    _same_counters(c, ref)
    check_logs(ctx, ref)
    check_frame(ctx, ref, n_aovs=len(kinds), kinds=kinds)


def _sorted_log(ref):
    return common.sort_log(ref.log())


# id: (camera, table, lens, lens mode, parameters)
MATRIX = {
    "po-size8": ("po", "size8", "double_gauss_50mm", 0, {}),
    "po-clamp16": ("po", "clamp16", "double_gauss_50mm", 0, {}),
    "po-size2048": ("po", "size2048", "double_gauss_50mm", 0, {}),
    "po-size2049": ("po", "size2049", "double_gauss_50mm", 0, {}),
    "po-clamp2049": ("po", "clamp2049", "double_gauss_50mm", 0, {}),
    "po-interpreter-size2049": ("po", "size2049", "double_gauss_50mm", 1, {}),
    "po-interpreter-clamp16": ("po", "clamp16", "double_gauss_50mm", 1, {}),
    "po-runtime-kernel-clamp16": ("po", "clamp16", "anamorphic_petzval_58mm", 0, {}),
    "po-blades6-size9": ("po", "size9", "double_gauss_50mm", 0, dict(bokeh_aperture_blades=6)),
    "thinlens-size8": ("thinlens", "size8", None, 0, {}),
    "thinlens-clamp16": ("thinlens", "clamp16", None, 0, {}),
    "thinlens-size2048": ("thinlens", "size2048", None, 0, {}),
    "thinlens-size2049": ("thinlens", "size2049", None, 0, {}),
    "thinlens-blades6-size9": ("thinlens", "size9", None, 0, dict(bokeh_aperture_blades=6)),
    "thinlens-anamorphic-clamp16": ("thinlens", "clamp16", None, 0, dict(bokeh_anamorphic=0.5)),
    "thinlens-chroma-clamp16": ("thinlens", "clamp16", None, 0, dict(abb_chromatic=0.5, abb_chromatic_type=0)),
    "thinlens-chroma-size2049": ("thinlens", "size2049", None, 0, dict(abb_chromatic=0.5, abb_chromatic_type=0)),
}


@pytest.mark.parametrize("row", sorted(MATRIX))
def test_image_through_the_pass(orc, gpu_ctx_factory, row):
    camera, name, lens, lens_mode, kw = MATRIX[row]
    p, table, keep, kinds = _camera(camera, lens or "double_gauss_50mm", **kw)
    visits, cols = _stream(p, kinds)
    tables = bokeh_tables.tables(name)
    ob = bokeh_tables.oracle_bokeh(orc, name)
    refs = []
    try:
        ref, end = _oracle(orc, p, table, visits, kinds, ob)
        refs.append(ref)
        rc = ref.counters()
        assert rc.redistributed_visits > 100 and rc.accepted_draws > 1000
        if kw.get("bokeh_aperture_blades"):
            # the same camera without the image: in polynomial optics the blades win over it, on the thin lens the image wins
            q = _camera(camera, lens or "double_gauss_50mm", image=0, **kw)[0]
            blades, _ = _oracle(orc, q, table, visits, kinds, None)
            refs.append(blades)
            same = np.array_equal(_sorted_log(ref), _sorted_log(blades))
            assert same == (camera == "po"), "the draws %s those of the blades alone" % ("are" if same else "are not")
        ctx = gpu_ctx_factory()
        runtime_kernel = lens is not None and lens.startswith("anamorphic")
        _set_up(ctx, p, table, kinds, tables, lens_mode, compiled=not runtime_kernel)
        if runtime_kernel:                       # (tests/test_gpu_lens_jit.py: set_lens started the compilation; wait for the kernel)
            ctx.lens_jit_wait(600.0)
            assert ctx.lens_jit_status()[0] == 2
        for again in (0, 1):
            c = _pass(ctx, visits)
            if again == 0:
                assert c.streamed == 0 and c.blind_chunks == 0
            elif lens_mode == 1 and tables["y"] > bokeh_tables.LDS_ROWS:
                assert c.streamed == 1 and c.fallback_chunks == 0, ctx.last_redo_note()
            _same_pass(ctx, c, ref, kinds)
            if end is not None:
                assert ctx.get_xor128_state() == end
                assert set(np.unique(ctx.draw_log()[:, 1] >> 30)) == {0, 1, 2}
                if again == 0:                   # the next pass continues the generator's stream
                    ref, end = _oracle(orc, p, table, visits, kinds, ob, start=end)
                    refs.append(ref)
    finally:
        for r in refs:
            r.close()
        orc.orc_bokeh_destroy(ob)


# ---- with an occlusion probe ---------------------------------------------------------------------------------------------------
PROBED = {
    "po-clamp16": ("po", {}),
    "thinlens-clamp16": ("thinlens", {}),
    "thinlens-chroma-clamp16": ("thinlens", dict(abb_chromatic=0.5, abb_chromatic_type=0)),
}


@pytest.mark.parametrize("row", sorted(PROBED))
def test_image_with_an_occlusion_probe(orc, gpu_ctx_factory, row):
    """The analytic sphere of tests/test_gpu_probe.py on both sides.  The probe kernels form each try's aperture point again,
    from the tables in global memory: the draws are the oracle's only if they form the point the solve formed."""
    camera, kw = PROBED[row]
    p, table, keep, kinds = _camera(camera, **kw)
    visits, cols = _stream(p, kinds)
    sphere = np.array(SPHERE, np.float32)
    probe = (oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
    ob = bokeh_tables.oracle_bokeh(orc, "clamp16")
    refs = []
    try:
        ref, end = _oracle(orc, p, table, visits, kinds, ob, probe=probe)
        refs.append(ref)
        free, _ = _oracle(orc, p, table, visits, kinds, ob)
        refs.append(free)
        assert ref.counters().accepted_draws > 1000
        assert not np.array_equal(_sorted_log(ref), _sorted_log(free)), "the sphere occludes nothing"
        ctx = gpu_ctx_factory()
        _set_up(ctx, p, table, kinds, bokeh_tables.tables("clamp16"))
        ctx.set_occlusion_probe(*probe)
        for again in (0, 1):
            before = ctx.probe_stats()
            c = _pass(ctx, visits)
            assert c.streamed == 0               # (with a probe a pass may not stream)
            _same_pass(ctx, c, ref, kinds)
            probed, occluded, calls = (x - y for x, y in zip(ctx.probe_stats(), before))
            assert 0 < occluded < probed, (probed, occluded, calls)
            if end is not None:
                assert ctx.get_xor128_state() == end
                if again == 0:
                    ref, end = _oracle(orc, p, table, visits, kinds, ob, probe=probe, start=end)
                    refs.append(ref)
    finally:
        for r in refs:
            r.close()
        orc.orc_bokeh_destroy(ob)


# ---- the context's state -------------------------------------------------------------------------------------------------------
def _other_size8_image():
    """an image of size8's size that is not size8's"""
    t = bokeh.build_tables(np.random.default_rng(0x0B0E).random((8, 8, 3), dtype=np.float32))
    a = bokeh_tables.tables("size8")
    assert (t["x"], t["y"]) == (a["x"], a["y"]) and not np.array_equal(t["rowIndices"], a["rowIndices"])
    assert not np.array_equal(t["cdfRow"], a["cdfRow"])
    return t


def test_a_second_image_on_a_live_context(orc, gpu_ctx_factory):
    """lentil_hip_set_bokeh frees and reallocates the four tables and forgets the first-batch model of the image before: a pass
    with image A, then B of the same size -- two passes, the oracle's with B --, then a table beyond the LDS limit."""
    p, table, keep, kinds = _camera("po")
    visits, cols = _stream(p, kinds)
    tb = _other_size8_image()
    btb = bokeh_tables.abi_table(tb)
    obs = [bokeh_tables.oracle_bokeh(orc, "size8"), orc.orc_bokeh_from_tables(C.byref(btb)), bokeh_tables.oracle_bokeh(orc, "clamp2049")]
    refs = []
    try:
        refs = [_oracle(orc, p, table, visits, kinds, ob)[0] for ob in obs]
        logs = [_sorted_log(r) for r in refs]
        assert not np.array_equal(logs[0], logs[1]) and not np.array_equal(logs[1], logs[2])
        ctx = gpu_ctx_factory()
        _set_up(ctx, p, table, kinds, bokeh_tables.tables("size8"))
        _same_pass(ctx, _pass(ctx, visits), refs[0], kinds)
        ctx.set_bokeh(tb)
        for _ in range(2):
            _same_pass(ctx, _pass(ctx, visits), refs[1], kinds)
        ctx.set_bokeh(bokeh_tables.tables("clamp2049"))
        _same_pass(ctx, _pass(ctx, visits), refs[2], kinds)
    finally:
        for r in refs:
            r.close()
        for ob in obs:
            orc.orc_bokeh_destroy(ob)


def _code(fn):
    with pytest.raises(capi.LentilError) as e:
        fn()
    return e.value.code


def test_refused_tables_and_a_missing_image(orc, gpu_ctx_factory):
    """Everything here is refused on the host, before any launch."""
    p, table, keep, kinds = _camera("po")
    visits, cols = _stream(p, kinds)
    a, b = bokeh_tables.seed_pairs()
    t8 = bokeh_tables.tables("size8")
    ctx = gpu_ctx_factory()
    _set_up(ctx, p, table, kinds, t8)
    ctx.set_draw_log(1 << 20)
    ctx.upload_visits(visits)
    ctx.clear_frame()
    # the image taken away, bokeh_enable_image still 1
    ctx.set_bokeh(None)
    inp = np.zeros((4, 6), np.float32)
    assert _code(ctx.redistribute) == _abi.ERR_INVALID
    assert _code(lambda: ctx.camera_rays(inp)) == _abi.ERR_INVALID
    assert _code(lambda: ctx.test_aperture_sample(a[:64], b[:64])) == _abi.ERR_INVALID
    # a table that is not square, one with a null array, one of size 0
    ctx.set_bokeh(t8)

    def raw(x, y, **null):
        bt = bokeh_tables.abi_table(t8)
        bt.x, bt.y = x, y
        for k in null:
            setattr(bt, k, None)
        ctx._chk(ctx.lib.lentil_hip_set_bokeh(ctx.h, C.byref(bt)))

    assert _code(lambda: raw(8, 4)) == _abi.ERR_INVALID
    assert _code(lambda: raw(4, 8)) == _abi.ERR_INVALID
    for k in ("cdfRow", "rowIndices", "cdfColumn", "columnIndices"):
        assert _code(lambda: raw(8, 8, **{k: True})) == _abi.ERR_INVALID
    assert _code(lambda: raw(0, 0)) == _abi.ERR_INVALID
    # ... each of which left the context without an image
    assert _code(lambda: ctx.test_aperture_sample(a[:64], b[:64])) == _abi.ERR_INVALID
    # a valid table afterwards works: the sampler and a pass
    ctx.set_bokeh(t8)
    want = bokeh_tables.oracle_samples(orc, "size8")
    assert np.array_equal(ctx.test_aperture_sample(a, b).view(np.uint64), want.view(np.uint64))
    ob = bokeh_tables.oracle_bokeh(orc, "size8")
    ref, _ = _oracle(orc, p, table, visits, kinds, ob)
    try:
        _same_pass(ctx, _pass(ctx, visits), ref, kinds)
    finally:
        ref.close()
        orc.orc_bokeh_destroy(ob)
