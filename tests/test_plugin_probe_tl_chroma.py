"""Scene occlusion through the plugin with abb_chromatic set (pota_amd/csrc/plugin/lentil_camera_node.cpp).

A thin-lens camera keeps its probe callback whatever abb_chromatic is: the frame out of the imager is the oracle's with the same
question asked through the same SDK calls (the stand-in SDK's analytic sphere behind AiTraceProbe; fa_probe_segments), and the
"not probed" warning is gone.  The thin lens draws its colour channels from one xor128 stream in the order the samples reach the
filter, so that render runs on one renderer thread: rows top to bottom, the oracle's own visit order.  Polynomial optics with abb_chromatic != 0 still says so once and renders unprobed.  Driven the way
test_plugin.py's test_scene_occlusion_through_the_plugin_matches_the_oracle drives its camera, and compared at its bar.
"""
import ctypes as C

import numpy as np
import pytest

import common
import oracle_lib
from pota_amd import _abi, capi
from test_plugin import AI_TYPE, _messages, _scene, fa  # noqa: F401  (fixture)

W, H, M, S = 64, 48, 9, 48
SPHERE = (6.0, 2.0, -70.0, 9.0)          # beside the axis, between the lens and the far highlights (cm, camera at the origin)


class _Renderer:
    def __init__(self, fa, p, f_hi):
        self.fa = fa
        visits, cols = common.make_stream(p, W, H, M, f_hi=f_hi)
        self.cols, self.n = cols, W * H * M
        n = self.n
        pix = np.arange(n) // M
        self.px = (pix % W).astype(np.int32); self.py = (pix // W).astype(np.int32)
        rng = np.random.default_rng(11)
        self.ox = rng.uniform(-0.5, 0.5, n).astype(np.float32); self.oy = rng.uniform(-0.5, 0.5, n).astype(np.float32)
        self.invd = np.full(n, 1.0 / 9.0, np.float32)
        zeros = np.zeros((n, 4), np.float32)
        z4 = np.repeat(cols["pos_z"][:, 3:4], 4, axis=1).copy()
        self.aov = {"RGBA": (AI_TYPE["RGBA"], cols["rgba"]), "P": (AI_TYPE["VECTOR"], cols["pos_z"]), "Z": (AI_TYPE["FLOAT"], z4),
                    "lentil_raydir": (AI_TYPE["RGB"], cols["raydir_time"]), "lentil_time": (AI_TYPE["FLOAT"], zeros),
                    "volume": (AI_TYPE["RGB"], zeros), "transmission": (AI_TYPE["RGBA"], zeros), "lentil_ignore": (AI_TYPE["FLOAT"], zeros)}
        self.keep = [np.ascontiguousarray(a, np.float32) for _, a in self.aov.values()]
        fa.fa_set_sphere_occluder.argtypes = [C.c_float] * 4
        fa.fa_set_sphere_occluder.restype = None
        fa.fa_probe_counts.argtypes = [C.c_void_p, C.c_int]
        fa.fa_probe_counts.restype = None
        self.counts = (C.c_uint64 * 2)()

    def render(self, sphere, configure, threads=4):
        """(image, segments the renderer was asked about, of them occluded, the messages)"""
        fa, vp = self.fa, C.c_void_p
        fa.fa_messages_clear()
        fa.fa_set_sphere_occluder(*[float(v) for v in sphere])
        fa.fa_probe_counts(self.counts, 1)
        u, cam = _scene(fa, W, H, ["RGBA RGBA gaussian_filter driver_exr"])
        configure(cam)
        fa.fa_set_samples(vp(u), self.n, self.px.ctypes.data_as(vp), self.py.ctypes.data_as(vp), self.ox.ctypes.data_as(vp),
                          self.oy.ctypes.data_as(vp), self.invd.ctypes.data_as(vp))
        for (name, (t, _)), a in zip(self.aov.items(), self.keep):
            fa.fa_set_aov(vp(u), name.encode(), t, a.ctypes.data_as(vp))
        rc = fa.fa_render(vp(u), threads, 16)
        msgs = _messages(fa)
        assert rc == 0 and fa.fa_error_count() == 0, msgs
        img = np.zeros((H, W, 4), np.float32)
        assert fa.fa_get_image(vp(u), b"RGBA", img.ctypes.data_as(vp)) == 0
        fa.fa_universe_destroy(vp(u))
        fa.fa_probe_counts(self.counts, 0)
        return img, int(self.counts[0]), int(self.counts[1]), msgs

    def oracle(self, orc, p, table, probe):
        """the resolved RGBA of the single-threaded oracle and its (attempted, accepted) draws"""
        # AOVs in the plugin's order: RGBA, lentil_debug (own z-buffer, no column), lentil_raydir (RGB widened with alpha 1)
        kinds = [_abi.FILTER_GAUSSIAN, _abi.FILTER_CLOSEST_DEBUG, _abi.FILTER_GAUSSIAN]
        ocols = dict(self.cols)
        widen = lambda a: np.ascontiguousarray(np.concatenate([a[:, :3], np.ones((self.n, 1), np.float32)], 1), np.float32)
        ocols["extra"] = [np.zeros_like(self.cols["rgba"]), widen(self.cols["raydir_time"])]
        ovisits, okeep = capi.make_visits(ocols, visits_per_pixel=M, pixels_per_row=W)
        lens = orc.orc_lens_create(C.byref(table)) if table is not None else None
        ref = oracle_lib.Frame(orc, p, n_aovs=3, kinds=kinds, keep_log=True)
        if probe:
            ref.set_probe(C.cast(self.fa.fa_probe_segments, C.c_void_p).value, None)
        ref.run(lens, None, ovisits)
        if lens:
            orc.orc_lens_destroy(lens)
        want = ref.resolve(0).reshape(p.yres, p.xres, 4)[:H, :W].copy()
        c = ref.counters()
        ref.close()
        return want, (int(c.attempted_draws), int(c.accepted_draws))


def _same(got, want):
    m = want != 0
    return np.array_equal(got != 0, m) and float(np.max(np.abs(got[m].astype(np.float64) - want[m]) / np.abs(want[m]))) < 1e-5


@pytest.mark.gpu
def test_thin_lens_with_chromatic_aberration_is_probed_through_the_plugin(fa, orc, monkeypatch):
    monkeypatch.setenv("LENTIL_SAMPLES_OVERRIDE", str(S))
    p = common.tl_setup(W, H, samples_override=S, abb_chromatic=0.6)
    r = _Renderer(fa, p, 0.03)

    def thin_lens(cam):
        fa.fa_node_set_int(C.c_void_p(cam), b"camera_type", 0)                # ThinLens
        fa.fa_node_set_flt(C.c_void_p(cam), b"fstop", C.c_float(1.4))
        fa.fa_node_set_flt(C.c_void_p(cam), b"abb_chromatic", C.c_float(0.6))

    try:
        got, probed, hits, msgs = r.render(SPHERE, thin_lens, threads=1)
        assert "not probed" not in msgs, msgs
        assert probed > 1000 and 0 < hits < probed, (probed, hits)
        fa.fa_set_sphere_occluder(*[float(v) for v in SPHERE])
        want, wc = r.oracle(orc, p, None, True)
        free, fc = r.oracle(orc, p, None, False)
        assert wc != fc                        # the occluder bites ...
        assert _same(got, want) and not _same(got, free)
        # ... and the three colour components differ: the pass was the chromatic one
        assert float(np.abs(got[..., 0] - got[..., 2]).max()) > 0.0
        # probing switched off asks nothing
        monkeypatch.setenv("LENTIL_OCCLUSION_PROBES", "0")
        got1, probed1, _, _ = r.render(SPHERE, thin_lens, threads=1)
        assert probed1 == 0 and _same(got1, free)
    finally:
        fa.fa_set_sphere_occluder(0.0, 0.0, 0.0, 0.0)


@pytest.mark.gpu
def test_polynomial_optics_with_chromatic_aberration_still_warns(fa, orc, monkeypatch):
    monkeypatch.setenv("LENTIL_SAMPLES_OVERRIDE", str(S))
    p, model, table, keep = common.po_setup(W, H, samples_override=S, focal_length=np.float32(35.0), abb_chromatic=0.5)
    r = _Renderer(fa, p, 0.03)

    def po(cam):
        fa.fa_node_set_int(C.c_void_p(cam), b"camera_type", 1)                # PolynomialOptics
        fa.fa_node_set_int(C.c_void_p(cam), b"lens_model", 0)
        fa.fa_node_set_flt(C.c_void_p(cam), b"abb_chromatic", C.c_float(0.5))

    try:
        got, probed, hits, msgs = r.render(SPHERE, po)
        assert "scene occlusion along the redistributed rays is not probed" in msgs, msgs
        assert probed == 0
        free, fc = r.oracle(orc, p, table, False)
        assert _same(got, free)
    finally:
        fa.fa_set_sphere_occluder(0.0, 0.0, 0.0, 0.0)
