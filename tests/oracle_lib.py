"""ctypes binding of oracle/liblentil_oracle.so -- TEST INFRASTRUCTURE (the checker)."""
import ctypes as C
import os
import subprocess

import numpy as np

from pota_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "oracle", "liblentil_oracle.so")


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def load():
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(
            os.path.join(ROOT, "oracle", "lentil_oracle.cpp")):
        build()
    L = C.CDLL(_SO)
    d, f, i, u32, u64, vp = C.c_double, C.c_float, C.c_int, C.c_uint32, C.c_uint64, C.c_void_p
    pd = C.POINTER(C.c_double)
    sig = {
        "orc_tea8": (u32, [u32, u32]),
        "orc_rng": (f, [C.POINTER(u32)]),
        "orc_xor128": (u32, [C.POINTER(u32)]),
        "orc_xor128_init": (None, [C.POINTER(u32)]),
        "orc_fast_sin": (f, [f]), "orc_fast_cos": (f, [f]),
        "orc_concentric_disk_sample": (None, [d, d, pd]),
        "orc_concentricDiskSample": (None, [f, f, pd, f, f]),
        "orc_triangular_aperture": (None, [pd, pd, d, d, d, i]),
        "orc_normalise": (None, [pd]),
        "orc_sphereToCs": (None, [pd, pd, pd, pd, d, d]),
        "orc_csToSphere": (None, [pd, pd, pd, pd, d, d]),
        "orc_cylinderToCs": (None, [pd, pd, pd, pd, d, d, i]),
        "orc_csToCylinder": (None, [pd, pd, pd, pd, d, d, i]),
        "orc_lens_ipow": (d, [d, i]),
        "orc_lens_create": (vp, [C.POINTER(_abi.LensTable)]),
        "orc_lens_destroy": (None, [vp]),
        "orc_poly_eval": (d, [vp, i, pd]),
        "orc_inv2x2": (None, [pd, pd, pd]),
        "orc_newton_step": (None, [pd, pd, d, pd, pd]),
        "orc_newton_error_bits": (i, [d, d, d, d, d, d, d]),
        "orc_lt_sample_aperture": (d, [vp, pd, pd, pd, pd, d, C.POINTER(i)]),
        "orc_lens_evaluate": (d, [vp, pd, pd]),
        "orc_pt_sample_aperture": (None, [vp, pd, pd, d]),
        "orc_bokeh_create": (vp, [vp, i, i, i]),
        "orc_bokeh_from_tables": (vp, [C.POINTER(_abi.BokehTable)]),
        "orc_bokeh_destroy": (None, [vp]),
        "orc_bokeh_tables": (None, [vp, vp, vp, vp, vp]),
        "orc_bokeh_sample": (None, [vp, f, f, pd]),
        "orc_po_aperture_sample": (None, [C.POINTER(_abi.Params), vp, u32, u32, pd]),
        "orc_trace_ray_bw_po": (i, [C.POINTER(_abi.Params), vp, vp, pd, pd, i, i, i, f, C.POINTER(i)]),
        "orc_get_coc_thinlens": (f, [C.POINTER(_abi.Params), f]),
        "orc_additional_luminance_soft_trans": (f, [C.POINTER(_abi.Params), f]),
        "orc_draw_count": (i, [C.POINTER(_abi.Params), f, f, f]),
        "orc_frame_create": (vp, [u32, u32, u32, vp, i]),
        "orc_frame_destroy": (None, [vp]),
        "orc_frame_buffer": (C.POINTER(f), [vp, u32]),
        "orc_frame_weight": (C.POINTER(f), [vp]),
        "orc_frame_zbuffer": (C.POINTER(f), [vp]),
        "orc_frame_zvisit": (C.POINTER(u32), [vp]),
        "orc_frame_buffer64": (pd, [vp, u32]),
        "orc_frame_weight64": (pd, [vp]),
        "orc_frame_counters": (None, [vp, C.POINTER(_abi.Counters)]),
        "orc_frame_set_xor128": (None, [vp, C.POINTER(C.c_uint32)]),
        "orc_frame_get_xor128": (None, [vp, C.POINTER(C.c_uint32)]),
        "orc_frame_log": (u64, [vp, vp, u64]),
        "orc_frame_set_crypto": (None, [vp, u32, u32, vp, vp]),
        "orc_frame_rebind_crypto": (i, [vp, u32, u32, vp, vp]),
        "orc_crypto_construct_cache": (i, [i, vp, vp, vp, vp, i]),
        "orc_crypto_rank": (None, [vp, u32, i, vp, vp]),
        "orc_crypto_pixel": (i, [vp, u32, u64, vp, vp, i, C.POINTER(f)]),
        "orc_frame_merge": (None, [vp, vp]),
        "orc_frame_set_camera_motion": (None, [vp, u32, vp]),
        "orc_frame_set_probe": (None, [vp, vp, vp, vp, u32]),
        "orc_frame_set_camera_shutter": (None, [vp, C.c_float, C.c_float]),
        "orc_redistribute": (i, [C.POINTER(_abi.Params), vp, vp, vp, C.POINTER(_abi.Visits), u64, u64]),
        "orc_redistribute_threads": (i, [C.POINTER(_abi.Params), vp, vp, vp, C.POINTER(_abi.Visits), u64, u64, u32, u64]),
        "orc_resolve": (None, [vp, u32, vp]),
        "orc_inverse_sample_density": (f, [i, f, i, C.POINTER(i)]),
        "orc_filter_closest_complete": (None, [i, vp, vp, i, vp]),
        "orc_filter_gaussian_complete": (None, [i, vp, vp, vp, i, f, i, f, vp, vp]),
        "orc_camera_get_y0_intersection_distance": (d, [vp, d, d]),
        "orc_logarithmic_focus_search": (d, [vp, d, d]),
        "orc_trace_backwards_for_fstop": (None, [vp, d, d, pd, pd]),
        "orc_trace_ray_focus_check": (i, [vp, d, d, pd]),
        "orc_trace_ray_fw_po": (None, [C.POINTER(_abi.Params), vp, vp, C.POINTER(u32), d, d, d, pd, pd, i,
                                       C.POINTER(f), C.POINTER(f), C.POINTER(f), C.POINTER(i)]),
        "orc_trace_ray_fw_thinlens": (None, [C.POINTER(_abi.Params), vp, C.POINTER(u32), d, d, pd, pd, i,
                                             C.POINTER(f), C.POINTER(f), C.POINTER(f), C.POINTER(i)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def sphere_occluder(lib):
    """address of orc_sphere_occluder, an analytic lentil_probe_fn: user -> four floats (centre, radius)"""
    return C.cast(lib.orc_sphere_occluder, C.c_void_p).value


def darr(*vals):
    return (C.c_double * len(vals))(*vals)


class Frame:
    """Oracle frame wrapper: run visits, read buffers as numpy."""

    def __init__(self, lib, params, n_aovs=1, kinds=None, keep_log=False, shadow=True):
        self.lib, self.params, self.n_aovs = lib, params, n_aovs
        k = (C.c_uint8 * n_aovs)(*(kinds or [0] * n_aovs))
        self.h = lib.orc_frame_create(params.xres, params.yres, n_aovs, C.cast(k, C.c_void_p), int(bool(keep_log)) | (0 if shadow else 2))
        self.np = params.xres * params.yres

    def run(self, lens, bokeh, visits, v0=0, v1=None):
        v1 = visits.n if v1 is None else v1
        rc = self.lib.orc_redistribute(C.byref(self.params), lens, bokeh, self.h, C.byref(visits), v0, v1)
        if rc:
            raise RuntimeError("oracle redistribute rc=%d" % rc)

    def run_threads(self, lens, bokeh, visits, n_threads, row_visits, v0=0, v1=None):
        """the same visits over n_threads threads into this one frame (orc_redistribute_threads): own-pixel sums by the thread
        that owns the rows, the draws added afterwards in visit order.  Returns False where that form does not apply."""
        v1 = visits.n if v1 is None else v1
        rc = self.lib.orc_redistribute_threads(C.byref(self.params), lens, bokeh, self.h, C.byref(visits), v0, v1, int(n_threads), int(row_visits))
        if rc == _abi.ERR_UNSUPPORTED:
            return False
        if rc:
            raise RuntimeError("oracle redistribute (threads) rc=%d" % rc)
        return True

    def run_auto(self, lens, bokeh, visits):
        """run_threads over this machine's CPUs where that form takes the stream (a uniform one), else run: for tests whose
        comparisons of draws' sums are made at the 1e-5 bar anyway (counters, draw log, untouched pixels: identical either way)"""
        rv = int(visits.pixels_per_row) * int(visits.visits_per_pixel)
        n = min(os.cpu_count() or 1, 32)
        if not (n > 1 and rv > 0 and int(visits.n) >= 20000 and self.run_threads(lens, bokeh, visits, n, rv)):
            self.run(lens, bokeh, visits)

    def buffer(self, aov=0):
        return np.ctypeslib.as_array(self.lib.orc_frame_buffer(self.h, aov), (self.np, 4)).copy()

    def weight(self):
        return np.ctypeslib.as_array(self.lib.orc_frame_weight(self.h), (self.np,)).copy()

    def zbuffer(self):
        return np.ctypeslib.as_array(self.lib.orc_frame_zbuffer(self.h), (self.np,)).copy()

    def zvisit(self):
        return np.ctypeslib.as_array(self.lib.orc_frame_zvisit(self.h), (self.np,)).copy()

    def buffer64(self, aov=0):
        return np.ctypeslib.as_array(self.lib.orc_frame_buffer64(self.h, aov), (self.np, 4)).copy()

    def weight64(self):
        return np.ctypeslib.as_array(self.lib.orc_frame_weight64(self.h), (self.np,)).copy()

    def resolve(self, aov=0):
        out = np.empty((self.np, 4), np.float32)
        self.lib.orc_resolve(self.h, aov, out.ctypes.data)
        return out

    def counters(self):
        c = _abi.Counters()
        self.lib.orc_frame_counters(self.h, C.byref(c))
        return c

    def log(self):
        n = self.lib.orc_frame_log(self.h, None, 0)
        rec = np.empty((n, 3), np.uint32)
        self.lib.orc_frame_log(self.h, rec.ctypes.data, n)
        return rec

    def set_crypto(self, hashes, weights):
        """per-AOV lists of [n, entries] fp32 arrays (kept alive by the wrapper)"""
        n = len(hashes)
        self._crypto_keep = ([np.ascontiguousarray(h, np.float32) for h in hashes],
                             [np.ascontiguousarray(w, np.float32) for w in weights])
        hp = (C.c_void_p * n)(*[h.ctypes.data for h in self._crypto_keep[0]])
        wp = (C.c_void_p * n)(*[w.ctypes.data for w in self._crypto_keep[1]])
        self.lib.orc_frame_set_crypto(self.h, n, self._crypto_keep[0][0].shape[1], C.cast(hp, C.c_void_p), C.cast(wp, C.c_void_p))

    def rebind_crypto(self, hashes, weights):
        """the columns of another stream (as many AOVs and entries); the maps stay: the next run adds to them"""
        n = len(hashes)
        keep = ([np.ascontiguousarray(h, np.float32) for h in hashes], [np.ascontiguousarray(w, np.float32) for w in weights])
        hp = (C.c_void_p * n)(*[h.ctypes.data for h in keep[0]])
        wp = (C.c_void_p * n)(*[w.ctypes.data for w in keep[1]])
        rc = self.lib.orc_frame_rebind_crypto(self.h, n, keep[0][0].shape[1], C.cast(hp, C.c_void_p), C.cast(wp, C.c_void_p))
        assert rc == 0, "rebind_crypto: another number of AOVs or entries than set_crypto's"
        self._crypto_keep = keep

    def set_probe(self, fn, user=None, camera_to_world=None):
        """the occlusion probe (include/lentil_hip.h: lentil_probe_fn) as the address of a C function, e.g. sphere_occluder()"""
        self._probe_keep = np.ascontiguousarray(camera_to_world, np.float32) if camera_to_world is not None else None
        n = 0 if self._probe_keep is None else (1 if self._probe_keep.ndim == 2 else self._probe_keep.shape[0])
        self.lib.orc_frame_set_probe(self.h, fn, user, self._probe_keep.ctypes.data if self._probe_keep is not None else None, n)

    def set_camera_shutter(self, start, end):
        self.lib.orc_frame_set_camera_shutter(self.h, float(start), float(end))

    def set_camera_motion(self, keys):
        """[n, 4, 4] world-to-camera matrices at shutter-relative times 0 ... 1"""
        k = np.ascontiguousarray(keys, np.float32)
        self.lib.orc_frame_set_camera_motion(self.h, k.shape[0], k.ctypes.data)

    def crypto_rank(self, crypto, rank):
        out = np.zeros((self.np, 4), np.float32)
        has = np.zeros(self.np, np.uint8)
        self.lib.orc_crypto_rank(self.h, crypto, rank, out.ctypes.data, has.ctypes.data)
        return out, has.astype(bool)

    def crypto_pixel(self, crypto, p, cap=256):
        ids = np.empty(cap, np.float32); wts = np.empty(cap, np.float32)
        tot = C.c_float()
        n = self.lib.orc_crypto_pixel(self.h, crypto, p, ids.ctypes.data, wts.ctypes.data, cap, C.byref(tot))
        assert n <= cap
        return ids[:n].copy(), wts[:n].copy(), tot.value

    def close(self):
        if self.h:
            self.lib.orc_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
