"""ctypes binding of liblentil_hip.so (the C-ABI declared in include/lentil_hip.h).

The product path: no CPU fallback.  If the HIP library is missing or no GPU is present the
calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LENTIL_HIP_LIB") or os.path.join(_PKG, "liblentil_hip.so")   # override: A/B runs of two builds

EXPORTS = [
    "lentil_hip_abi_version", "lentil_hip_create", "lentil_hip_destroy", "lentil_hip_last_error", "lentil_hip_last_redo_note",
    "lentil_hip_set_params", "lentil_hip_set_lens", "lentil_hip_set_bokeh", "lentil_hip_alloc_frame", "lentil_hip_set_camera_motion", "lentil_hip_set_camera_shutter",
    "lentil_hip_upload_visits", "lentil_hip_bind_visits", "lentil_hip_clear_frame",
    "lentil_hip_redistribute", "lentil_hip_resolve", "lentil_hip_sync", "lentil_hip_download_aov",
    "lentil_hip_download_accum", "lentil_hip_download_records", "lentil_hip_accum_buffer", "lentil_hip_stream",
    "lentil_hip_set_closest_exchange", "lentil_hip_zkey_buffer", "lentil_hip_closest_gather",
    "lentil_hip_touched_rows", "lentil_hip_merge_rows", "lentil_hip_resolve_rows",
    "lentil_hip_pack_rows", "lentil_hip_merge_packed_rows", "lentil_hip_compact_rows", "lentil_hip_merge_sparse",
    "lentil_hip_get_counters", "lentil_hip_last_timing", "lentil_hip_last_launches", "lentil_hip_set_draw_log",
    "lentil_hip_batch_model_stats", "lentil_hip_process_stats", "lentil_hip_process_stall_notes", "lentil_hip_set_async", "lentil_hip_pass_totals", "lentil_hip_set_occlusion_probe", "lentil_hip_probe_stats",
    "lentil_hip_set_occlusion_probe_device", "lentil_hip_probe_device_stats", "lentil_hip_test_sphere_occluder_device", "lentil_hip_debug_batch_estimate", "lentil_hip_box_probe",
    "lentil_hip_lens_jit_status", "lentil_hip_lens_jit_wait", "lentil_hip_debug_lens_jit_source", "lentil_hip_debug_lens_jit_compile",
    "lentil_hip_download_draw_log", "lentil_hip_test_lt_sample_aperture",
    "lentil_hip_test_trace_bw_po", "lentil_hip_test_aperture_sample", "lentil_hip_debug_scan_bands", "lentil_hip_debug_scan_lean_counts", "lentil_hip_debug_last_scan", "lentil_hip_debug_last_crypto",
    "lentil_hip_lens_is_compiled", "lentil_hip_set_lens_mode",
    "lentil_hip_focus_search", "lentil_hip_test_y0_intersection", "lentil_hip_camera_rays", "lentil_hip_camera_rays_path",
    "lentil_hip_trace_points", "lentil_hip_trace_points_path",
    "lentil_hip_camera_rays_spectral", "lentil_hip_trace_points_spectral",
    "lentil_hip_plan_visits", "lentil_hip_list_draws", "lentil_hip_list_draws_path", "lentil_hip_draw_channels",
    "lentil_hip_list_draws_spectral", "lentil_hip_trace_points_probed",
    "lentil_hip_set_visit_lambdas", "lentil_hip_spectral_pass_stats",
    "lentil_hip_set_xor128_state", "lentil_hip_get_xor128_state", "lentil_hip_tl_chroma_stats", "lentil_hip_test_xor128_jump",
    "lentil_hip_host_alloc", "lentil_hip_host_free", "lentil_hip_visits_begin", "lentil_hip_visits_append",
    "lentil_hip_visits_wait", "lentil_hip_visits_end",
    "lentil_hip_comm_unique_id", "lentil_hip_comm_init", "lentil_hip_comm_destroy", "lentil_hip_allreduce",
    "lentil_hip_exchange_bands", "lentil_hip_exchange_stats", "lentil_hip_exchange_counts", "lentil_hip_degenerate_stats", "lentil_hip_streams_concurrent",
    "lentil_hip_alloc_crypto", "lentil_hip_upload_crypto", "lentil_hip_bind_crypto", "lentil_hip_download_crypto",
    "lentil_hip_download_crypto_table", "lentil_hip_visits_begin_crypto", "lentil_hip_visits_append_crypto",
]

# lentil_hip_debug_last_scan()[0]: the scan kernels (include/lentil_hip.h, LENTIL_SCAN_*)
SCAN_DMA2, SCAN_DMA, SCAN_DMA_MULTI, SCAN_UNIFORM, SCAN_UNIFORM_MULTI, SCAN_RUNS, SCAN_RAGGED = range(1, 8)
SCAN_NAMES = {SCAN_DMA2: "dma2", SCAN_DMA: "dma", SCAN_DMA_MULTI: "dma_multi", SCAN_UNIFORM: "uniform",
              SCAN_UNIFORM_MULTI: "uniform_multi", SCAN_RUNS: "runs", SCAN_RAGGED: "ragged"}
# lentil_hip_debug_last_crypto()[0]: the own-pixel cryptomatte kernels (include/lentil_hip.h, LENTIL_CRYPTO_DIRECT_*)
CRYPTO_DIRECT_ATOMIC, CRYPTO_DIRECT_OWNER, CRYPTO_DIRECT_TILE = 1, 2, 3
CRYPTO_FLAGS_FROM_WORK, CRYPTO_WIPE_FLUSHED = 1, 2          # ... [3]'s bits

_lib = None


def process_stats():
    """(streamed passes begun, passes that hit the stuck time-out, ... of which injected, passes wiped and run again) -- all contexts of this process"""
    lib = load_library()
    n = (C.c_uint64 * 4)()
    rc = lib.lentil_hip_process_stats(n)
    if rc:
        raise RuntimeError("lentil_hip_process_stats: %d" % rc)
    return tuple(int(x) for x in n)


def process_stall_notes():
    """the redo notes of this process's passes that hit the stuck time-out unasked (lentil_hip_process_stall_notes)"""
    lib = load_library()
    buf = C.create_string_buffer(1 << 14)
    lib.lentil_hip_process_stall_notes(buf, 1 << 14)
    return buf.value.decode(errors="replace")


def _tea8(v0, v1):
    """tea<8> (src/global.h:32-57) on uint32 arrays"""
    v0 = np.asarray(v0, np.uint32).copy()
    v1 = np.broadcast_to(np.asarray(v1, np.uint32), v0.shape).copy()
    s0 = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(8):
            s0 = np.uint32((int(s0) + 0x9E3779B9) & 0xFFFFFFFF)
            v0 += ((v1 << np.uint32(4)) + np.uint32(0xA341316C)) ^ (v1 + s0) ^ ((v1 >> np.uint32(5)) + np.uint32(0xC8013EA4))
            v1 += ((v0 << np.uint32(4)) + np.uint32(0xAD90777D)) ^ (v0 + s0) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7E95761E))
    return v0


def ray_rng_state(ray_id, seed):
    """The xor128 state (uint32 [..., 4]) lentil_hip_camera_rays starts ray `ray_id` from: w0 = tea8(id, seed), w1 = tea8(id, w0),
    w2 = tea8(id, w1), w3 = tea8(id, w2); the generator's initial constants where all four are zero."""
    rid = np.asarray(ray_id, np.uint32)
    w = [_tea8(rid, np.uint32(int(seed) & 0xFFFFFFFF))]
    for _ in range(3):
        w.append(_tea8(rid, w[-1]))
    st = np.stack(w, -1)
    st[~st.any(-1)] = np.array([123456789, 362436069, 521288629, 88675123], np.uint32)
    return st


class LentilError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lentil_hip error %d: %s" % (code, msg))
        self.code = code


def load_library():
    """dlopen liblentil_hip.so; raises if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as
    # /opt/rocm's).  If torch is going to be used in this process (device memory, RCCL) it must be
    # loaded first so that this library binds to the runtime torch uses; loading /opt/rocm's runtime
    # first leaves torch without a visible GPU.
    if os.environ.get("LENTIL_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "lentil_hip_abi_version": (i, []),
        "lentil_hip_create": (i, [i, C.POINTER(vp)]),
        "lentil_hip_destroy": (i, [vp]),
        "lentil_hip_last_error": (C.c_char_p, [vp]),
        "lentil_hip_last_redo_note": (C.c_char_p, [vp]),
        "lentil_hip_set_params": (i, [vp, C.POINTER(_abi.Params)]),
        "lentil_hip_set_lens": (i, [vp, C.POINTER(_abi.LensTable)]),
        "lentil_hip_set_bokeh": (i, [vp, C.POINTER(_abi.BokehTable)]),
        "lentil_hip_alloc_frame": (i, [vp, u32, vp]),
        "lentil_hip_set_camera_motion": (i, [vp, u32, vp]),
        "lentil_hip_set_camera_shutter": (i, [vp, C.c_float, C.c_float]),
        "lentil_hip_upload_visits": (i, [vp, C.POINTER(_abi.Visits)]),
        "lentil_hip_bind_visits": (i, [vp, C.POINTER(_abi.Visits)]),
        "lentil_hip_clear_frame": (i, [vp]),
        "lentil_hip_redistribute": (i, [vp]),
        "lentil_hip_resolve": (i, [vp]),
        "lentil_hip_sync": (i, [vp]),
        "lentil_hip_download_aov": (i, [vp, u32, vp]),
        "lentil_hip_download_accum": (i, [vp, u32, vp, vp]),
        "lentil_hip_download_records": (i, [vp, vp, u64, C.POINTER(u32)]),
        "lentil_hip_accum_buffer": (i, [vp, C.POINTER(vp), C.POINTER(u64)]),
        "lentil_hip_stream": (i, [vp, C.POINTER(vp)]),
        "lentil_hip_set_closest_exchange": (i, [vp, i, u32]),
        "lentil_hip_zkey_buffer": (i, [vp, C.POINTER(vp), C.POINTER(u64)]),
        "lentil_hip_closest_gather": (i, [vp]),
        "lentil_hip_touched_rows": (i, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "lentil_hip_merge_rows": (i, [vp, u32, u32, vp, vp]),
        "lentil_hip_pack_rows": (i, [vp, u32, u32, vp]),
        "lentil_hip_merge_packed_rows": (i, [vp, u32, u32, vp, vp]),
        "lentil_hip_compact_rows": (i, [vp, u32, u32, vp, vp, vp, u32, C.POINTER(u32)]),
        "lentil_hip_merge_sparse": (i, [vp, u32, u32, u32, vp, vp, vp]),
        "lentil_hip_resolve_rows": (i, [vp, u32, u32]),
        "lentil_hip_get_counters": (i, [vp, C.POINTER(_abi.Counters)]),
        "lentil_hip_last_timing": (i, [vp, C.POINTER(C.c_float)]),
        "lentil_hip_last_launches": (i, [vp, C.POINTER(C.c_uint32)]),
        "lentil_hip_debug_last_scan": (i, [vp, C.POINTER(C.c_uint32)]),
        "lentil_hip_debug_last_crypto": (i, [vp, C.POINTER(C.c_uint32)]),
        "lentil_hip_batch_model_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "lentil_hip_process_stats": (i, [C.POINTER(C.c_uint64)]),
        "lentil_hip_process_stall_notes": (i, [C.c_char_p, C.c_uint64]),
        "lentil_hip_set_async": (i, [vp, i]),
        "lentil_hip_set_occlusion_probe": (i, [vp, vp, vp, vp]),
        "lentil_hip_probe_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "lentil_hip_set_occlusion_probe_device": (i, [vp, vp, vp, vp]),
        "lentil_hip_probe_device_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "lentil_hip_test_sphere_occluder_device": (i, [vp, vp, u32, vp, vp, vp]),
        "lentil_hip_pass_totals": (i, [vp, C.POINTER(_abi.PassTotals), i]),
        "lentil_hip_box_probe": (i, [vp, C.POINTER(C.c_double)]),
        "lentil_hip_lens_jit_status": (i, [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
        "lentil_hip_lens_jit_wait": (i, [vp, C.c_double]),
        "lentil_hip_debug_lens_jit_compile": (i, [vp, i, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64,
                                                  C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "lentil_hip_debug_lens_jit_source": (i, [vp, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "lentil_hip_debug_batch_estimate": (i, [vp, C.c_uint64, vp, C.c_uint32, vp]),
        "lentil_hip_alloc_crypto": (i, [vp, u32, u32]),
        "lentil_hip_upload_crypto": (i, [vp, C.POINTER(_abi.CryptoVisits)]),
        "lentil_hip_bind_crypto": (i, [vp, C.POINTER(_abi.CryptoVisits)]),
        "lentil_hip_download_crypto": (i, [vp, u32, u32, vp, vp]),
        "lentil_hip_visits_begin_crypto": (i, [vp, u32]),
        "lentil_hip_visits_append_crypto": (i, [vp, C.POINTER(_abi.Visits), C.POINTER(_abi.CryptoVisits), C.POINTER(u64)]),
        "lentil_hip_download_crypto_table": (i, [vp, u32, C.POINTER(u32), vp, vp, vp]),
        "lentil_hip_set_draw_log": (i, [vp, u64]),
        "lentil_hip_download_draw_log": (i, [vp, vp, u64, C.POINTER(u64)]),
        "lentil_hip_test_lt_sample_aperture": (i, [vp, u64, vp, vp, C.c_double, vp, vp, vp]),
        "lentil_hip_test_trace_bw_po": (i, [vp, u64, vp, vp, vp, vp, vp, vp]),
        "lentil_hip_test_aperture_sample": (i, [vp, u64, vp, vp, vp]),
        "lentil_hip_lens_is_compiled": (i, [vp]),
        "lentil_hip_set_lens_mode": (i, [vp, i]),
        "lentil_hip_focus_search": (i, [vp, C.c_double, C.c_double, C.POINTER(C.c_double)]),
        "lentil_hip_camera_rays": (i, [vp, C.POINTER(_abi.CameraRayBatch)]),
        "lentil_hip_camera_rays_path": (i, [vp, C.POINTER(C.c_int)]),
        "lentil_hip_trace_points": (i, [vp, C.POINTER(_abi.PointBatch)]),
        "lentil_hip_trace_points_path": (i, [vp, C.POINTER(C.c_int)]),
        "lentil_hip_camera_rays_spectral": (i, [vp, C.POINTER(_abi.CameraRayBatch), vp]),
        "lentil_hip_trace_points_spectral": (i, [vp, C.POINTER(_abi.PointBatch), vp]),
        "lentil_hip_trace_points_probed": (i, [vp, C.POINTER(_abi.PointBatch), C.POINTER(_abi.PointProbe)]),
        "lentil_hip_plan_visits": (i, [vp, u64, u64, vp, C.c_uint32, C.POINTER(u64)]),
        "lentil_hip_list_draws": (i, [vp, C.POINTER(_abi.DrawList)]),
        "lentil_hip_list_draws_spectral": (i, [vp, C.POINTER(_abi.DrawList), vp]),
        "lentil_hip_list_draws_path": (i, [vp, C.POINTER(C.c_int)]),
        "lentil_hip_set_visit_lambdas": (i, [vp, vp, u64, u32]),
        "lentil_hip_spectral_pass_stats": (i, [vp, C.POINTER(u64)]),
        "lentil_hip_draw_channels": (i, [C.POINTER(_abi.Params), C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(C.c_float)]),
        "lentil_hip_set_xor128_state": (i, [vp, C.POINTER(C.c_uint32)]),
        "lentil_hip_get_xor128_state": (i, [vp, C.POINTER(C.c_uint32)]),
        "lentil_hip_tl_chroma_stats": (i, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "lentil_hip_test_xor128_jump": (i, [C.POINTER(C.c_uint32), u64, C.POINTER(C.c_uint32)]),
        "lentil_hip_test_y0_intersection": (i, [vp, u64, vp, C.c_double, vp, vp, vp]),
        "lentil_hip_host_alloc": (i, [C.POINTER(vp), u64]),
        "lentil_hip_host_free": (i, [vp]),
        "lentil_hip_visits_begin": (i, [vp, C.POINTER(_abi.Visits), u64]),
        "lentil_hip_visits_append": (i, [vp, C.POINTER(_abi.Visits), C.POINTER(u64)]),
        "lentil_hip_visits_wait": (i, [vp, u64]),
        "lentil_hip_visits_end": (i, [vp, C.POINTER(u64)]),
        "lentil_hip_comm_unique_id": (i, [vp]),
        "lentil_hip_comm_init": (i, [vp, vp, i, i]),
        "lentil_hip_comm_destroy": (i, [vp]),
        "lentil_hip_allreduce": (i, [vp]),
        "lentil_hip_exchange_bands": (i, [vp, vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "lentil_hip_exchange_stats": (i, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "lentil_hip_exchange_counts": (i, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "lentil_hip_degenerate_stats": (i, [vp, C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "lentil_hip_streams_concurrent": (i, [vp, C.POINTER(C.c_int)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.lentil_hip_abi_version() != 1:
        raise RuntimeError("liblentil_hip.so ABI version mismatch")
    _lib = lib
    return lib


def draw_channels(p):
    """The colour channels the draw loop of these parameters traces per attempt (lentil_hip_draw_channels; no context, no GPU)
    -> (n_channels, lambda: float64 [3], micrometres, rgb_weight: float32 [3, 3], channel x colour component)."""
    import numpy as np
    n = C.c_uint32()
    lam = (C.c_double * 3)()
    w = (C.c_float * 9)()
    rc = load_library().lentil_hip_draw_channels(C.byref(p), C.byref(n), lam, w)
    if rc != _abi.OK:
        raise LentilError(rc, "lentil_hip_draw_channels")
    return int(n.value), np.array(lam[:], np.float64), np.array(w[:], np.float32).reshape(3, 3)


def sphere_occluder_device():
    """address of lentil_hip_test_sphere_occluder_device, the library's analytic lentil_probe_device_fn: user -> four host
    floats (centre, radius)"""
    return C.cast(load_library().lentil_hip_test_sphere_occluder_device, C.c_void_p).value


def host_alloc(nbytes):
    """Page-locked host memory from the library (lentil_hip_host_alloc) as a ctypes char array; free with host_free."""
    p = C.c_void_p()
    rc = load_library().lentil_hip_host_alloc(C.byref(p), nbytes)
    if rc:
        raise LentilError(rc, "lentil_hip_host_alloc(%d)" % nbytes)
    return p.value


def host_free(ptr):
    load_library().lentil_hip_host_free(C.c_void_p(ptr))


def make_crypto_visits(hashes, weights, ptr=lambda a: a.ctypes.data):
    """lentil_crypto_visits from per-AOV lists of [n, entries] fp32 arrays.  Returns (CryptoVisits, keepalive)."""
    c = _abi.CryptoVisits()
    c.n_crypto = len(hashes)
    c.n, c.entries = hashes[0].shape
    keep = []
    for a, (h, w) in enumerate(zip(hashes, weights)):
        assert h.shape == w.shape == (c.n, c.entries)
        c.hash[a] = ptr(h)
        c.weight[a] = ptr(w)
        keep += [h, w]
    return c, keep


def make_visits(cols, visits_per_pixel=0, pixels_per_row=0, pixel_x0=0, pixel_y0=0, pixel_row_stride=1,
                ptr=lambda a: a.ctypes.data):
    """Fill a lentil_visits from a dict of columns (numpy arrays, or anything `ptr` understands).

    cols: rgba, pos_z, raydir_time, volume_ignore, transmission [n,4] fp32; optional extra (list),
    pixel (uint32 [n]), inv_density (fp32 [n]).  Returns (Visits, keepalive)."""
    v = _abi.Visits()
    n = int(cols["rgba"].shape[0])
    v.n = n
    v.visits_per_pixel = visits_per_pixel
    v.pixels_per_row = pixels_per_row
    v.pixel_x0, v.pixel_y0 = pixel_x0, pixel_y0
    v.pixel_row_stride = pixel_row_stride
    extra = list(cols.get("extra", []))
    v.n_extra = len(extra)
    for name in ("rgba", "pos_z", "raydir_time", "volume_ignore", "transmission"):
        setattr(v, name, ptr(cols[name]) if n else None)
    for k, e in enumerate(extra):
        v.extra[k] = ptr(e) if (n and e is not None) else None      # None: an AOV without a column (lentil_debug)
    if cols.get("pixel") is not None:
        v.pixel = ptr(cols["pixel"])
    if cols.get("inv_density") is not None:
        v.inv_density = ptr(cols["inv_density"])
    return v, cols


def lens_jit_compile(table, compile=True):
    """(rc, emitted source, compiler log, seconds, code bytes) -- no context, no GPU (lentil_hip_debug_lens_jit_compile)"""
    lib = load_library()
    n = C.c_uint64(0)
    lib.lentil_hip_debug_lens_jit_compile(C.byref(table), 0, None, 0, C.byref(n), None, 0, None, None)
    src = C.create_string_buffer(int(n.value) + 1)
    log = C.create_string_buffer(1 << 16)
    sec, nb = C.c_double(0.0), C.c_uint64(0)
    rc = lib.lentil_hip_debug_lens_jit_compile(C.byref(table), 1 if compile else 0, src, int(n.value) + 1, None, log, 1 << 16, C.byref(sec), C.byref(nb))
    return int(rc), src.value.decode(), log.value.decode(errors="replace"), float(sec.value), int(nb.value)


_LAMBDAS_PER = {"camera_rays": "ray", "trace_points": "point", "list_draws": "visit", "set_visit_lambdas": "visit"}


def _lambdas_arg(call, lambdas, n, device):
    """The lambdas argument of the spectral calls, checked against the call's other arrays: n entries of float64, and of their
    kind -- device None: they are numpy (host pointers), so lambdas is a numpy float64 array (or a plain sequence); else they
    are torch tensors on GPU `device`, so lambdas is a contiguous float64 tensor there.  -> (the array to keep alive, its
    pointer).  ValueError otherwise: a numpy array handed over as device memory, or the reverse, would be read as what it is
    not."""
    is_tensor = hasattr(lambdas, "data_ptr") and not isinstance(lambdas, np.ndarray)
    if device is None:
        if is_tensor:
            raise ValueError("%s: lambdas is a tensor, the other arrays are numpy" % call)
        if isinstance(lambdas, np.ndarray) and lambdas.dtype != np.float64:
            raise ValueError("%s: lambdas must be float64, not %s" % (call, lambdas.dtype))
        lam = np.ascontiguousarray(lambdas, np.float64)
        if lam.shape != (n,):
            raise ValueError("%s: lambdas must be [%d], one per %s" % (call, n, _LAMBDAS_PER[call]))
        return lam, lam.ctypes.data
    import torch
    if not is_tensor:
        raise ValueError("%s: lambdas is not a tensor, the other arrays are" % call)
    if lambdas.dtype != torch.float64:
        raise ValueError("%s: lambdas must be float64, not %s" % (call, lambdas.dtype))
    if not lambdas.is_cuda or lambdas.device.index != device:
        raise ValueError("%s: lambdas is on %s, the context on GPU %d" % (call, lambdas.device, device))
    if not lambdas.is_contiguous():
        raise ValueError("%s: lambdas must be contiguous" % call)
    if tuple(lambdas.shape) != (n,):
        raise ValueError("%s: lambdas must be [%d], one per %s" % (call, n, _LAMBDAS_PER[call]))
    return lambdas, lambdas.data_ptr()


class Context:
    """One lentil_hip_ctx: one GPU, one stream (mirrors the ownership of the reference's Camera)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.device = int(device)
        rc = self.lib.lentil_hip_create(device, C.byref(self.h))
        if rc:
            raise LentilError(rc, (self.lib.lentil_hip_last_error(None) or b"").decode())
        self.params = None
        self.n_aovs = 0
        self._keep = {}

    def _chk(self, rc):
        if rc:
            raise LentilError(rc, (self.lib.lentil_hip_last_error(self.h) or b"").decode())

    def close(self):
        if self.h:
            self.lib.lentil_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- setup
    def set_params(self, params):
        self._chk(self.lib.lentil_hip_set_params(self.h, C.byref(params)))
        self.params = params

    def set_lens(self, table):
        self._chk(self.lib.lentil_hip_set_lens(self.h, C.byref(table)))

    def lens_is_compiled(self):
        return bool(self.lib.lentil_hip_lens_is_compiled(self.h))

    def set_lens_mode(self, mode):
        """0 = compiled-in kernel when the table is a shipped lens, 1 = always the table interpreter (passes, camera rays and
        the focus search)."""
        self._chk(self.lib.lentil_hip_set_lens_mode(self.h, mode))

    def set_bokeh(self, tables):
        """tables: dict with x, y, cdfRow, rowIndices, cdfColumn, columnIndices (numpy) or None."""
        if tables is None:
            self._chk(self.lib.lentil_hip_set_bokeh(self.h, None))
            return
        b = _abi.BokehTable()
        b.x, b.y = int(tables["x"]), int(tables["y"])
        arrs = {k: np.ascontiguousarray(tables[k]) for k in ("cdfRow", "rowIndices", "cdfColumn", "columnIndices")}
        assert arrs["cdfRow"].dtype == np.float32 and arrs["rowIndices"].dtype == np.int32
        assert arrs["cdfColumn"].dtype == np.float32 and arrs["columnIndices"].dtype == np.int32
        for k, a in arrs.items():
            setattr(b, k, a.ctypes.data)
        self._chk(self.lib.lentil_hip_set_bokeh(self.h, C.byref(b)))

    def alloc_frame(self, n_aovs=1, kinds=None):
        k = (C.c_uint8 * n_aovs)(*(kinds or [0] * n_aovs))
        self._chk(self.lib.lentil_hip_alloc_frame(self.h, n_aovs, C.cast(k, C.c_void_p)))
        self.n_aovs = n_aovs

    # --- visits
    def set_camera_shutter(self, start, end):
        """the absolute times of the first and the last camera matrix key (Arnold's shutter_start / shutter_end); 0 ... 1 until set"""
        self._chk(self.lib.lentil_hip_set_camera_shutter(self.h, float(start), float(end)))

    def set_camera_motion(self, keys):
        """[n, 4, 4] world-to-camera matrices at equidistant times over the shutter (None / one key: the static matrix)"""
        if keys is None:
            self._chk(self.lib.lentil_hip_set_camera_motion(self.h, 0, None))
            return
        k = np.ascontiguousarray(keys, np.float32)
        self._chk(self.lib.lentil_hip_set_camera_motion(self.h, k.shape[0], k.ctypes.data))

    def upload_visits(self, visits):
        self._chk(self.lib.lentil_hip_upload_visits(self.h, C.byref(visits)))

    def bind_visits(self, visits, keepalive=None):
        self._chk(self.lib.lentil_hip_bind_visits(self.h, C.byref(visits)))
        self._keep["visits"] = keepalive

    # --- hot path
    def clear_frame(self):
        self._chk(self.lib.lentil_hip_clear_frame(self.h))

    def redistribute(self):
        self._chk(self.lib.lentil_hip_redistribute(self.h))

    def resolve(self):
        self._chk(self.lib.lentil_hip_resolve(self.h))

    def sync(self):
        self._chk(self.lib.lentil_hip_sync(self.h))

    # --- results
    @property
    def n_pixels(self):
        return int(self.params.xres) * int(self.params.yres)

    def download_aov(self, aov=0):
        out = np.empty((self.n_pixels, 4), np.float32)
        self._chk(self.lib.lentil_hip_download_aov(self.h, aov, out.ctypes.data))
        return out

    def download_accum(self, aov=0):
        buf = np.empty((self.n_pixels, 4), np.float32)
        w = np.empty((self.n_pixels,), np.float32)
        self._chk(self.lib.lentil_hip_download_accum(self.h, aov, buf.ctypes.data, w.ctypes.data))
        return buf, w

    def download_records(self):
        """[n_pixels, stride] fp32: every AOV's accumulators (floats 4a .. 4a+3) and the weight (float 4 * n_aovs) in one copy"""
        st = C.c_uint32(0)
        self._chk(self.lib.lentil_hip_download_records(self.h, None, 0, C.byref(st)))
        rec = np.empty((self.n_pixels, int(st.value)), np.float32)
        self._chk(self.lib.lentil_hip_download_records(self.h, rec.ctypes.data, rec.size, C.byref(st)))
        return rec

    def accum_buffer(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.lentil_hip_accum_buffer(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_closest_exchange(self, deferred, visit_id_base=0):
        self._chk(self.lib.lentil_hip_set_closest_exchange(self.h, 1 if deferred else 0, visit_id_base))

    def zkey_buffer(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.lentil_hip_zkey_buffer(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def closest_gather(self):
        self._chk(self.lib.lentil_hip_closest_gather(self.h))

    def set_xor128_state(self, state):
        self._chk(self.lib.lentil_hip_set_xor128_state(self.h, (C.c_uint32 * 4)(*[int(x) for x in state])))

    def get_xor128_state(self):
        st = (C.c_uint32 * 4)()
        self._chk(self.lib.lentil_hip_get_xor128_state(self.h, st))
        return list(st)

    def tl_chroma_stats(self):
        """(items, dependent items, bytes received from other ranks) of the last thin-lens abb_chromatic > 0 pass
        (lentil_hip_tl_chroma_stats)"""
        n = [C.c_uint64() for _ in range(3)]
        self._chk(self.lib.lentil_hip_tl_chroma_stats(self.h, *[C.byref(x) for x in n]))
        return tuple(int(x.value) for x in n)

    def test_xor128_jump(self, state, k):
        """xor128 state advanced by k outputs, by the device jump-ahead (lentil_hip_test_xor128_jump)"""
        out = (C.c_uint32 * 4)()
        self._chk(self.lib.lentil_hip_test_xor128_jump((C.c_uint32 * 4)(*[int(x) for x in state]), int(k), out))
        return list(out)

    def focus_search(self, focal_distance, lam):
        best = C.c_double()
        self._chk(self.lib.lentil_hip_focus_search(self.h, focal_distance, lam, C.byref(best)))
        return best.value

    def camera_rays(self, inp, first_ray=0, lam=0.55, exposure=1.0, seed=0, differentials=True, want_tries=False, lambdas=None):
        """Forward camera rays in a batch (lentil_hip_camera_rays): camera_create_ray for every row of inp, fp32 [n, 6] =
        sx, sy, dsx, dsy, lensx, lensy -> fp32 [n, 21] = origin, dir, weight, dOdx, dOdy, dDdx, dDdy (and, want_tries, int32
        [n]: the vignetted tries of each ray's own trace).  Ray i draws its retries from its own xor128 state, the four
        words ray_rng_state(first_ray + i, seed) -- the same whatever batch the ray is part of.
        numpy in: host pointers, numpy out, complete on return.  A contiguous torch tensor on this context's device: device
        pointers, torch tensors out, enqueued on the context's stream (stream()) without waiting.  The caller orders both ends:
        whatever produced inp must be complete on, or ordered before, the context's stream; sync() or the stream orders the
        results; and inp and the returned tensors must stay alive until the stream has passed the call.
        lambdas: float64 [n], micrometres, of inp's kind (numpy with numpy, a contiguous tensor on the same GPU with a tensor;
        it stays alive like inp): ray i at lambdas[i] instead of every ray at lam (lentil_hip_camera_rays_spectral)."""
        flags = 0 if differentials else _abi.RAYS_NO_DIFFERENTIALS
        b = _abi.CameraRayBatch()
        if isinstance(inp, np.ndarray) or not hasattr(inp, "data_ptr"):
            a = np.ascontiguousarray(inp, np.float32)
            if a.ndim != 2 or a.shape[1] != _abi.RAY_IN_FLOATS:
                raise ValueError("camera_rays: inp must be [n, 6]")
            n = a.shape[0]
            out = np.empty((n, _abi.RAY_OUT_FLOATS), np.float32)
            tries = np.empty((n,), np.int32) if want_tries else None
            ptrs = (a.ctypes.data, out.ctypes.data, tries.ctypes.data if want_tries else None)
            kind = None
        else:
            import torch
            if inp.dtype != torch.float32 or inp.dim() != 2 or inp.shape[1] != _abi.RAY_IN_FLOATS:
                raise ValueError("camera_rays: inp must be a float32 [n, 6] tensor")
            if not inp.is_cuda or inp.device.index != self.device:
                raise ValueError("camera_rays: inp is on %s, the context on GPU %d" % (inp.device, self.device))
            if not inp.is_contiguous():      # (a copy here would run on torch's stream, unordered with the context's)
                raise ValueError("camera_rays: inp must be contiguous")
            a = inp
            n = a.shape[0]
            out = torch.empty((n, _abi.RAY_OUT_FLOATS), dtype=torch.float32, device=a.device)
            tries = torch.empty((n,), dtype=torch.int32, device=a.device) if want_tries else None
            ptrs = (a.data_ptr(), out.data_ptr(), tries.data_ptr() if want_tries else None)
            flags |= _abi.RAYS_DEVICE_POINTERS
            kind = self.device
        if lambdas is not None:
            lambdas, lam_ptr = _lambdas_arg("camera_rays", lambdas, n, kind)
        b.n, b.first_ray = n, int(first_ray)
        b.inp, b.out, b.tries = (p if n else None for p in ptrs)
        b.lam, b.exposure, b.rng_seed, b.flags = float(lam), float(exposure), int(seed) & 0xFFFFFFFF, flags
        if lambdas is not None:
            self._chk(self.lib.lentil_hip_camera_rays_spectral(self.h, C.byref(b), lam_ptr if n else None))
        else:
            self._chk(self.lib.lentil_hip_camera_rays(self.h, C.byref(b)))
        return (out, tries) if want_tries else out

    def camera_rays_path(self):
        """What the last camera_rays call ran: one of _abi.RAYS_PATH_* (lentil_hip_camera_rays_path).  The compiled paths need
        LENTIL_RAYS_COMPILED=1 in the environment when the context is created; the default is the interpreter."""
        path = C.c_int()
        self._chk(self.lib.lentil_hip_camera_rays_path(self.h, C.byref(path)))
        return path.value

    def trace_points(self, cs, pixel, attempts, first_attempt=None, lam=0.0, want_xy=True, want_sensor=False, want_tries=False,
                     lambdas=None):
        """Scene points traced backward through the lens in a batch (lentil_hip_trace_points): for every point (cs fp32 [n, 3],
        camera space, cm; pixel uint32 [n] = px | py << 16, the source pixel that seeds the draws) and every attempt
        first_attempt[point] ... + attempts - 1 (uint32 [n]; None: from 0), where a draw of the pass puts it.
        -> a dict: "pixel" uint32 [n, attempts] (the linear pixel, _abi.POINT_VIGNETTED or _abi.POINT_OUTSIDE; a torch tensor holds the
        same bits as int32: the two codes read -1 and -2) and, as asked for,
        "xy" fp64 [n, attempts, 2] (continuous pixel coordinates, NaN where vignetted), "sensor" fp64 [n, attempts, 2]
        (polynomial optics: mm on the sensor) and "tries" int32 [n, attempts].  lam: micrometres, 0 = params.lambda_bw.
        numpy in: host pointers, numpy out, complete on return.  Contiguous torch tensors on this context's device: device
        pointers, torch tensors out, enqueued on the context's stream (stream()) without waiting; the caller orders both ends as
        for camera_rays, and with device pointers the seeds first_attempt + attempts + vignetting_retries must fit 32 bits.
        lambdas: float64 [n], micrometres, 0 = params.lambda_bw, of cs's kind (numpy with numpy, a contiguous tensor on the same
        GPU with tensors): point j at lambdas[j] instead of every point at lam (lentil_hip_trace_points_spectral)."""
        b = _abi.PointBatch()
        attempts = int(attempts)
        if isinstance(cs, np.ndarray) or not hasattr(cs, "data_ptr"):
            a = np.ascontiguousarray(cs, np.float32)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("trace_points: cs must be [n, 3]")
            n = a.shape[0]
            px = np.ascontiguousarray(pixel, np.uint32)
            fa = None if first_attempt is None else np.ascontiguousarray(first_attempt, np.uint32)
            if px.shape != (n,) or (fa is not None and fa.shape != (n,)):
                raise ValueError("trace_points: pixel and first_attempt must be [n]")
            k = max(attempts, 0)
            out = {"pixel": np.empty((n, k), np.uint32)}
            if want_xy:
                out["xy"] = np.empty((n, k, 2), np.float64)
            if want_sensor:
                out["sensor"] = np.empty((n, k, 2), np.float64)
            if want_tries:
                out["tries"] = np.empty((n, k), np.int32)
            ptr = lambda t: None if t is None else t.ctypes.data      # noqa: E731
            flags, kind = 0, None
        else:
            import torch
            if cs.dtype != torch.float32 or cs.dim() != 2 or cs.shape[1] != 3:
                raise ValueError("trace_points: cs must be a float32 [n, 3] tensor")
            n = cs.shape[0]
            a, px, fa = cs, pixel, first_attempt
            for name, t in (("cs", a), ("pixel", px), ("first_attempt", fa)):
                if t is None:
                    continue
                if not t.is_cuda or t.device.index != self.device:
                    raise ValueError("trace_points: %s is on %s, the context on GPU %d" % (name, t.device, self.device))
                if not t.is_contiguous():      # (a copy here would run on torch's stream, unordered with the context's)
                    raise ValueError("trace_points: %s must be contiguous" % name)
                if t is not a and (t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or tuple(t.shape) != (n,)):
                    raise ValueError("trace_points: %s must be a 32-bit integer [n] tensor" % name)
            k = max(attempts, 0)
            out = {"pixel": torch.empty((n, k), dtype=torch.int32, device=a.device)}      # (the bits of a uint32)
            if want_xy:
                out["xy"] = torch.empty((n, k, 2), dtype=torch.float64, device=a.device)
            if want_sensor:
                out["sensor"] = torch.empty((n, k, 2), dtype=torch.float64, device=a.device)
            if want_tries:
                out["tries"] = torch.empty((n, k), dtype=torch.int32, device=a.device)
            ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
            flags, kind = _abi.POINTS_DEVICE_POINTERS, self.device
        if lambdas is not None:
            lambdas, lam_ptr = _lambdas_arg("trace_points", lambdas, n, kind)
        b.n_points, b.attempts, b.flags, b.lam = n, attempts & 0xFFFFFFFF, flags, float(lam)
        if n:
            b.cs, b.pixel, b.first_attempt = ptr(a), ptr(px), ptr(fa)
            b.out_pixel, b.out_xy, b.out_sensor, b.out_tries = (ptr(out.get(key)) for key in ("pixel", "xy", "sensor", "tries"))
        if lambdas is not None:
            self._chk(self.lib.lentil_hip_trace_points_spectral(self.h, C.byref(b), lam_ptr if n else None))
        else:
            self._chk(self.lib.lentil_hip_trace_points(self.h, C.byref(b)))
        return out

    def trace_points_path(self):
        """What the last trace_points call ran: one of _abi.POINTS_PATH_* (lentil_hip_trace_points_path)."""
        path = C.c_int()
        self._chk(self.lib.lentil_hip_trace_points_path(self.h, C.byref(path)))
        return path.value

    def trace_points_probed(self, cs, pixel, attempts, origin, first_attempt=None, time=None, exempt=None, lam=0.0, lambdas=None,
                            want_xy=True, want_sensor=False, want_tries=True):
        """trace_points under the context's occlusion probe (lentil_hip_trace_points_probed): a try whose segment from
        origin[point] (float32 [n, 3], world space) to the try's aperture point is occluded fails like one the lens vignettes.
        time: float32 [n], the samples' times (None: 0); exempt: uint8 [n], non-zero = supplied by the skydome, never occluded
        and never asked about (None: no point); lambdas: float64 [n], a wavelength per point (None: lam for all).  The other
        arguments and the dict that comes back are trace_points'.  numpy arrays: host pointers; contiguous torch tensors on
        this context's device: device pointers, torch tensors out (the caller orders the inputs before the context's stream, as
        for trace_points) -- either way the outputs are final on return.  Every array is of cs's kind; ValueError before any
        call otherwise."""
        b, pp = _abi.PointBatch(), _abi.PointProbe()
        attempts = int(attempts)
        extra = (("origin", origin), ("time", time), ("exempt", exempt))
        if isinstance(cs, np.ndarray) or not hasattr(cs, "data_ptr"):
            for name, t in (("pixel", pixel), ("first_attempt", first_attempt)) + extra:
                if hasattr(t, "data_ptr") and not isinstance(t, np.ndarray):
                    raise ValueError("trace_points_probed: %s is a tensor, cs is not" % name)
            if origin is None:
                raise ValueError("trace_points_probed: origin is required")
            a = np.ascontiguousarray(cs, np.float32)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("trace_points_probed: cs must be [n, 3]")
            n = a.shape[0]
            px = np.ascontiguousarray(pixel, np.uint32)
            fa = None if first_attempt is None else np.ascontiguousarray(first_attempt, np.uint32)
            if px.shape != (n,) or (fa is not None and fa.shape != (n,)):
                raise ValueError("trace_points_probed: pixel and first_attempt must be [n]")
            org = np.ascontiguousarray(origin, np.float32)
            if org.shape != (n, 3):
                raise ValueError("trace_points_probed: origin must be [n, 3]")
            tm = None if time is None else np.ascontiguousarray(time, np.float32)
            ex = None if exempt is None else np.ascontiguousarray(exempt, np.uint8)
            if (tm is not None and tm.shape != (n,)) or (ex is not None and ex.shape != (n,)):
                raise ValueError("trace_points_probed: time and exempt must be [n]")
            k = max(attempts, 0)
            out = {"pixel": np.empty((n, k), np.uint32)}
            if want_xy:
                out["xy"] = np.empty((n, k, 2), np.float64)
            if want_sensor:
                out["sensor"] = np.empty((n, k, 2), np.float64)
            if want_tries:
                out["tries"] = np.empty((n, k), np.int32)
            ptr = lambda t: None if t is None else t.ctypes.data      # noqa: E731
            flags, kind = 0, None
        else:
            import torch
            if cs.dtype != torch.float32 or cs.dim() != 2 or cs.shape[1] != 3:
                raise ValueError("trace_points_probed: cs must be a float32 [n, 3] tensor")
            n = cs.shape[0]
            if origin is None:
                raise ValueError("trace_points_probed: origin is required")
            a, px, fa, org, tm, ex = cs, pixel, first_attempt, origin, time, exempt
            ints = (torch.int32, getattr(torch, "uint32", torch.int32))
            want = {"cs": ((torch.float32,), (n, 3)), "pixel": (ints, (n,)), "first_attempt": (ints, (n,)), "origin": ((torch.float32,), (n, 3)),
                    "time": ((torch.float32,), (n,)), "exempt": ((torch.uint8,), (n,))}
            for name, t in (("cs", a), ("pixel", px), ("first_attempt", fa)) + extra:
                if t is None:
                    continue
                if not hasattr(t, "data_ptr") or isinstance(t, np.ndarray):
                    raise ValueError("trace_points_probed: %s is not a tensor, cs is" % name)
                if not t.is_cuda or t.device.index != self.device:
                    raise ValueError("trace_points_probed: %s is on %s, the context on GPU %d" % (name, t.device, self.device))
                if not t.is_contiguous():      # (a copy here would run on torch's stream, unordered with the context's)
                    raise ValueError("trace_points_probed: %s must be contiguous" % name)
                if t.dtype not in want[name][0] or tuple(t.shape) != want[name][1]:
                    raise ValueError("trace_points_probed: %s must be a %s %s tensor" % (name, want[name][0][0], list(want[name][1])))
            k = max(attempts, 0)
            out = {"pixel": torch.empty((n, k), dtype=torch.int32, device=a.device)}      # (the bits of a uint32)
            if want_xy:
                out["xy"] = torch.empty((n, k, 2), dtype=torch.float64, device=a.device)
            if want_sensor:
                out["sensor"] = torch.empty((n, k, 2), dtype=torch.float64, device=a.device)
            if want_tries:
                out["tries"] = torch.empty((n, k), dtype=torch.int32, device=a.device)
            ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
            flags, kind = _abi.POINTS_DEVICE_POINTERS, self.device
        lam_ptr = None
        if lambdas is not None:
            lambdas, lam_ptr = _lambdas_arg("trace_points", lambdas, n, kind)
        b.n_points, b.attempts, b.flags, b.lam = n, attempts & 0xFFFFFFFF, flags, float(lam)
        if n:
            b.cs, b.pixel, b.first_attempt = ptr(a), ptr(px), ptr(fa)
            b.out_pixel, b.out_xy, b.out_sensor, b.out_tries = (ptr(out.get(key)) for key in ("pixel", "xy", "sensor", "tries"))
            pp.origin, pp.time, pp.exempt, pp.lambdas = ptr(org), ptr(tm), ptr(ex), lam_ptr
        self._chk(self.lib.lentil_hip_trace_points_probed(self.h, C.byref(b), C.byref(pp)))
        return out

    def _visit_range(self, first, n):
        first = int(first)
        if n is None:
            n = max(int(self.counters().visits) - first, 0)
        return first, int(n)

    def _device_records(self, n):
        """n 32-byte records on this context's GPU, as a uint8 [n, 32] torch tensor"""
        import torch
        return torch.empty((n, 32), dtype=torch.uint8, device="cuda:%d" % self.device)

    def plan_visits(self, first=0, n=None, device=False, totals=True):
        """What the visit prologue decides for the bound visits first ... first + n - 1 (n None: to the stream's end)
        (lentil_hip_plan_visits) -> (records, totals): records a numpy array of _abi.VisitPlan, one per visit (cs, add_energy,
        weight, samples, pixel = px | py << 16, flags & _abi.PLAN_REDISTRIBUTE); totals (visits, redistributed visits, the sum of
        their samples -- an upper bound on what list_draws finds for the range), or None with totals=False.
        device=True: the records stay on the GPU, a uint8 [n, 32] torch tensor (.cpu().numpy().view(_abi.VisitPlan) reads it);
        with totals=False as well the call only enqueues on the context's stream (stream()), the caller orders it (sync())."""
        first, n = self._visit_range(first, n)
        tot = (C.c_uint64 * 3)() if totals else None
        if device:
            out = self._device_records(n)
            ptr, flags = (out.data_ptr() if n else None), _abi.PLAN_DEVICE_POINTERS
        else:
            out = np.empty(n, _abi.VisitPlan)
            ptr, flags = (out.ctypes.data if n else None), 0
        self._chk(self.lib.lentil_hip_plan_visits(self.h, first, n, ptr, flags, tot))
        return out, (tuple(int(t) for t in tot) if totals else None)

    def list_draws(self, first=0, n=None, capacity=None, lam=0.0, device=False, probed=False, channels=False, lambdas=None):
        """The accepted draws of the bound visits first ... first + n - 1 (lentil_hip_list_draws) -> (records, n_draws,
        attempts): records a numpy array of _abi.Draw (visit, attempt, pixel, tries, xy), in no particular order, the first
        min(n_draws, capacity) of it filled and returned; n_draws the accepted draws found (above capacity: ask again with more
        room); attempts the attempts made.  capacity None: sized from plan_visits' totals[2], which always suffices.
        lam: micrometres, 0 = params.lambda_bw.  device=True: the records stay on the GPU, a uint8 [capacity, 32] torch tensor,
        whole (the call returns when it is filled).  probed=True (_abi.DRAWS_PROBED): the list under the context's occlusion
        probe -- tries then counts occluded tries too, and the probe's callback is called once per turn, on this thread.
        channels=True (_abi.DRAWS_CHANNELS): the caller reads attempt as n | channel << 30 -- what polynomial optics with
        abb_chromatic != 0 need (up to three records per attempt, a channel's tries / xy / pixel its own); any other mode gives
        the plain list.  totals[2] does not bound that list, so capacity None then sizes it by a counting call (capacity 0).
        lambdas: float64 [n], micrometres, 0 = params.lambda_bw -- visit first + i at lambdas[i] instead of every visit at lam
        (lentil_hip_list_draws_spectral); numpy with device=False, a contiguous tensor on this context's GPU with device=True."""
        first, n = self._visit_range(first, n)
        flags = (_abi.DRAWS_PROBED if probed else 0) | (_abi.DRAWS_CHANNELS if channels else 0)
        if lambdas is not None:
            lambdas, lam_ptr = _lambdas_arg("list_draws", lambdas, n, self.device if device else None)
            call = lambda b: self.lib.lentil_hip_list_draws_spectral(self.h, C.byref(b), lam_ptr if n else None)      # noqa: E731
        else:
            call = lambda b: self.lib.lentil_hip_list_draws(self.h, C.byref(b))      # noqa: E731
        if capacity is None and channels and n:
            cnt = C.c_uint64()
            b = _abi.DrawList()
            b.first_visit, b.n_visits, b.capacity, b.lam, b.flags = first, n, 0, float(lam), flags
            if device and lambdas is not None:      # (no `out` here: the flag says where lambdas lie)
                b.flags |= _abi.DRAWS_DEVICE_POINTERS
            b.n_draws = C.pointer(cnt)
            self._chk(call(b))
            capacity = cnt.value
        elif capacity is None:
            capacity = self.plan_visits(first, n)[1][2] if n else 0
        capacity = int(capacity)
        nd, att = C.c_uint64(), C.c_uint64()
        b = _abi.DrawList()
        b.first_visit, b.n_visits, b.capacity, b.lam = first, n, capacity, float(lam)
        b.n_draws, b.attempts = C.pointer(nd), C.pointer(att)
        if device:
            out = self._device_records(capacity)
            b.out, b.flags = (out.data_ptr() if capacity else None), _abi.DRAWS_DEVICE_POINTERS
        else:
            out = np.empty(capacity, _abi.Draw)
            b.out, b.flags = (out.ctypes.data if capacity else None), 0
        b.flags |= flags
        self._chk(call(b))
        if not device:
            out = out[:min(nd.value, capacity)]
        return out, nd.value, att.value

    def list_draws_path(self):
        """What the last list_draws call ran: one of _abi.DRAWS_PATH_* (lentil_hip_list_draws_path)."""
        path = C.c_int()
        self._chk(self.lib.lentil_hip_list_draws_path(self.h, C.byref(path)))
        return path.value

    def test_y0_intersection(self, sensor_shift, lam):
        import numpy as np
        sh = np.ascontiguousarray(sensor_shift, np.float64)
        n = sh.shape[0]
        dist, sensor, out = np.empty(n), np.empty((n, 5)), np.empty((n, 5))
        self._chk(self.lib.lentil_hip_test_y0_intersection(self.h, n, sh.ctypes.data, lam, dist.ctypes.data,
                                                           sensor.ctypes.data, out.ctypes.data))
        return dist, sensor, out

    # --- the visit stream handed over piece by piece (include/lentil_hip.h "piece by piece")
    def visits_begin(self, layout, capacity_hint=0):
        self._chk(self.lib.lentil_hip_visits_begin(self.h, C.byref(layout), capacity_hint))

    def visits_append(self, part):
        t = C.c_uint64()
        self._chk(self.lib.lentil_hip_visits_append(self.h, C.byref(part), C.byref(t)))
        return t.value

    def visits_begin_crypto(self, entries):
        self._chk(self.lib.lentil_hip_visits_begin_crypto(self.h, entries))

    def visits_append_crypto(self, part, caches):
        t = C.c_uint64()
        self._chk(self.lib.lentil_hip_visits_append_crypto(self.h, C.byref(part), C.byref(caches), C.byref(t)))
        return t.value

    def visits_wait(self, ticket):
        self._chk(self.lib.lentil_hip_visits_wait(self.h, ticket))

    def visits_end(self):
        n = C.c_uint64()
        self._chk(self.lib.lentil_hip_visits_end(self.h, C.byref(n)))
        return n.value

    # --- the native exchange (RCCL inside the library; include/lentil_hip.h "multi-GPU, the exchange itself")
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        lib = load_library()
        rc = lib.lentil_hip_comm_unique_id(buf)
        if rc != 0:
            raise RuntimeError("lentil_hip_comm_unique_id: %s" % (lib.lentil_hip_last_error(None) or b"").decode())
        return bytes(buf)

    def comm_init(self, uid, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(self.lib.lentil_hip_comm_init(self.h, buf, rank, world))

    def comm_destroy(self):
        self._chk(self.lib.lentil_hip_comm_destroy(self.h))

    def allreduce(self):
        self._chk(self.lib.lentil_hip_allreduce(self.h))

    def exchange_bands(self, visit_rows, bounds=None, sparse=True):
        lo, hi = C.c_int32(), C.c_int32()
        b = None
        if bounds is not None:
            b = (C.c_int32 * len(bounds))(*[int(x) for x in bounds])
        self._chk(self.lib.lentil_hip_exchange_bands(self.h, b, int(visit_rows), 1 if sparse else 0,
                                                     C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def streams_concurrent(self):
        """0: the pass's four streams share hardware queues, 1: they run side by side, 2: and a spare one beside them"""
        v = C.c_int(0)
        self._chk(self.lib.lentil_hip_streams_concurrent(self.h, C.byref(v)))
        return int(v.value)

    def exchange_stats(self):
        """(bytes sent, bytes received) by this rank in its last exchange_bands / allreduce"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.lentil_hip_exchange_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def exchange_counts(self):
        """(exchange_bands calls that ran in the fixed-capacity form, directed pairs whose entries overflowed their message)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.lentil_hip_exchange_counts(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def degenerate_stats(self):
        """(degenerate, flagged pixels, nodes sent, nodes received, passes run again) of the last pass and the exchange behind
        it: closest-filtered candidates at depth 0 / NaN (lentil_hip_degenerate_stats)"""
        d = C.c_uint32()
        n = [C.c_uint64() for _ in range(4)]
        self._chk(self.lib.lentil_hip_degenerate_stats(self.h, C.byref(d), *[C.byref(x) for x in n]))
        return (int(d.value),) + tuple(int(x.value) for x in n)

    def touched_rows(self):
        lo, hi = C.c_int32(), C.c_int32()
        self._chk(self.lib.lentil_hip_touched_rows(self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def merge_rows(self, row_begin, n_rows, acc_ptr, key_ptr=None):
        self._chk(self.lib.lentil_hip_merge_rows(self.h, row_begin, n_rows, acc_ptr, key_ptr))

    def pack_rows(self, row_begin, n_rows, dst_ptr):
        self._chk(self.lib.lentil_hip_pack_rows(self.h, row_begin, n_rows, dst_ptr))

    def merge_packed_rows(self, row_begin, n_rows, packed_ptr, key_ptr=None):
        self._chk(self.lib.lentil_hip_merge_packed_rows(self.h, row_begin, n_rows, packed_ptr, key_ptr))

    def compact_rows(self, row_begin, n_rows, idx_ptr, vals_ptr, keys_ptr, capacity):
        n = C.c_uint32()
        self._chk(self.lib.lentil_hip_compact_rows(self.h, row_begin, n_rows, idx_ptr, vals_ptr, keys_ptr, capacity, C.byref(n)))
        return n.value

    def merge_sparse(self, row_begin, n_rows, n, idx_ptr, vals_ptr, keys_ptr=None):
        self._chk(self.lib.lentil_hip_merge_sparse(self.h, row_begin, n_rows, n, idx_ptr, vals_ptr, keys_ptr))

    def resolve_rows(self, row_begin, n_rows):
        self._chk(self.lib.lentil_hip_resolve_rows(self.h, row_begin, n_rows))

    def stream(self):
        s = C.c_void_p()
        self._chk(self.lib.lentil_hip_stream(self.h, C.byref(s)))
        return s.value

    def last_redo_note(self):
        """Why the last streamed pass that was redone the chunked way gave up ("" if none was)."""
        return (self.lib.lentil_hip_last_redo_note(self.h) or b"").decode()

    def counters(self):
        c = _abi.Counters()
        self._chk(self.lib.lentil_hip_get_counters(self.h, C.byref(c)))
        return c

    def set_occlusion_probe(self, fn, user=None, camera_to_world=None):
        """fn: address of a lentil_probe_fn (C function; None switches probing off); user: address handed back to it;
        camera_to_world: [4, 4] fp32 (row-vector convention) or None for the inverse of the world-to-camera matrix"""
        self._probe_keep = (np.ascontiguousarray(camera_to_world, np.float32) if camera_to_world is not None else None)
        self._chk(self.lib.lentil_hip_set_occlusion_probe(self.h, fn, user, self._probe_keep.ctypes.data if self._probe_keep is not None else None))

    def probe_stats(self):
        """(segments probed, of them occluded, callback calls) since the context was created"""
        n = (C.c_uint64 * 3)()
        self._chk(self.lib.lentil_hip_probe_stats(self.h, n))
        return tuple(int(x) for x in n)

    def set_occlusion_probe_device(self, fn, user=None, camera_to_world=None):
        """fn: address of a lentil_probe_device_fn, which enqueues the renderer's answers on the stream it is given (None switches
        probing off; replaces a host callback); user and camera_to_world as for set_occlusion_probe"""
        self._probe_keep = (np.ascontiguousarray(camera_to_world, np.float32) if camera_to_world is not None else None)
        self._chk(self.lib.lentil_hip_set_occlusion_probe_device(self.h, fn, user, self._probe_keep.ctypes.data if self._probe_keep is not None else None))

    def probe_device_stats(self):
        """(lists handed to the device callback, host waits made for such lists, lists that did not fit their buffers, the longest
        list) since the context was created"""
        n = (C.c_uint64 * 4)()
        self._chk(self.lib.lentil_hip_probe_device_stats(self.h, n))
        return tuple(int(x) for x in n)

    def set_visit_lambdas(self, lambdas=None, device=False):
        """a wavelength per visit of the bound stream for the pass (lentil_hip_set_visit_lambdas; micrometres, 0:
        params.lambda_bw), None: switched off.  device False: a numpy float64 array (or a plain sequence), copied by the
        library before the call returns; True: a contiguous float64 tensor on this context's GPU, bound -- the context keeps
        a reference, the caller leaves its content alone while a pass runs.  The column's length is its own: a pass over a
        stream of another number of visits refuses it."""
        if lambdas is None:
            self._lambdas_keep = None
            self._chk(self.lib.lentil_hip_set_visit_lambdas(self.h, None, 0, 0))
            return
        keep, ptr = _lambdas_arg("set_visit_lambdas", lambdas, len(lambdas), self.device if device else None)
        self._chk(self.lib.lentil_hip_set_visit_lambdas(self.h, ptr, len(lambdas), _abi.LAMBDAS_DEVICE_POINTER if device else 0))
        self._lambdas_keep = keep if device else None

    def spectral_pass_stats(self):
        """(passes run with a wavelength column over polynomial optics, solve tasks the spectral kernel took in them, the lens
        path of the last such pass as list_draws_path reports one, 0) since the context was created"""
        n = (C.c_uint64 * 4)()
        self._chk(self.lib.lentil_hip_spectral_pass_stats(self.h, n))
        return tuple(int(x) for x in n)

    def set_async(self, on):
        """the asynchronous end of a pass (include/lentil_hip.h): off = every redistribute waits for its own end"""
        self._chk(self.lib.lentil_hip_set_async(self.h, 1 if on else 0))

    def pass_totals(self, reset=False):
        """sums over the passes looked at since the last reset (observes the context: waits for what is in flight)"""
        t = _abi.PassTotals()
        self._chk(self.lib.lentil_hip_pass_totals(self.h, C.byref(t), 1 if reset else 0))
        return t

    def last_timing(self):
        ms = (C.c_float * 3)()
        self._chk(self.lib.lentil_hip_last_timing(self.h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def last_launches(self):
        n = (C.c_uint32 * 2)()
        self._chk(self.lib.lentil_hip_last_launches(self.h, n))
        return int(n[0]), int(n[1])

    def last_scan(self):
        """(kernel -- SCAN_DMA2 ... SCAN_RAGGED --, pixels per tile/group, dynamic LDS bytes, blocks) of the last pass's scan launch"""
        n = (C.c_uint32 * 4)()
        self._chk(self.lib.lentil_hip_debug_last_scan(self.h, n))
        return tuple(int(x) for x in n)

    def debug_last_crypto(self):
        """(kernel -- CRYPTO_DIRECT_ATOMIC / _OWNER / _TILE, 0 none --, the tile kernel's kTables, blocks, bit 0: flags from the
        work lists | bit 1: a put-off wipe flushed) of the last pass's own-pixel cryptomatte kernel; zeros before the first"""
        n = (C.c_uint32 * 4)()
        self._chk(self.lib.lentil_hip_debug_last_crypto(self.h, n))
        return tuple(int(x) for x in n)

    def lens_jit_status(self):
        """(state, compile seconds): 0 nothing to compile, 1 compiling, 2 specialised kernel in use, -1 failed"""
        st, sec = C.c_int(0), C.c_double(0.0)
        self._chk(self.lib.lentil_hip_lens_jit_status(self.h, C.byref(st), C.byref(sec)))
        return int(st.value), float(sec.value)

    def lens_jit_wait(self, timeout_seconds=0.0):
        self._chk(self.lib.lentil_hip_lens_jit_wait(self.h, float(timeout_seconds)))

    def lens_jit_source(self):
        n = C.c_uint64(0)
        self._chk(self.lib.lentil_hip_debug_lens_jit_source(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(int(n.value) + 1)
        self._chk(self.lib.lentil_hip_debug_lens_jit_source(self.h, buf, int(n.value) + 1, None))
        return buf.value.decode()

    def box_probe(self):
        """what the GPU delivers right now: fp64 chain rate, shader clock, copy / read bandwidth, hardware queues, CUs"""
        p = (C.c_double * 6)()
        self._chk(self.lib.lentil_hip_box_probe(self.h, p))
        return {"fp64_mul_add_tflops": round(p[0], 2), "shader_clock_mhz_under_fp64": round(p[1], 1), "copy_gbs": round(p[2], 1),
                "read_gbs": round(p[3], 1), "gpu_max_hw_queues": int(p[4]), "compute_units": int(p[5])}

    def batch_model_stats(self):
        """(calibrations, lean passes, lean passes that needed a second round after all, margin sixteenths)"""
        n = (C.c_uint64 * 4)()
        self._chk(self.lib.lentil_hip_batch_model_stats(self.h, n))
        return tuple(int(x) for x in n)

    def debug_batch_estimate(self, cs_xyz, samples):
        """[n, 4]: share well inside the frame, share inside, share vignetted, first batch -- for camera-space points [n, 3]"""
        import numpy as np
        cs = np.ascontiguousarray(cs_xyz, np.float32)
        out = np.zeros((cs.shape[0], 4), np.float32)
        self._chk(self.lib.lentil_hip_debug_batch_estimate(self.h, cs.shape[0], cs.ctypes.data, int(samples), out.ctypes.data))
        return out

    # --- cryptomatte AOVs
    def alloc_crypto(self, n_crypto, slots_per_pixel=0):
        self._chk(self.lib.lentil_hip_alloc_crypto(self.h, n_crypto, slots_per_pixel))

    def upload_crypto(self, crypto_visits):
        self._chk(self.lib.lentil_hip_upload_crypto(self.h, C.byref(crypto_visits)))

    def bind_crypto(self, crypto_visits, keepalive=None):
        self._chk(self.lib.lentil_hip_bind_crypto(self.h, C.byref(crypto_visits)))
        self._keep["crypto"] = keepalive

    def download_crypto(self, crypto, rank):
        """(np x 4 RGBA, np bool: the pixel's map has more than `rank` entries)"""
        out = np.empty((self.n_pixels, 4), np.float32)
        has = np.empty(self.n_pixels, np.uint8)
        self._chk(self.lib.lentil_hip_download_crypto(self.h, crypto, rank, out.ctypes.data, has.ctypes.data))
        return out, has.astype(bool)

    def download_crypto_table(self, crypto):
        """(id bits [np, slots] uint32 with 0xFFFFFFFF = free, weights [np, slots], totals [np])"""
        slots = C.c_uint32()
        self._chk(self.lib.lentil_hip_download_crypto_table(self.h, crypto, C.byref(slots), None, None, None))
        ids = np.empty((self.n_pixels, slots.value), np.uint32)
        wts = np.empty((self.n_pixels, slots.value), np.float32)
        tot = np.empty(self.n_pixels, np.float32)
        self._chk(self.lib.lentil_hip_download_crypto_table(self.h, crypto, C.byref(slots), ids.ctypes.data, wts.ctypes.data,
                                                            tot.ctypes.data))
        return ids, wts, tot

    def set_draw_log(self, capacity):
        self._chk(self.lib.lentil_hip_set_draw_log(self.h, capacity))

    def draw_log(self):
        n = C.c_uint64()
        self._chk(self.lib.lentil_hip_download_draw_log(self.h, None, 0, C.byref(n)))
        rec = np.empty((n.value, 3), np.uint32)
        if n.value:
            self._chk(self.lib.lentil_hip_download_draw_log(self.h, rec.ctypes.data, n.value, C.byref(n)))
        return rec

    # --- primitive tests
    def test_lt_sample_aperture(self, scene, ap, lam):
        scene = np.ascontiguousarray(scene, np.float64)
        ap = np.ascontiguousarray(ap, np.float64)
        n = scene.shape[0]
        sensor = np.empty((n, 5)); out = np.empty((n, 5)); T = np.empty((n,))
        self._chk(self.lib.lentil_hip_test_lt_sample_aperture(
            self.h, n, scene.ctypes.data, ap.ctypes.data, lam, sensor.ctypes.data, out.ctypes.data, T.ctypes.data))
        return sensor, out, T

    def test_trace_bw_po(self, target, px, py, attempt):
        target = np.ascontiguousarray(target, np.float64)
        px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32)
        attempt = np.ascontiguousarray(attempt, np.int32)
        n = target.shape[0]
        xy = np.empty((n, 2)); ok = np.empty((n,), np.int32)
        self._chk(self.lib.lentil_hip_test_trace_bw_po(
            self.h, n, target.ctypes.data, px.ctypes.data, py.ctypes.data, attempt.ctypes.data,
            xy.ctypes.data, ok.ctypes.data))
        return xy, ok

    def test_aperture_sample(self, a, b):
        a = np.ascontiguousarray(a, np.uint32); b = np.ascontiguousarray(b, np.uint32)
        xy = np.empty((a.shape[0], 2))
        self._chk(self.lib.lentil_hip_test_aperture_sample(self.h, a.shape[0], a.ctypes.data, b.ctypes.data,
                                                           xy.ctypes.data))
        return xy
