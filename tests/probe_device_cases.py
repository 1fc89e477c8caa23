"""Occlusion probes answered on the GPU (lentil_hip_set_occlusion_probe_device): the cases of tests/test_gpu_probe_device.py and
tests/test_native_exchange_probe_device.py, importable without a GPU.

Every case is the 96 x 64 frame of tests/test_gpu_probe.py -- 9 visits per pixel, 2 % highlights -- behind an analytic sphere;
the reference is the oracle with its own sphere occluder.  A case is a dict: `name`, `camera` ("po" polynomial optics, "tl" the
plain thin lens, "tlc" the thin lens with abb_chromatic = 0.6), `S` = samples_override, `f_hi`, `n_extra`, `sphere` (camera
space, cm; radius last), `moved` (the camera of test_probe_with_a_given_camera_to_world_and_a_moved_camera; "given": with
AiCameraToWorldMatrix handed over, "null": computed by the library), `env` (what the library reads at lentil_hip_create) and
`exempt`: the degenerate lists, which need not satisfy what tests/test_probe_device_cases.py holds every other case to -- the
sphere occludes some but not all segments, and the oracle's accepted draws differ from the unprobed frame's.
"""
import ctypes as C

import numpy as np

import common

W, H, M = 96, 64, 9
SPHERE = (6.0, 2.0, -70.0, 9.0)       # beside the optical axis, between the lens and the far highlights
KINDS_TLC = [0, 0, 1]
# Round 0 of LONG lists more segments than the apply kernel's grid has lanes (num_cu * 4 blocks of 256: 262 144 on the
# 256 CUs of an MI355X), so lanes go round its loop more than once.  One chunk holds the whole list.  The smallest
# samples_override that gets there: see the test's docstring for the lengths measured on either side.
LONG_S = 254
APPLY_GRID_LANES_PER_CU = 4 * 256

BASE = dict(camera="po", S=48, f_hi=0.02, n_extra=1, sphere=SPHERE, moved=None, env={}, exempt=False)


def _case(name, **kw):
    c = dict(BASE)
    c.update(kw)
    c["name"] = name
    return c


CASES = [
    # 1. two passes each, three chunk streams side by side
    _case("po", env={"LENTIL_CHUNKS": "3"}),
    _case("tl", camera="tl", env={"LENTIL_CHUNKS": "3"}),
    # 2. a list longer than the apply grid
    _case("po-long", S=LONG_S, n_extra=0, env={"LENTIL_CHUNKS": "1"}),
    # 3. degenerate lists
    _case("no-highlights", f_hi=0.0, exempt=True),
    _case("radius-0", sphere=(6.0, 2.0, -70.0, 0.0), exempt=True),
    _case("lens-swallowed", sphere=(0.0, 0.0, 0.0, 40.0), exempt=True),
    # 4. a blind pass whose lists may hold 64 segments
    _case("overflow", env={"LENTIL_PROBE_DEVICE_CAP": "64"}),
    # 5. sub-batches of items (the figures of test_sub_batches_when_the_result_pool_is_small)
    _case("sub-batches", S=64, n_extra=0, env={"LENTIL_MAX_POOL_UNITS": "20000", "LENTIL_CHUNKS": "5"}),
    # 6. a camera away from the origin
    _case("moved-given", S=32, n_extra=0, moved="given"),
    _case("moved-null", S=32, n_extra=0, moved="null"),
    # 7. thin lens with abb_chromatic = 0.6 (tests/test_gpu_probe_tl_chroma.py)
    _case("tlc", camera="tlc", n_extra=2),
    _case("tlc-rerun", camera="tlc", n_extra=2, tlc=dict(abb_chromatic_type=1, abb_coma=0.35, optical_vignetting_distance=2.0,
                                                          optical_vignetting_radius=1.5)),
    # 8. across ranks: the stream and parameters of tests/test_native_exchange_tl_chroma.py
    _case("tlc-ranks", camera="tlc", n_extra=2, tlc=dict(abb_chromatic_type=0, abb_coma=0.35, optical_vignetting_distance=2.0,
                                                          optical_vignetting_radius=1.5)),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PARITY = [c for c in CASES if not c["exempt"]]


def ids(cases):
    return [c["name"] for c in cases]


def moved_camera():
    """camera-to-world of the moved camera (row-vector convention: p_world = p_cam @ c2w) and its fp32 inverse"""
    a = np.float32(0.1)
    rot = np.array([[np.cos(a), 0, -np.sin(a), 0], [0, 1, 0, 0], [np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], np.float64)
    tr = np.eye(4); tr[3, :3] = (5.0, -3.0, 20.0)
    c2w = (rot @ tr).astype(np.float32)
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    return c2w, w2c


def setup(c):
    """(params, lens table or None, visits, sphere as four floats, camera_to_world to hand over or None, what must stay alive)"""
    if c["camera"] == "po":
        p, model, table, keep = common.po_setup(W, H, samples_override=c["S"])
    elif c["camera"] == "tl":
        p, model, table, keep = common.tl_setup(W, H, samples_override=c["S"]), None, None, None
    else:
        p = common.tl_setup(W, H, samples_override=c["S"], abb_chromatic=0.6, **c.get("tlc", dict(abb_chromatic_type=0, abb_coma=0.0, optical_vignetting_distance=0.0,
                                                                                              optical_vignetting_radius=1.5)))
        model = table = keep = None
    sphere = np.array(c["sphere"], np.float32)
    c2w_arg = None
    if c["moved"]:
        c2w, w2c = moved_camera()
        for r in range(4):
            for k in range(4):
                p.world_to_camera[r][k] = float(w2c[r, k])
    visits, cols = common.make_stream(p, W, H, M, f_hi=c["f_hi"], n_extra=c["n_extra"])
    if c["moved"]:
        # samples generated in camera space, moved into the world; so is the sphere
        pos = cols["pos_z"]
        ph = np.concatenate([pos[:, :3].astype(np.float64), np.ones((pos.shape[0], 1))], axis=1) @ c2w.astype(np.float64)
        pos[:, :3] = ph[:, :3].astype(np.float32)
        sw = np.array([c["sphere"][0], c["sphere"][1], c["sphere"][2], 1.0]) @ c2w.astype(np.float64)
        sphere = np.array([sw[0], sw[1], sw[2], c["sphere"][3]], np.float32)
        if c["moved"] == "given":
            c2w_arg = c2w
    return p, table, visits, sphere, c2w_arg, (model, keep, cols)


def kinds(c):
    return KINDS_TLC if c["camera"] == "tlc" else None


def n_aovs(c):
    return 1 + c["n_extra"]


class Counting:
    """the oracle's sphere occluder behind a CFUNCTYPE wrapper that counts segments and occluded answers"""

    def __init__(self, orc):
        import oracle_lib
        fn_t = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)
        inner = fn_t(oracle_lib.sphere_occluder(orc))
        import threading
        self.probed = self.occluded = 0
        lock = threading.Lock()       # (the threaded oracle calls from all its threads)

        def counting(user, n, seg, occluded):
            inner(user, n, seg, occluded)
            occ = (1 if C.c_uint8.from_address(occluded).value else 0) if n == 1 else sum(1 for b in (C.c_uint8 * n).from_address(occluded) if b)
            with lock:
                self.probed += n
                self.occluded += occ

        self._keep = (inner, fn_t(counting))
        self.address = C.cast(self._keep[1], C.c_void_p).value


def stream_key(c):
    """everything of a case the oracle's run depends on"""
    return (c["camera"], c["S"], c["f_hi"], c["n_extra"], tuple(c["sphere"]), c["moved"], tuple(sorted(c.get("tlc", {}).items())))


_ORACLE = {}      # (stream_key, how) -> frame: every run is made once per session and never changed


def oracle(orc, c, how="probed"):
    """The oracle's frame of the case, computed once.  how: "probed" (the oracle's own sphere occluder), "free" (no probe),
    "counted" (the sphere behind Counting; the frame's `.counting` holds the sums).  Polynomial optics and the plain thin lens run
    threaded; the chromatic thin lens draws from one generator in visit order and runs single-threaded."""
    import oracle_lib
    key = (stream_key(c), how)
    if key not in _ORACLE:
        p, table, visits, sphere, c2w, keep = setup(c)
        counting = Counting(orc) if how == "counted" else None
        fn = counting.address if counting else oracle_lib.sphere_occluder(orc)
        probe = None if how == "free" else ((fn, sphere.ctypes.data) if c2w is None else (fn, sphere.ctypes.data, c2w))
        if c["camera"] == "tlc" or counting:
            # (the counting wrapper holds the interpreter's lock: threads would only queue for it)
            lens = orc.orc_lens_create(C.byref(table)) if table is not None else None
            ref = oracle_lib.Frame(orc, p, n_aovs=n_aovs(c), kinds=kinds(c), keep_log=True)
            if probe is not None:
                ref.set_probe(*probe)
            ref.run(lens, None, visits)
            if lens:
                orc.orc_lens_destroy(lens)
            st = (C.c_uint32 * 4)()
            orc.orc_frame_get_xor128(ref.h, st)
            ref.xor128_end = list(st)
        else:
            ref = common.ThreadedOracle(orc, p, table, visits, 4, n_aovs=n_aovs(c), kinds=kinds(c), probe=probe)
        ref.counting = counting
        ref.keep = (keep, sphere, visits)
        _ORACLE[key] = ref
    return _ORACLE[key]


def sorted_log(ref):
    return common.sort_log(ref.log())
