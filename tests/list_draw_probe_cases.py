"""The case table of the LENTIL_DRAWS_PROBED tests (tests/test_gpu_list_draws_probed.py: lentil_hip_list_draws under an
occlusion probe against the oracle; tests/test_list_draw_probe_cases.py: the table itself against the oracle alone, no GPU).
A plain module: no fixtures, fixed seeds; what it computes is computed once per process and never written to.

A case is a case of tests/list_draw_cases.py's kind (setup() there builds it: a frame of 32x24 to 96x64, 9 visits per pixel, a
stream of common.make_stream's generator) plus a "scene": the analytic sphere of tests/test_gpu_probe.py, orc_sphere_occluder
on the CPU and lentil_hip_test_sphere_occluder_device on the GPU.  Its expectation is the oracle's single-threaded pass under
orc_frame_set_probe with the draw log kept.

What the oracle asks and what the library asks differ by design: the oracle probes every try it reaches before it solves it
(src/lentil.h:613-629), and every attempt that looks at a seed asks about it again; the library asks once per (visit, seed),
and only about the seeds that got through the lens.  With enable_dof = 0 every seed of a visit has the same aperture point
(0, 0), so all segments of one visit coincide: "once per (visit, seed)" then means as many identical segments as the walk
reaches lens-passing seeds, and the answer is the same for all of them -- a visit is drawn as without a probe or not at all.
"""
import ctypes as C

import numpy as np

import common
import list_draw_cases as lc
import oracle_lib
from pota_amd import _abi, capi

M = lc.M
SPHERE = (6.0, 2.0, -70.0, 9.0)            # cm, camera at the origin looking down -z: beside the axis, in front of the far highlights

CASES = {}


def _case(name, sphere=SPHERE, c2w=None, mutate=None, model=False, **kw):
    """kw: what list_draw_cases._case takes.  sphere: (cx, cy, cz, r) in camera space, centimetres -- moved into the world and
    scaled to the case's unit by setup(); or a function of the setup dict.  c2w: "given": the probe gets camera_to_world
    explicitly.  mutate(p, cols, s): changes the copied parameters and columns before the visits are made.  model: the case has
    a static camera at the origin, centimetres and polynomial optics -- the exact model of the GPU test applies."""
    assert name not in CASES
    kw.setdefault("frame", (32, 24))                           # (the oracle takes 0.2 ms per attempt, and asks through Python)
    CASES[name] = dict(name=name, sphere=sphere, c2w=c2w, mutate=mutate, model=model, kw=kw)


# samples-N: slab boundaries, with occlusion pushing visits across them
for _s in (4, 16, 63, 64, 65, 130):
    _case("samples-%d" % _s, model=True, samples=_s, frame=(32, 24), f_hi=0.05 if _s < 63 else 0.01)
# retries: -1 makes no try, so nothing is asked and nothing is listed
for _r in (-1, 0, 3, 15):
    _case("retries%d" % _r, model=_r >= 0, samples=16, vignetting_retries=_r)
# swallowed: a sphere so large and near that some visits are fully occluded: all 5 * samples attempts, no record
_case("swallowed", sphere=(4.0, 1.0, -40.0, 14.0), model=True, samples=16, vignetting_retries=3)


def _edge_sphere(s):
    thf = common.tan_half_fov(s["p"])
    return (0.95 * thf * 70.0, 0.0, -70.0, 9.0)


# highlights at the frame's edge (most draws miss the frame), the sphere out there with them
_case("edge", sphere=_edge_sphere, model=True, samples=16, vignetting_retries=0, edge=(0.9, 1.25))
_case("tl-plain", camera="tl", samples=20)
_case("tl-coma-vignetting", camera="tl", samples=20, abb_coma=0.35, optical_vignetting_distance=2.0, optical_vignetting_radius=1.5)
_case("bokeh-image", model=True, samples=20, bokeh="blacklines12", bokeh_enable_image=1)
_case("blades5", model=True, samples=20, bokeh_aperture_blades=5)
_case("no-dof", model=True, samples=20, enable_dof=0)               # (see the module's docstring)
_case("moving-camera", samples=16, motion=True)
_case("unit-mm", samples=16, unit=_abi.UNIT_MM)
_case("ragged", model=True, samples=0, ragged=True, frame=(64, 48), f_hi=0.02)
_case("lens-interpreter", model=True, samples=24, f_hi=0.015, lens_mode=1, path=_abi.DRAWS_PATH_INTERPRETER)
_case("lens-anamorphic", model=True, samples=8, frame=(32, 24), f_hi=0.01, vignetting_retries=3, lens="anamorphic_petzval_58mm", seed=0x52, path=_abi.DRAWS_PATH_INTERPRETER)


def _moved_c2w():
    """the camera of test_probe_with_a_given_camera_to_world_and_a_moved_camera: a rotation about y and a translation"""
    a = np.float32(0.1)
    rot = np.array([[np.cos(a), 0, -np.sin(a), 0], [0, 1, 0, 0], [np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], np.float64)
    tr = np.eye(4); tr[3, :3] = (5.0, -3.0, 20.0)
    return (rot @ tr).astype(np.float32)                       # row-vector convention: p_world = p_cam @ c2w


def _move_camera(p, cols, s):
    c2w = _moved_c2w()
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    for r in range(4):
        for c in range(4):
            p.world_to_camera[r][c] = float(w2c[r, c])
    pos = cols["pos_z"]                                        # generated in camera space, moved into the world
    ph = np.concatenate([pos[:, :3].astype(np.float64), np.ones((pos.shape[0], 1))], axis=1) @ c2w.astype(np.float64)
    pos[:, :3] = ph[:, :3].astype(np.float32)
    s["world"] = c2w


_case("moved-camera-given", c2w="given", mutate=_move_camera, samples=16)
_case("moved-camera-computed", mutate=_move_camera, samples=16)


def _skydome(p, cols, s):
    """every other highlight comes from the skydome: depth infinite, the ray's direction where the position was"""
    p.enable_skydome = 1
    hi = np.nonzero(s["highlights"])[0][::2]
    pos = cols["pos_z"]
    d = pos[hi, :3].astype(np.float64)
    d /= np.linalg.norm(d, axis=1)[:, None]
    cols["raydir_time"][hi, :3] = d.astype(np.float32)
    pos[hi, 3] = np.float32(1.0e30)                            # AI_INFINITE
    s["skydome"] = hi


_case("skydome", mutate=_skydome, samples=16)

ALL = sorted(CASES)
MODEL = sorted(n for n in CASES if CASES[n]["model"])

_setups, _oracles, _keep = {}, {}, []


def _lc_setup(name, kw):
    """list_draw_cases.setup() of a case that is not in its table: entered for the call, taken out again"""
    key = "probed:" + name
    saved = dict(lc.CASES)
    try:
        lc.CASES.clear()
        lc._case(key, **kw)
        return lc.setup(key)
    finally:
        lc.CASES.clear()
        lc.CASES.update(saved)


def setup(name):
    """list_draw_cases.setup()'s dict, and: sphere (float32 [4], world space, the case's unit), c2w (float32 [4, 4] or None: what
    the probe is given as camera_to_world), skydome (visits the skydome supplied, or None), model (bool)"""
    if name in _setups:
        return _setups[name]
    c = CASES[name]
    s = dict(_lc_setup(name, c["kw"]))
    s.update(name=name, model=c["model"], skydome=None, world=None)
    if c["mutate"]:
        p = lc._copy_params(s["p"])
        cols = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s["cols"].items()}
        c["mutate"](p, cols, s)
        if "pixel" in cols:
            visits, keepv = capi.make_visits(cols, visits_per_pixel=0)
        else:
            visits, keepv = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=s["frame"][0])
        _keep.append(keepv)
        for a in cols.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        s.update(p=p, p_oracle=lc._copy_params(p), cols=cols, visits=visits)
    sp = np.array(c["sphere"](s) if callable(c["sphere"]) else c["sphere"], np.float64)
    if s["world"] is not None:
        sp[:3] = (np.array([sp[0], sp[1], sp[2], 1.0]) @ s["world"].astype(np.float64))[:3]
    sp = sp / lc._UNIT_SCALE[int(s["p"].unitModel)]            # (centre and radius alike: the same scene in another unit)
    s["sphere"] = sp.astype(np.float32)
    s["sphere"].setflags(write=False)
    s["c2w"] = s["world"] if c["c2w"] == "given" else None
    _setups[name] = s
    return s


PROBE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)


class Recorder:
    """a lentil_probe_fn in Python: hands every list to `inner` (the address of a C lentil_probe_fn) and keeps what it saw --
    calls (list lengths), segments (float32 [n, 6]: origin, target), answers (uint8 [n])"""

    def __init__(self, inner, user):
        self._inner = PROBE_FN(inner)
        self._user = user
        self.calls, self._seg, self._occ = [], [], []
        self.fn = PROBE_FN(self._call)
        self.address = C.cast(self.fn, C.c_void_p).value

    def _call(self, user, n, seg, occ):
        self._inner(self._user, n, seg, occ)
        self.calls.append(int(n))
        self._seg.append(C.string_at(seg, 24 * n))
        self._occ.append(C.string_at(occ, n))

    def segments(self):
        return np.frombuffer(b"".join(self._seg), np.float32).reshape(-1, 6)

    def answers(self):
        return np.frombuffer(b"".join(self._occ), np.uint8)


def oracle_pass(orc, name, probed=True):
    """the oracle's single-threaded pass over the case's stream, under the case's probe or free of it -> dict: log uint32
    [n, 3] sorted by (visit, attempt), visits / redistributed / attempted / accepted (its counters) and, probed, segments
    float32 [k, 6] / answers uint8 [k]: everything the oracle asked, in its order (repeats included)"""
    key = (name, probed)
    if key in _oracles:
        return _oracles[key]
    s = setup(name)
    p = s["p_oracle"]
    lens = orc.orc_lens_create(C.byref(s["table"])) if s["table"] is not None else None
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    fr = oracle_lib.Frame(orc, p, n_aovs=1, keep_log=True)
    rec = None
    try:
        if s["keys"] is not None:
            fr.set_camera_motion(s["keys"])
        if probed:
            rec = Recorder(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data)
            fr.set_probe(rec.address, None, s["c2w"])
        fr.run(lens, ob, s["visits"])
        c = fr.counters()
        o = dict(log=common.sort_log(fr.log()), visits=int(c.visits), redistributed=int(c.redistributed_visits),
                 attempted=int(c.attempted_draws), accepted=int(c.accepted_draws))
        if probed:
            o["segments"], o["answers"] = rec.segments(), rec.answers()
    finally:
        fr.close()
        if lens:
            orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _oracles[key] = o
    return o
