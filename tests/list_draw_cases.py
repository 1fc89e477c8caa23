"""The case table of the lentil_hip_plan_visits / lentil_hip_list_draws tests (tests/test_gpu_list_draws.py: the kernels
against the oracle; tests/test_list_draw_cases.py: the table itself against the oracle alone, no GPU).  A plain module: no
fixtures, fixed seeds; what it computes -- streams, the oracle's passes -- is computed once per process and never written to.

A case is a small frame (32x24 to 96x64, 9 visits per pixel) with a stream of common.make_stream; its expectation is the
oracle's single-threaded pass over that stream with the draw log kept: (visit, attempt, pixel) per accepted draw, the
counters, and the exact fp64 sums of the frame.
"""
import ctypes as C

import numpy as np

import common
import oracle_lib
from pota_amd import _abi, capi, workload

M = 9
LAM_BLUE = float(np.float32(0.45))          # the float the oracle's parameters hold, not the literal

CASES = {}
# the formula's counts grow with the square of the frame's height: at 32 rows they all sit near the floor of 4, so the case
# turns bidir_sample_mult up (the default is 5) until the counts straddle a slab: 8 ... 209
FORMULA_MULT = 40


def _case(name, camera="po", frame=(48, 32), samples=16, f_hi=0.03, seed=0x5EED, lens="double_gauss_50mm", lens_mode=None,
          path=None, bokeh=None, motion=False, ragged=False, lam=0.0, edge=None, unit=None, **params):
    """samples: samples_override (0: the reference's formula); lens_mode: what set_lens_mode gets (None: the default);
    path: what list_draws_path must report; edge: (lo, hi) -- every highlight is moved to lo ... hi of the half frame width
    from the centre, left or right (1.0: the frame's edge); unit: the unitModel, the stream's positions scaled to match"""
    assert name not in CASES
    if path is None:
        path = _abi.DRAWS_PATH_THIN_LENS if camera == "tl" else _abi.DRAWS_PATH_COMPILED_IN
    CASES[name] = dict(name=name, camera=camera, frame=frame, samples=samples, f_hi=f_hi, seed=seed, lens=lens, lens_mode=lens_mode,
                       path=path, bokeh=bokeh, motion=motion, ragged=ragged, lam=lam, edge=edge, unit=unit, params=params)


# samples-N: a partial slab, the slab boundary, several slabs, a 5 * samples that is no multiple of 64
SAMPLES_N = (4, 16, 63, 64, 65, 130, 200)
for _s in SAMPLES_N:
    _case("samples-%d" % _s, samples=_s, frame=(32, 24), f_hi=0.05 if _s < 63 else 0.02)      # (the oracle takes 0.2 ms per attempt)
# formula: the reference's own draw counts, different from visit to visit
_case("formula", samples=0, frame=(48, 32), f_hi=0.02, bidir_sample_mult=FORMULA_MULT)
# retries
for _r in (-1, 0, 3, 15):
    _case("retries%d" % _r, samples=16, vignetting_retries=_r)
# short: visits that run into 5 * samples before they have their draws -- highlights around the frame's edge
_case("short-po", samples=16, vignetting_retries=0, edge=(0.9, 1.25))
_case("short-tl", camera="tl", samples=16, edge=(0.9, 1.25), optical_vignetting_distance=2.0, optical_vignetting_radius=0.6)
# lens paths
_case("lens-double-gauss", samples=24)
# (the oracle's backward trace through the two Petzvals fails often and is slow: smaller frames, fewer draws)
_case("lens-petzval", samples=12, frame=(32, 24), lens="petzval_58mm", seed=0x51)
_case("lens-anamorphic", samples=8, frame=(32, 24), lens="anamorphic_petzval_58mm", seed=0x52, path=_abi.DRAWS_PATH_INTERPRETER)
_case("lens-interpreter", samples=24, lens_mode=1, path=_abi.DRAWS_PATH_INTERPRETER)
LENS_CASES = ("lens-double-gauss", "lens-petzval", "lens-anamorphic", "lens-interpreter")
# aperture samplers
_case("blades5", samples=20, bokeh_aperture_blades=5)
_case("bokeh-image", samples=20, bokeh="blacklines12", bokeh_enable_image=1)
_case("no-dof", samples=20, enable_dof=0)
# thin lens
_case("tl-plain", camera="tl", samples=20)
_case("tl-coma-vignetting", camera="tl", samples=20, abb_coma=0.35, optical_vignetting_distance=2.0, optical_vignetting_radius=1.5)
# a moving camera: two keys, lentil_time spread over the shutter
_case("moving-camera", samples=16, motion=True)
# a ragged stream: per-visit pixel and inverse density
_case("ragged", samples=0, ragged=True, frame=(64, 48), f_hi=0.02)
# fitted_bidir_add_energy
_case("add-energy", samples=16, bidir_add_energy=2.5)
# units
_case("unit-mm", samples=16, unit=_abi.UNIT_MM)
_case("unit-m", samples=16, unit=_abi.UNIT_M)
# wavelength: the list is asked for at 0.45, the context's lambda_bw stays 0.55
_case("lambda", samples=16, lam=LAM_BLUE)

ALL = sorted(CASES)
OWN_FILM_CASES = ("lens-double-gauss", "tl-coma-vignetting", "add-energy")

_UNIT_SCALE = {_abi.UNIT_MM: 0.1, _abi.UNIT_CM: 1.0, _abi.UNIT_DM: 10.0, _abi.UNIT_M: 100.0}


def motion_keys():
    """two world-to-camera keys (row-vector convention): the identity, and a camera a few centimetres further along x and y"""
    keys = np.stack([np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)])
    keys[1, 3, :3] = (3.0, -2.0, 0.5)
    return keys


def _copy_params(p):
    return type(p).from_buffer_copy(p)


_setups, _oracles = {}, {}


def setup(name):
    """dict: p (the context's parameters), p_oracle (the oracle's: lambda_bw is the case's wavelength), table / keep (None: thin
    lens), bokeh (a case of tests/bokeh_tables.py or None), visits, cols, keys (motion keys or None), frame, samples, lam,
    lens_mode, path, n (visits)"""
    if name in _setups:
        return _setups[name]
    c = CASES[name]
    w, h = c["frame"]
    params = dict(c["params"])
    if c["unit"] is not None:
        params["unitModel"] = c["unit"]
    if c["camera"] == "po":
        p, model, table, keep = common.po_setup(w, h, lens=c["lens"], samples_override=c["samples"], **params)
    else:
        p, table, keep = common.tl_setup(w, h, samples_override=c["samples"], **params), None, None
    cols = workload.generate(np, 0, w * h * M, w, h, M, seed=c["seed"], f_hi=c["f_hi"],
                             focus_dist=float(p.focus_distance) / (10.0 if p.cameraType == 1 else 1.0),
                             tan_half_fov=common.tan_half_fov(p))
    n = w * h * M
    rng = np.random.default_rng(c["seed"] ^ 0xC0FFEE)
    hi = cols["rgba"][:, 0] == np.float32(workload.HIGHLIGHT_RADIANCE)
    if c["edge"]:
        # the highlights go to the frame's left and right edges, half of them beyond: most of their draws miss the frame
        lo, up = c["edge"]
        pos = cols["pos_z"]
        k = int(hi.sum())
        side = np.where(rng.random(k) < 0.5, -1.0, 1.0)
        depth = -pos[hi, 2].astype(np.float64)
        pos[hi, 0] = (side * rng.uniform(lo, up, k) * common.tan_half_fov(p) * depth).astype(np.float32)
    if c["unit"] is not None:
        # the same scene in another unit: the camera-space positions come out (nearly) as the centimetre stream's
        cols["pos_z"][:, :3] = (cols["pos_z"][:, :3] / np.float32(_UNIT_SCALE[c["unit"]])).astype(np.float32)
    keys = None
    if c["motion"]:
        keys = motion_keys()
        cols["raydir_time"][:, 3] = rng.uniform(-0.1, 1.1, n).astype(np.float32)      # (beyond the shutter: clamped to a key)
    if c["ragged"]:
        px = rng.integers(0, w, n).astype(np.uint32)
        py = rng.integers(0, h, n).astype(np.uint32)
        cols["pixel"] = (px | (py << np.uint32(16))).astype(np.uint32)
        cols["inv_density"] = rng.choice(np.array([1 / 9., 1 / 16., 0.14], np.float32), n).astype(np.float32)
        visits, keepv = capi.make_visits(cols, visits_per_pixel=0)
    else:
        visits, keepv = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=w)
    for a in cols.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    p_oracle = _copy_params(p)
    if c["lam"] != 0.0:
        p_oracle.lambda_bw = c["lam"]
    s = dict(name=name, p=p, p_oracle=p_oracle, table=table, keep=keep, bokeh=c["bokeh"], visits=visits, cols=cols, keys=keys,
             frame=c["frame"], samples=c["samples"], lam=c["lam"], lens_mode=c["lens_mode"], path=c["path"], n=n, camera=c["camera"],
             highlights=hi)
    _setups[name] = s
    return s


def oracle_pass(orc, name):
    """the oracle's single-threaded pass over the case's stream -> dict: log uint32 [n, 3] sorted by (visit, attempt),
    visits / redistributed / attempted / accepted (its counters), buffer64 [pixels, 4] and weight64 [pixels] (its exact sums)"""
    if name in _oracles:
        return _oracles[name]
    s = setup(name)
    p = s["p_oracle"]
    lens = orc.orc_lens_create(C.byref(s["table"])) if s["table"] is not None else None
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    fr = oracle_lib.Frame(orc, p, n_aovs=1, keep_log=True)
    try:
        if s["keys"] is not None:
            fr.set_camera_motion(s["keys"])
        fr.run(lens, ob, s["visits"])
        c = fr.counters()
        o = dict(log=common.sort_log(fr.log()), visits=int(c.visits), redistributed=int(c.redistributed_visits),
                 attempted=int(c.attempted_draws), accepted=int(c.accepted_draws), buffer64=fr.buffer64(0), weight64=fr.weight64())
    finally:
        fr.close()
        if lens:
            orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    for a in (o["log"], o["buffer64"], o["weight64"]):
        a.setflags(write=False)
    _oracles[name] = o
    return o


def per_visit(log):
    """(visits, records per visit, last attempt per visit, contiguous per visit: attempts 0 ... records - 1) of a sorted log"""
    vis, first, count = np.unique(log[:, 0], return_index=True, return_counts=True)
    last = log[first + count - 1, 1].astype(np.int64)
    return vis, count, last, last == count - 1


def formula_samples(orc, name):
    """the reference's draw count of every highlight of a case whose camera stands still at the origin, in centimetres: the
    oracle's own pieces (orc_get_coc_thinlens, orc_draw_count) over the stream's columns -> (visits, samples)"""
    s = setup(name)
    p = s["p_oracle"]
    assert s["keys"] is None and p.unitModel == _abi.UNIT_CM and p.samples_override == 0
    vis = np.nonzero(s["highlights"])[0]
    rgba, pos = s["cols"]["rgba"], s["cols"]["pos_z"]
    invd = s["cols"].get("inv_density")
    out = np.zeros(vis.size, np.int64)
    for i, v in enumerate(vis):
        lum = np.float32(np.float64(np.float32(np.float32(rgba[v, 0] + rgba[v, 1]) + rgba[v, 2])) / 3.0)
        coc = orc.orc_get_coc_thinlens(C.byref(p), float(pos[v, 2]))
        out[i] = orc.orc_draw_count(C.byref(p), float(lum), coc, float(invd[v]) if invd is not None else float(p.inverse_sample_density))
    return vis, out
