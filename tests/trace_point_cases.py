"""The case table of the lentil_hip_trace_points tests (tests/test_gpu_trace_points.py: the kernel against the oracle;
tests/test_trace_point_cases.py: the table itself against the oracle alone, no GPU).  A plain module: no fixtures, fixed
seeds; what it computes -- inputs, the oracle's answers -- is computed once per process and never written to.

A polynomial-optics case is a batch: n points x K attempts.  Its expectation is orc_trace_ray_bw_po per query (ok, tries,
sensor x / y) and, restated here in fp64, the sensor -> pixel mapping the oracle's visit loop applies to it.
A pass case is a stream the oracle redistributes single-threaded with its draw log kept: the batch then asks for every
attempt 0 ... the last logged one of every visit in the log.
"""
import ctypes as C

import numpy as np

import common
import oracle_lib
from pota_amd import _abi, lens_io

VIGNETTED, OUTSIDE = _abi.POINT_VIGNETTED, _abi.POINT_OUTSIDE

# wavelengths as the oracle takes them: a float argument (the batch's double holds the same value)
LAM_BLUE, LAM_RED = float(np.float32(0.45)), float(np.float32(0.65))

CASES = {}


def _case(name, n, k, frame=(64, 48), lens="double_gauss_50mm", lam=0.0, first="random", seed=3, bokeh=None, perturb=False,
          lens_mode=None, path=_abi.POINTS_PATH_COMPILED_IN, **params):
    """first: "random" (first_attempt uniform below 3000), None (the NULL pointer: attempts from 0)
    lens_mode: what to pass to set_lens_mode (None: the default); path: what trace_points_path must report afterwards"""
    assert name not in CASES
    CASES[name] = dict(name=name, n=n, k=k, frame=frame, lens=lens, lam=lam, first=first, seed=seed, bokeh=bokeh,
                       perturb=perturb, lens_mode=lens_mode, path=path, params=params)


# po-flat: the 4096 points of test_trace_bw_po_bit_exact, one attempt each -- under every retry budget
_case("po-flat", 4096, 1)
for _r in (-1, 0, 3):
    _case("po-flat-retries%d" % _r, 4096, 1, vignetting_retries=_r)
# po-slabs: a partial slab, an exact one, the step into a second, a third
for _k in (1, 63, 64, 65, 130):
    _case("po-slabs-k%d" % _k, 24, _k, frame=(96, 64), seed=40 + _k)
_case("po-slabs-k65-from0", 24, 65, frame=(96, 64), seed=77, first=None)
# lens paths
_case("po-flat-interpreter", 4096, 1, lens_mode=1, path=_abi.POINTS_PATH_INTERPRETER)
_case("petzval", 512, 3, lens="petzval_58mm", seed=5)
_case("anamorphic", 512, 3, lens="anamorphic_petzval_58mm", seed=6, path=_abi.POINTS_PATH_INTERPRETER)     # cylindrical pupil; not compiled in
_case("perturbed", 512, 3, seed=7, perturb=True, path=_abi.POINTS_PATH_INTERPRETER)                       # a table nobody ships
# aperture samplers
_case("blades5", 512, 3, seed=8, bokeh_aperture_blades=5)
_case("bokeh-image", 512, 3, seed=9, bokeh="blacklines12", bokeh_enable_image=1)
_case("no-dof", 512, 3, seed=10, enable_dof=0)
# wavelength (0: params.lambda_bw, every case above)
_case("lambda-blue", 512, 3, seed=11, lam=LAM_BLUE)
_case("lambda-red", 512, 3, seed=12, lam=LAM_RED)

PO_CASES = sorted(CASES)

PASS_CASES = {
    "pass-tl-vignetting": dict(camera="tl", params=dict(abb_coma=0.35, optical_vignetting_distance=2.0, optical_vignetting_radius=1.5)),
    "pass-tl-plain": dict(camera="tl", params={}),
    "pass-po": dict(camera="po", params={}),
}
PASS_FRAME, PASS_M, PASS_SAMPLES, PASS_F_HI = (96, 64), 9, 16, 0.02


def pack_pixel(px, py):
    return (np.asarray(px).astype(np.uint32) | (np.asarray(py).astype(np.uint32) << np.uint32(16))).astype(np.uint32)


_setups, _oracles, _passes = {}, {}, {}


def setup(name):
    """dict: p, table, keep (owns the table's terms), bokeh (a case of tests/bokeh_tables.py or None), cs float32 [n, 3],
    pixel uint32 [n], first uint32 [n] or None, k, lam, px / py int arrays"""
    if name in _setups:
        return _setups[name]
    c = CASES[name]
    w, h = c["frame"]
    p, model, table, keep = common.po_setup(w, h, lens=c["lens"], **c["params"])
    if c["perturb"]:
        # one coefficient of the first outer-pupil polynomial moved by a part in a thousand: another table hash
        spec = dict(model.spec)
        spec["polys"] = {k: [list(t) for t in v] for k, v in model.spec["polys"].items()}
        coeff, exps = spec["polys"]["out_x"][1]
        spec["polys"]["out_x"][1] = [coeff * (1.0 + 1.0 / 1024.0), exps]
        table, keep = lens_io.make_lens_table(spec)
    rng = np.random.default_rng(c["seed"])
    n = c["n"]
    # drawn as test_trace_bw_po_bit_exact draws them (millimetres in front of the lens), stored as the renderer has them
    target = np.stack([rng.uniform(-600, 600, n), rng.uniform(-400, 400, n), rng.uniform(500, 5000, n)], 1)
    px = rng.integers(0, w, n).astype(np.int32)
    py = rng.integers(0, h, n).astype(np.int32)
    att = rng.integers(0, 3000, n).astype(np.uint32)
    cs = np.ascontiguousarray((-target / 10.0).astype(np.float32))
    s = dict(name=name, p=p, table=table, keep=keep, bokeh=c["bokeh"], cs=cs, px=px, py=py, pixel=pack_pixel(px, py),
             first=att if c["first"] == "random" else None, k=c["k"], lam=c["lam"], lens_mode=c["lens_mode"], path=c["path"])
    for a in (cs, s["pixel"], att):
        a.setflags(write=False)
    _setups[name] = s
    return s


def pixel_mapping(p, sensor):
    """the oracle's sensor -> pixel mapping (its visit loop, the lines that follow the backward trace) restated in fp64:
    sensor [..., 2] -> (xy [..., 2], pixel uint32 [...]: the linear pixel or OUTSIDE).  The aspect ratio is formed as the
    oracle forms it: both resolutions widened to double, then divided."""
    sx, sy = sensor[..., 0], sensor[..., 1]
    half = np.float64(p.sensor_width) * 0.5
    aspect = np.float64(p.xres_without_region) / np.float64(p.yres_without_region)
    s0 = sx / half
    s1 = sy / half * aspect
    pixel0 = (((s0 + 1.0) / 2.0) * np.float64(p.xres_without_region)) - np.float64(p.region_min_x)
    pixel1 = (((-s1 + 1.0) / 2.0) * np.float64(p.yres_without_region)) - np.float64(p.region_min_y)
    with np.errstate(invalid="ignore"):
        outside = (pixel0 >= p.xres) | (pixel0 < 0) | (pixel1 >= p.yres) | (pixel1 < 0) | (pixel0 != pixel0) | (pixel1 != pixel1)
        ix = np.where(outside, 0, np.floor(pixel0)).astype(np.int64)
        iy = np.where(outside, 0, np.floor(pixel1)).astype(np.int64)
    pixel = np.where(outside, OUTSIDE, ix + iy * int(p.xres)).astype(np.uint32)
    return np.stack([pixel0, pixel1], -1), pixel


def oracle_po(orc, name):
    """the oracle over every query of a polynomial-optics case -> dict: ok bool [n, k], tries int32 [n, k], sensor fp64
    [n, k, 2] (NaN where not ok), xy fp64 [n, k, 2], pixel uint32 [n, k] (VIGNETTED where not ok)"""
    if name in _oracles:
        return _oracles[name]
    s = setup(name)
    p, n, k = s["p"], s["cs"].shape[0], s["k"]
    lens = orc.orc_lens_create(C.byref(s["table"]))
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    lam = s["lam"] if s["lam"] != 0.0 else p.lambda_bw
    ok = np.zeros((n, k), bool)
    tries = np.zeros((n, k), np.int32)
    sensor = np.full((n, k, 2), np.nan)
    sp, tr = (C.c_double * 2)(), C.c_int()
    try:
        for i in range(n):
            cs = s["cs"][i]
            target = oracle_lib.darr(-float(cs[0]) * 10.0, -float(cs[1]) * 10.0, -float(cs[2]) * 10.0)
            first = int(s["first"][i]) if s["first"] is not None else 0
            for m in range(k):
                ok[i, m] = orc.orc_trace_ray_bw_po(C.byref(p), lens, ob, target, sp, int(s["px"][i]), int(s["py"][i]), first + m,
                                                   lam, C.byref(tr))
                tries[i, m] = tr.value
                if ok[i, m]:
                    sensor[i, m] = sp[0], sp[1]
    finally:
        orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    xy, pixel = pixel_mapping(p, sensor)
    pixel = np.where(ok, pixel, VIGNETTED).astype(np.uint32)
    o = dict(ok=ok, tries=tries, sensor=sensor, xy=xy, pixel=pixel)
    for a in o.values():
        a.setflags(write=False)
    _oracles[name] = o
    return o


def classes(o):
    """the four classes of a polynomial-optics case's queries -> dict of counts"""
    ok, tries, pixel = o["ok"], o["tries"], o["pixel"]
    return dict(vignetted=int((~ok).sum()), retried=int((ok & (tries > 0)).sum()), outside=int((ok & (pixel == OUTSIDE)).sum()),
                inside=int((ok & (pixel < OUTSIDE)).sum()), queries=int(ok.size))


def pass_case(orc, name):
    """the oracle's single-threaded pass of a pass case -> dict: p, table (None: thin lens), keep, cs float32 [n, 3], pixel
    uint32 [n], k, last int [n] (the last logged attempt of each visit), landed: pixel uint32 [n, k] (the logged pixel where
    (visit, attempt) is in the log, VIGNETTED elsewhere), visits (their numbers)"""
    if name in _passes:
        return _passes[name]
    c = PASS_CASES[name]
    w, h = PASS_FRAME
    if c["camera"] == "po":
        p, model, table, keep = common.po_setup(w, h, samples_override=PASS_SAMPLES, **c["params"])
    else:
        p, table, keep = common.tl_setup(w, h, samples_override=PASS_SAMPLES, **c["params"]), None, None
    identity = np.eye(4, dtype=np.float32)
    assert np.array_equal(np.array([[p.world_to_camera[r][q] for q in range(4)] for r in range(4)], np.float32), identity)
    assert p.unitModel == _abi.UNIT_CM and p.abb_chromatic == 0.0
    visits, cols = common.make_stream(p, w, h, PASS_M, f_hi=PASS_F_HI)
    fr = common.run_oracle(orc, p, table, visits, keep_log=True, threads=1)
    log = fr.log()
    fr.close()
    assert log.shape[0] > 0
    vis = np.unique(log[:, 0])
    idx = np.searchsorted(vis, log[:, 0])
    k = int(log[:, 1].max()) + 1
    last = np.zeros(vis.size, np.int64)
    np.maximum.at(last, idx, log[:, 1].astype(np.int64))
    landed = np.full((vis.size, k), VIGNETTED, np.uint32)
    landed[idx, log[:, 1]] = log[:, 2]
    pos = np.asarray(cols["pos_z"], np.float32).reshape(-1, 4)
    cs = np.ascontiguousarray(pos[vis, :3])            # world_to_camera is the identity, the unit centimetres
    pix = vis // PASS_M
    r = dict(name=name, p=p, table=table, keep=keep, cs=cs, pixel=pack_pixel(pix % w, pix // w), k=k, last=last, landed=landed,
             visits=vis)
    for a in (cs, r["pixel"], last, landed):
        a.setflags(write=False)
    _passes[name] = r
    return r


def pass_counts(r):
    """(absent, attempts): attempts up to each visit's last logged one, and how many of them are not in the log"""
    upto = np.arange(r["k"])[None, :] <= r["last"][:, None]
    return int((upto & (r["landed"] == VIGNETTED)).sum()), int(upto.sum())
