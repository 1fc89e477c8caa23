"""The case table of the spectral batch tests (tests/test_gpu_spectral_rays.py, tests/test_gpu_spectral_points.py: the
kernels against the oracle; tests/test_spectral_cases.py: the table itself against the oracle alone, no GPU).  A plain
module: no fixtures, fixed seeds; what it computes is computed once per process and never written to.

A ray case: a lens, a set-up, n camera samples, a wavelength per ray.  Its expectation is oracle_rays called per ray with
that ray's wavelength.  A point case: a lens, n points x K attempts, a wavelength per point; its expectation is
orc_trace_ray_bw_po per query with the point's wavelength (0: params.lambda_bw) and the sensor -> pixel mapping of
tests/trace_point_cases.py.  The backward oracle takes its wavelength as a float, so the points' wavelengths are float32
values widened; the forward oracle takes a double, and the rays' wavelengths use all of it.

Every polynomial-optics case also carries `pair`: two of its own wavelengths, under each of which the whole case is traced
once more (every ray, every query at the one wavelength).  tests/test_spectral_cases.py holds each case to what it is there
for with them: the wavelength moves (nearly) every result, it changes whether some ray or query retries -- so the lanes of a
wave disagree about retrying -- and something retries at all.
"""
import ctypes as C

import numpy as np

import common
import oracle_lib
import trace_point_cases as tc
from pota_amd import _abi
from test_gpu_camera_rays import _bokeh_tables, _inputs, oracle_rays

W, H = 640, 360
SEED = 0x1234
LAM_BLUE, LAM_RED = tc.LAM_BLUE, tc.LAM_RED            # float32 values: both oracles take them exactly
LAM_PALETTE = (LAM_BLUE, float(np.float32(0.55)), LAM_RED)
N_RAYS = 600                                           # two blocks and a partial wave

RAY_LENSES = ("double_gauss_50mm", "petzval_58mm", "anamorphic_petzval_58mm")
RAY_SETUPS = {
    "disk": dict(),
    "image": dict(bokeh_enable_image=1),
    "retries0": dict(vignetting_retries=0),
    "no_dof": dict(enable_dof=0),
}
RAY_CASES = ["%s/%s" % (lens, setup) for lens in RAY_LENSES for setup in sorted(RAY_SETUPS)]

_ray_setups, _ray_oracles, _ray_pairs = {}, {}, {}


def ray_lambdas(n, seed=17):
    """n wavelengths uniform in [0.40, 0.70] micrometres"""
    return np.random.default_rng(seed).uniform(0.40, 0.70, n)


def ray_setup(name):
    """dict: p, table, keep, tables (set_bokeh's, or None), image (bool), inp float32 [n, 6], lambdas fp64 [n], pair"""
    if name not in _ray_setups:
        lens, setup = name.split("/")
        kw = RAY_SETUPS[setup]
        p, model, table, keep = common.po_setup(W, H, lens=lens, **kw)
        # the samples reach past the image circle (|sx| up to 1.1), where what vignettes depends on the wavelength
        inp = _inputs(N_RAYS, 9, 1.1, 0.7)
        lambdas = ray_lambdas(N_RAYS)
        for a in (inp, lambdas):
            a.setflags(write=False)
        _ray_setups[name] = dict(name=name, p=p, table=table, keep=keep, image=bool(kw.get("bokeh_enable_image")), inp=inp,
                                 lambdas=lambdas, pair=(float(lambdas.min()), float(lambdas.max())))
    return _ray_setups[name]


def _rays_at(orc, s, lambdas):
    """oracle_rays per ray, each with its own wavelength -> ([n, 21] float32, [n] int32)"""
    tables, ob = _bokeh_tables(orc) if s["image"] else (None, None)
    lens = orc.orc_lens_create(C.byref(s["table"]))
    n = s["inp"].shape[0]
    out, tries = np.zeros((n, 21), np.float32), np.zeros(n, np.int32)
    try:
        for i in range(n):
            o, t = oracle_rays(orc, s["p"], lens, ob, s["inp"][i:i + 1], first_ray=i, lam=float(lambdas[i]), seed=SEED)
            out[i], tries[i] = o[0], t[0]
    finally:
        orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    out.setflags(write=False)
    tries.setflags(write=False)
    return out, tries


def ray_tables(orc, name):
    """set_bokeh's tables of a case (None: it has none)"""
    return _bokeh_tables(orc)[0] if ray_setup(name)["image"] else None


def oracle_ray_case(orc, name):
    """(out, tries) of a ray case: ray i traced at lambdas[i] with id i and SEED"""
    if name not in _ray_oracles:
        s = ray_setup(name)
        _ray_oracles[name] = _rays_at(orc, s, s["lambdas"])
    return _ray_oracles[name]


def oracle_ray_pair(orc, name):
    """((out, tries) with every ray at pair[0], the same at pair[1])"""
    if name not in _ray_pairs:
        s = ray_setup(name)
        n = s["inp"].shape[0]
        _ray_pairs[name] = tuple(_rays_at(orc, s, np.full(n, lam)) for lam in s["pair"])
    return _ray_pairs[name]


# ---- points --------------------------------------------------------------------------------------------------------------------
POINT_LENSES = {
    # name: (lens, what to pass to set_lens_mode, the path trace_points_path must report)
    "dg": ("double_gauss_50mm", None, _abi.POINTS_PATH_COMPILED_IN),
    "petzval": ("petzval_58mm", None, _abi.POINTS_PATH_COMPILED_IN),
    "dg-interpreter": ("double_gauss_50mm", 1, _abi.POINTS_PATH_INTERPRETER),
}
POINT_ATTEMPTS = (1, 64, 65, 130)                      # a one-lane slab, an exact one, the step into a second, a third
N_POINTS = 9
N_CANDIDATES = 600
K_PROBE = 8
POINT_CASES = ["%s/k%d" % (lens, k) for lens in sorted(POINT_LENSES) for k in POINT_ATTEMPTS]
FRAME = (96, 64)

_point_setups, _point_oracles, _point_pairs = {}, {}, {}


def float32_lambdas(n, seed):
    """n wavelengths uniform in [0.40, 0.70], float32 values widened (what the backward oracle can be asked for)"""
    return np.random.default_rng(seed).uniform(0.40, 0.70, n).astype(np.float32).astype(np.float64)


def trace_queries(orc, p, table, cs, px, py, first, k, lambdas):
    """orc_trace_ray_bw_po over n points x k attempts, point j at lambdas[j] (0: p.lambda_bw) -> dict as
    trace_point_cases.oracle_po's: ok, tries, sensor, xy, pixel"""
    n = cs.shape[0]
    lens = orc.orc_lens_create(C.byref(table))
    ok, tries, sensor = np.zeros((n, k), bool), np.zeros((n, k), np.int32), np.full((n, k, 2), np.nan)
    sp, tr = (C.c_double * 2)(), C.c_int()
    try:
        for i in range(n):
            target = oracle_lib.darr(-float(cs[i, 0]) * 10.0, -float(cs[i, 1]) * 10.0, -float(cs[i, 2]) * 10.0)
            lam = float(lambdas[i]) if lambdas[i] != 0.0 else p.lambda_bw
            assert float(np.float32(lam)) == lam
            f0 = int(first[i]) if first is not None else 0
            for m in range(k):
                ok[i, m] = orc.orc_trace_ray_bw_po(C.byref(p), lens, None, target, sp, int(px[i]), int(py[i]), f0 + m, lam, C.byref(tr))
                tries[i, m] = tr.value
                if ok[i, m]:
                    sensor[i, m] = sp[0], sp[1]
    finally:
        orc.orc_lens_destroy(lens)
    xy, pixel = tc.pixel_mapping(p, sensor)
    o = dict(ok=ok, tries=tries, sensor=sensor, xy=xy, pixel=np.where(ok, pixel, tc.VIGNETTED).astype(np.uint32))
    for a in o.values():
        a.setflags(write=False)
    return o


def draw_points(p, n, seed, frame=FRAME):
    """n scene points as tests/trace_point_cases.py draws them -> (cs float32 [n, 3], px, py int32 [n], first uint32 [n])"""
    rng = np.random.default_rng(seed)
    target = np.stack([rng.uniform(-600, 600, n), rng.uniform(-400, 400, n), rng.uniform(500, 5000, n)], 1)
    px = rng.integers(0, frame[0], n).astype(np.int32)
    py = rng.integers(0, frame[1], n).astype(np.int32)
    first = rng.integers(0, 3000, n).astype(np.uint32)
    return np.ascontiguousarray((-target / 10.0).astype(np.float32)), px, py, first


_chosen = {}


def _chosen_points(orc, lens, k, pair):
    """Nine points are too few to meet a query whose try count depends on the wavelength by chance (one query in a hundred or
    fewer does), and a point that no attempt gets through at either wavelength says nothing about the wavelength.  So the
    points are chosen: N_CANDIDATES drawn points are probed with their first min(k, K_PROBE) attempts at the pair's two
    wavelengths; those whose probed attempts all get through at both are kept, and of these the first two whose try counts
    differ between the two go in, then the first seven others."""
    key = (lens, k)
    if key not in _chosen:
        p, model, table, keep = common.po_setup(FRAME[0], FRAME[1], lens=lens)
        cs, px, py, first = draw_points(p, N_CANDIDATES, 100 + k)
        if k != 130:
            first = None                                # (the NULL pointer: attempts from 0)
        probe = [trace_queries(orc, p, table, cs, px, py, first, min(k, K_PROBE), np.full(N_CANDIDATES, lam)) for lam in pair]
        through = probe[0]["ok"].all(1) & probe[1]["ok"].all(1)
        moved = np.nonzero(through & (probe[0]["tries"] != probe[1]["tries"]).any(1))[0][:2]
        assert moved.size == 2, "fewer than two candidates whose try counts depend on the wavelength"
        rest = np.setdiff1d(np.nonzero(through)[0], moved)[:N_POINTS - 2]
        pick = np.sort(np.concatenate([moved, rest]))
        assert pick.size == N_POINTS
        _chosen[key] = (p, table, keep, np.ascontiguousarray(cs[pick]), px[pick], py[pick], None if first is None else first[pick])
    return _chosen[key]


def point_setup(orc, name):
    """dict: p, table, keep, lens_mode, path, cs float32 [9, 3], px, py, pixel uint32 [9], first uint32 [9] or None (the
    NULL pointer, all cases but k130), k, lambdas fp64 [9], pair"""
    if name not in _point_setups:
        lens_name, k = name.split("/k")
        k = int(k)
        lens, lens_mode, path = POINT_LENSES[lens_name]
        lambdas = float32_lambdas(N_POINTS, 200 + k)
        pair = (float(lambdas.min()), float(lambdas.max()))
        p, table, keep, cs, px, py, first = _chosen_points(orc, lens, k, pair)
        s = dict(name=name, p=p, table=table, keep=keep, lens_mode=lens_mode, path=path, cs=cs, px=px, py=py,
                 pixel=tc.pack_pixel(px, py), first=first, k=k, lambdas=lambdas, pair=pair)
        for a in (s["cs"], s["pixel"], s["lambdas"]):
            a.setflags(write=False)
        _point_setups[name] = s
    return _point_setups[name]


def oracle_point_case(orc, name):
    if name not in _point_oracles:
        s = point_setup(orc, name)
        _point_oracles[name] = trace_queries(orc, s["p"], s["table"], s["cs"], s["px"], s["py"], s["first"], s["k"], s["lambdas"])
    return _point_oracles[name]


def oracle_point_pair(orc, name):
    if name not in _point_pairs:
        s = point_setup(orc, name)
        _point_pairs[name] = tuple(trace_queries(orc, s["p"], s["table"], s["cs"], s["px"], s["py"], s["first"], s["k"],
                                                 np.full(N_POINTS, lam)) for lam in s["pair"])
    return _point_pairs[name]
