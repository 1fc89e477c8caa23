"""The batches of the lentil_hip_trace_points_probed tests (tests/test_gpu_trace_points_probed.py: the kernel against the
oracle's probed pass, the unprobed call, the probed list and an exact model; tests/test_trace_point_probe_cases.py: the table
itself against the oracle alone, no GPU).  A plain module: no fixtures, fixed seeds; what it computes is computed once per
process and never written to.

It builds on tests/list_draw_probe_cases.py (`pc`): the same cases, spheres, setup() and oracle_pass().  A case's batch has one
point per redistributed visit of its stream and K = the largest 5 * samples of them attempts per point: query (point, m) is
attempt m of that visit.

Where cs and pixel come from.  The model cases (pc.MODEL: a static camera at the origin, centimetres, polynomial optics) read
them off the columns as tests/trace_point_cases.py does for its pass comparison: the world-to-camera matrix is the identity,
so cs is pos_z.xyz; the redistributed visits are the stream's highlights (test_trace_point_probe_cases.py checks the count
against the oracle's).  Every other case (a moved or moving camera, another unit, the thin lens) takes them from the plan of
lentil_hip_plan_visits -- the library's visit prologue, which tests/test_gpu_list_draws.py holds to the oracle's -- and the
GPU test checks that the two sources agree where both exist.
"""
import collections
import ctypes as C

import numpy as np

import list_draw_cases as lc
import list_draw_probe_cases as pc
import oracle_lib
import trace_point_cases as tc
from pota_amd import _abi

M = pc.M
VIGNETTED, OUTSIDE = _abi.POINT_VIGNETTED, _abi.POINT_OUTSIDE
ORACLE_MODEL = ("samples-4", "retries0", "retries3", "swallowed", "no-dof")       # small enough for the oracle, seed by seed
AI_EPSILON, AI_INFINITE = np.float32(1.0e-4), np.float32(1.0e30)

_batches, _models = {}, {}


def from_skydome(pos_z):
    """sample_is_from_skydome (src/lentil_filter.cpp:119-133) over the pos_z column -> uint8 [n]"""
    small = (np.abs(pos_z[:, :3]) < AI_EPSILON).all(axis=1)
    return ((pos_z[:, 3].astype(np.float64) == np.float64(AI_INFINITE)) | small).astype(np.uint8)


def batch(name, plan=None):
    """dict: visits int64 [n] (the redistributed visits), cs float32 [n, 3], pixel uint32 [n], origin float32 [n, 3], time
    float32 [n], exempt uint8 [n], samples int64 [n], k.  plan: lentil_hip_plan_visits' records of the whole stream; None: from
    the columns (model cases with a samples_override)."""
    key = (name, plan is not None)
    if key in _batches:
        return _batches[key]
    s = pc.setup(name)
    cols = s["cols"]
    if plan is None:
        assert s["model"] and s["samples"] > 0
        red = np.nonzero(s["highlights"])[0]
        cs = np.ascontiguousarray(cols["pos_z"][red, :3])
        if "pixel" in cols:
            pixel = np.ascontiguousarray(cols["pixel"][red])
        else:
            pix = red // M
            pixel = tc.pack_pixel(pix % s["frame"][0], pix // s["frame"][0])
        samples = np.full(red.size, s["samples"], np.int64)
    else:
        red = np.nonzero(plan["flags"] & _abi.PLAN_REDISTRIBUTE)[0]
        cs = np.ascontiguousarray(plan["cs"][red])
        pixel = np.ascontiguousarray(plan["pixel"][red])
        samples = plan["samples"][red].astype(np.int64)
    b = dict(name=name, visits=red.astype(np.int64), cs=cs, pixel=pixel, origin=np.ascontiguousarray(cols["pos_z"][red, :3]),
             time=np.ascontiguousarray(cols["raydir_time"][red, 3]), exempt=np.ascontiguousarray(from_skydome(cols["pos_z"][red])),
             samples=samples, k=int(samples.max()) * 5 if red.size else 1)
    for a in b.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _batches[key] = b
    return b


def segments(orc, s, b, n_seeds, first=0):
    """the segments of seeds first ... first + n_seeds - 1 of every point of a model case (identity camera, centimetres: the
    aperture point is the target as it stands), as _model of tests/test_gpu_list_draws_probed.py forms them, and the sphere's
    answers -> (seg float32 [n, n_seeds, 6], occ bool [n, n_seeds])"""
    p = s["p"]
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    n = b["cs"].shape[0]
    seg = np.zeros((n, n_seeds, 6), np.float32)
    seg[:, :, :3] = b["origin"][:, None, :]
    ap = (C.c_double * 2)()
    for i in range(n):
        px, py = int(b["pixel"][i] & 0xFFFF), int(b["pixel"][i] >> 16)
        for j in range(n_seeds):
            orc.orc_po_aperture_sample(C.byref(p), ob, (px * py + px) & 0xFFFFFFFF, (first + j) & 0xFFFFFFFF, ap)
            seg[i, j, 3] = np.float32(-ap[0] * 0.1)
            seg[i, j, 4] = np.float32(-ap[1] * 0.1)
    seg += np.float32(0.0)                                        # (-0 -> +0, as the matrix product's sums leave it)
    if ob:
        orc.orc_bokeh_destroy(ob)
    occ = np.zeros(n * n_seeds, np.uint8)
    flat = np.ascontiguousarray(seg.reshape(-1, 6))
    if flat.shape[0]:
        orc.orc_sphere_occluder(C.c_void_p(s["sphere"].ctypes.data), C.c_uint64(flat.shape[0]), C.c_void_p(flat.ctypes.data),
                                C.c_void_p(occ.ctypes.data))
    return seg, occ.reshape(n, n_seeds).astype(bool)


def walk(passes, occ, k, retries):
    """the reference's try loop (src/lentil.h:573-661 under a probe) over per-seed facts: passes / occ bool [n, k + max(retries,
    0)] -> dict: tries int32 [n, k] (the failed tries: all retries + 1 of them where no seed passes), hit int64 [n, k] (the
    passing seed's offset, -1: none), asked bool [n, seeds] (the seeds some query reaches and the lens lets through)"""
    n = passes.shape[0]
    tries = np.zeros((n, k), np.int32)
    hit = np.full((n, k), -1, np.int64)
    asked = np.zeros(passes.shape, bool)
    live = np.ones((n, k), bool)
    cols = np.arange(k)[None, :]
    for t in range(max(retries + 1, 0)):
        through = live & passes[:, t:t + k]
        asked[:, t:t + k] |= through
        got = through & ~occ[:, t:t + k]
        hit = np.where(got, cols + t, hit)
        live &= ~got
        tries[live] += 1
    return dict(tries=tries, hit=hit, asked=asked)


def oracle_model(orc, name):
    """A small model case seed by seed, from the oracle alone -> dict: k, retries, passes / occ bool [n, seeds], sensor fp64
    [n, seeds, 2], seg float32 [n, seeds, 6], free_tries int32 [n, k] (orc_trace_ray_bw_po's own tries: no probe), and walk()'s
    tries / hit / asked, and xy fp64 [n, k, 2] / pixel uint32 [n, k] of the passing seeds (VIGNETTED where none)."""
    if name in _models:
        return _models[name]
    assert name in ORACLE_MODEL
    s, b = pc.setup(name), batch(name)
    p = s["p_oracle"]
    retries = int(p.vignetting_retries)
    k, n = b["k"], b["cs"].shape[0]
    seeds = k + max(retries, 0)
    p0 = lc._copy_params(p)
    p0.vignetting_retries = 0                                      # one try: the seed's own outcome in the lens
    lens = orc.orc_lens_create(C.byref(s["table"]))
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    passes = np.zeros((n, seeds), bool)
    sensor = np.full((n, seeds, 2), np.nan)
    free_tries = np.zeros((n, k), np.int32)
    sp, tr = (C.c_double * 2)(), C.c_int()
    try:
        for i in range(n):
            cs = b["cs"][i]
            target = oracle_lib.darr(-float(cs[0]) * 10.0, -float(cs[1]) * 10.0, -float(cs[2]) * 10.0)
            px, py = int(b["pixel"][i] & 0xFFFF), int(b["pixel"][i] >> 16)
            for m in range(seeds):
                passes[i, m] = bool(orc.orc_trace_ray_bw_po(C.byref(p0), lens, ob, target, sp, px, py, m, p.lambda_bw, C.byref(tr)))
                if passes[i, m]:
                    sensor[i, m] = sp[0], sp[1]
            for m in range(k):
                orc.orc_trace_ray_bw_po(C.byref(p), lens, ob, target, sp, px, py, m, p.lambda_bw, C.byref(tr))
                free_tries[i, m] = tr.value
    finally:
        orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    seg, occ = segments(orc, s, b, seeds)
    o = dict(k=k, retries=retries, passes=passes, occ=occ, sensor=sensor, seg=seg, free_tries=free_tries)
    o.update(walk(passes, occ, k, retries))
    got = o["hit"] >= 0
    at = np.where(got, o["hit"], 0)
    sen = np.where(got[..., None], np.take_along_axis(sensor, at[..., None].repeat(2, -1), axis=1), np.nan)
    xy, pixel = tc.pixel_mapping(p, sen)
    o["xy"], o["pixel"] = xy, np.where(got, pixel, VIGNETTED).astype(np.uint32)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _models[name] = o
    return o


def made(inside, samples):
    """the attempts the reference makes of every point (while accepted < samples and attempt < 5 * samples) given which
    queries land in the frame: inside bool [n, k], samples [n] -> int64 [n]"""
    acc = np.cumsum(inside, axis=1)
    full = acc >= samples[:, None]
    return np.where(full.any(axis=1), full.argmax(axis=1) + 1, 5 * samples).astype(np.int64)


def made_from_log(log, visits, samples):
    """the same from a pass's draw log: a visit with `samples` records stopped behind its last one, every other ran to
    5 * samples -> (made int64 [n], landed uint32 [n, k]: the logged pixel, VIGNETTED where (visit, attempt) is not in the log)"""
    k = int(samples.max()) * 5 if visits.size else 1
    idx = np.searchsorted(visits, log[:, 0])
    assert log.shape[0] == 0 or (idx < visits.size).all() and (visits[idx] == log[:, 0]).all()
    landed = np.full((visits.size, k), VIGNETTED, np.uint32)
    landed[idx, log[:, 1]] = log[:, 2]
    count = np.bincount(idx, minlength=visits.size)
    last = np.full(visits.size, -1, np.int64)
    np.maximum.at(last, idx, log[:, 1].astype(np.int64))
    return np.where(count >= samples, last + 1, 5 * samples).astype(np.int64), landed


def asked_counter(seg, asked):
    """the asked segments as a multiset of 24-byte rows"""
    return collections.Counter(row.tobytes() for row in seg[asked])
