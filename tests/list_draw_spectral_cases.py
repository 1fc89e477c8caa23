"""The case table of the lentil_hip_list_draws_spectral tests (tests/test_gpu_list_draws_spectral.py: the two spectral list
kernels against the oracle and against the scalar call; tests/test_list_draw_spectral_cases.py: the table itself against the
oracle alone, no GPU).  A plain module: no fixtures, fixed seeds; what it computes is computed once per process and never
written to.

A case is a case of tests/list_draw_cases.py ("plain") or of tests/list_draw_probe_cases.py ("probed": with the analytic
sphere), built by their setup() on the smallest frames at which the kernels can still go wrong (32x24 and 48x32, 9 visits per
pixel), with the context's lambda_bw at float32(0.62) -- so that an entry of 0 ("params.lambda_bw") is told from the default
0.55 -- and a wavelength per visit from a palette of four: 0.45, 0.55, 0.65 (float32 values widened: the backward oracle takes a
float) and 0.  Two assignments: "random", a palette entry per visit from a seeded generator, so that the redistributed
neighbours of a 64-visit group differ; and "blocks", constant over three contiguous sub-ranges whose cut points are no
multiples of 64.

The expectation: per distinct wavelength the oracle's single-threaded pass with the draw log kept and p.lambda_bw set to that
wavelength (the probed cases under the sphere), and of each pass the records of the visits that carry that wavelength: four
oracle passes per case.
"""
import ctypes as C

import numpy as np

import common
import list_draw_cases as lc
import list_draw_probe_cases as pc
import oracle_lib
import trace_point_cases as tc

M = lc.M
LAMBDA_BW = float(np.float32(0.62))
PALETTE = (float(np.float32(0.45)), float(np.float32(0.55)), float(np.float32(0.65)), 0.0)
LAM_BLUE, LAM_RED = PALETTE[0], PALETTE[2]
BLOCKS = (LAM_RED, 0.0, LAM_BLUE)           # the "blocks" assignment's three wavelengths, in the order of its sub-ranges

# kind -> the names of the sibling table that are taken over
PLAIN = ("samples-4", "samples-64", "samples-65", "samples-130", "formula", "retries0", "retries15", "short-po", "lens-petzval",
         "lens-anamorphic", "lens-interpreter", "bokeh-image", "moving-camera", "ragged", "tl-plain")
PROBED = ("samples-16", "samples-65", "retries0", "retries3", "swallowed", "edge", "skydome", "lens-anamorphic", "tl-plain")
ALL = [("plain", n) for n in PLAIN] + [("probed", n) for n in PROBED]
IDS = ["%s/%s" % k for k in ALL]
FRAMES = ((32, 24), (48, 32))

_setups, _passes = {}, {}


# What a case changes of its sibling's set-up, so that the wavelength shows in it (tests/test_list_draw_spectral_cases.py asks
# that a quarter of its listed visits differ between 0.45 and 0.65): the chromatic shift is a fraction of a pixel, and a visit
# of four draws rarely shows it on the coarser frame.  samples-4 takes the finer of the two frames.  ragged comes down from
# 64x48 to 48x32, where the reference's formula would leave every count at its floor of 4: bidir_sample_mult is turned up as
# list_draw_cases turns it up for "formula" at this very frame, and the counts differ from visit to visit again.
OVERRIDES = {
    "samples-4": dict(frame=FRAMES[1]),
    "ragged": dict(frame=FRAMES[1], bidir_sample_mult=lc.FORMULA_MULT),
}


def _plain_kw(name):
    """what list_draw_cases._case was given for `name`, with the case's OVERRIDES"""
    c = lc.CASES[name]
    kw = {k: c[k] for k in ("camera", "frame", "samples", "f_hi", "seed", "lens", "lens_mode", "path", "bokeh", "motion", "ragged",
                            "lam", "edge", "unit")}
    kw.update(c["params"])
    kw.update(OVERRIDES.get(name, {}))
    return kw


def setup(kind, name):
    """the sibling table's setup() dict (a copy) with p: lambda_bw = LAMBDA_BW, and kind, key; probed: sphere, c2w, skydome too"""
    key = (kind, name)
    if key in _setups:
        return _setups[key]
    if kind == "plain":
        kw = _plain_kw(name)
        s = dict(pc._lc_setup("spectral:" + name, kw) if name in OVERRIDES else lc.setup(name))
        assert s["lam"] == 0.0
    else:
        s = dict(pc.setup(name))
    assert tuple(s["frame"]) in FRAMES
    p = lc._copy_params(s["p"])
    p.lambda_bw = LAMBDA_BW
    assert float(p.lambda_bw) == LAMBDA_BW and p.abb_chromatic == 0.0
    s.update(p=p, p_oracle=None, kind=kind, key=key, name=name)
    _setups[key] = s
    return s


def cuts(n):
    """the two cut points of the "blocks" assignment over n visits: no multiples of 64"""
    c1, c2 = n // 5 + 13, n // 2 + 77
    assert 0 < c1 < c2 < n and c1 % 64 and c2 % 64
    return c1, c2


def lambdas(kind, name, assignment="random"):
    """float64 [n]: the wavelength of every visit of the case's stream"""
    s = setup(kind, name)
    n = s["n"]
    if assignment == "random":
        which = np.random.default_rng(0x5EC7 ^ (n * 31 + len(name))).integers(0, len(PALETTE), n)
        lam = np.asarray(PALETTE)[which]
    else:
        assert assignment == "blocks"
        c1, c2 = cuts(n)
        lam = np.empty(n)
        lam[:c1], lam[c1:c2], lam[c2:] = BLOCKS
    lam.setflags(write=False)
    return lam


def effective(lam):
    """what an entry means: 0 is the context's lambda_bw"""
    return LAMBDA_BW if lam == 0.0 else float(lam)


def oracle_pass(orc, kind, name, lam):
    """the oracle's single-threaded pass over the case's stream with every visit at `lam` (a palette entry; 0: LAMBDA_BW), the
    probed cases under the sphere -> dict: log uint32 [n, 3] sorted by (visit, attempt), visits / redistributed / attempted /
    accepted (its counters)"""
    s = setup(kind, name)
    eff = effective(lam)
    if s["camera"] == "tl":
        eff = LAMBDA_BW                      # (the thin lens reads no wavelength: one pass serves every entry)
    key = (kind, name, eff)
    if key in _passes:
        return _passes[key]
    p = lc._copy_params(s["p"])
    p.lambda_bw = eff
    assert float(p.lambda_bw) == eff          # a float32 value: the oracle's parameters hold it exactly
    lens = orc.orc_lens_create(C.byref(s["table"])) if s["table"] is not None else None
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    fr = oracle_lib.Frame(orc, p, n_aovs=1, keep_log=True)
    try:
        if s["keys"] is not None:
            fr.set_camera_motion(s["keys"])
        if kind == "probed":
            rec = pc.Recorder(oracle_lib.sphere_occluder(orc), s["sphere"].ctypes.data)
            fr.set_probe(rec.address, None, s["c2w"])
        fr.run(lens, ob, s["visits"])
        c = fr.counters()
        o = dict(log=common.sort_log(fr.log()), visits=int(c.visits), redistributed=int(c.redistributed_visits),
                 attempted=int(c.attempted_draws), accepted=int(c.accepted_draws))
    finally:
        fr.close()
        if lens:
            orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    o["log"].setflags(write=False)
    _passes[key] = o
    return o


def expected_log(orc, kind, name, lam):
    """the draw log of the pass in which visit v is at lam[v]: of every distinct wavelength's pass the records of the visits
    that carry it -> uint32 [k, 3] sorted by (visit, attempt)"""
    parts = []
    for value in np.unique(lam):
        log = oracle_pass(orc, kind, name, float(value))["log"]
        parts.append(log[lam[log[:, 0]] == value])
    log = common.sort_log(np.concatenate(parts)) if parts else np.zeros((0, 3), np.uint32)
    return log


def attempts_per_visit(log, red, samples):
    """the attempts every redistributed visit made, from its records and its draw count: up to its last accepted draw if that
    was the `samples`-th, else all 5 * samples.  log: sorted; red: the redistributed visits (sorted); samples: theirs
    -> int64 [red.size]"""
    samples = np.asarray(samples, np.int64)
    made = 5 * samples
    vis, count, last, _ = lc.per_visit(log)
    assert np.isin(vis, red).all()
    at = np.searchsorted(red, vis)
    full = count == samples[at]
    made[at[full]] = last[full] + 1
    return made


def trace_records(orc, s, cs, pixel, visit, seed, lam):
    """orc_trace_ray_bw_po once per record: the point cs[i] (camera space, centimetres: plan_visits' cs), the source pixel
    pixel[i] (px | py << 16), the seed seed[i], the wavelength lam[visit[i]] (0: LAMBDA_BW) -> dict: ok, tries, xy fp64 [k, 2],
    pixel uint32 [k] (trace_point_cases.pixel_mapping over the sensor position)"""
    p = s["p"]
    k = len(visit)
    lens = orc.orc_lens_create(C.byref(s["table"]))
    ob = None
    if s["bokeh"]:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, s["bokeh"])
    ok, tries, sensor = np.zeros(k, bool), np.zeros(k, np.int32), np.full((k, 2), np.nan)
    sp, tr = (C.c_double * 2)(), C.c_int()
    try:
        for i in range(k):
            target = oracle_lib.darr(-float(cs[i, 0]) * 10.0, -float(cs[i, 1]) * 10.0, -float(cs[i, 2]) * 10.0)
            ok[i] = orc.orc_trace_ray_bw_po(C.byref(p), lens, ob, target, sp, int(pixel[i] & 0xFFFF), int(pixel[i] >> 16), int(seed[i]),
                                            effective(lam[visit[i]]), C.byref(tr))
            tries[i] = tr.value
            if ok[i]:
                sensor[i] = sp[0], sp[1]
    finally:
        orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    xy, pix = tc.pixel_mapping(p, sensor)
    return dict(ok=ok, tries=tries, xy=xy, pixel=np.where(ok, pix, tc.VIGNETTED).astype(np.uint32))


def visit_differences(a, b):
    """two sorted logs of one stream -> (visits listed in either, those whose records differ in an accepted attempt or a pixel,
    those whose sets of accepted attempts differ)"""
    def by_visit(log):
        vis, first, count = np.unique(log[:, 0], return_index=True, return_counts=True)
        return {int(v): log[f:f + c, 1:] for v, f, c in zip(vis, first, count)}
    da, db = by_visit(a), by_visit(b)
    listed = sorted(set(da) | set(db))
    empty = np.zeros((0, 2), np.uint32)
    differ = [v for v in listed if not np.array_equal(da.get(v, empty), db.get(v, empty))]
    attempts = [v for v in listed if not np.array_equal(da.get(v, empty)[:, 0], db.get(v, empty)[:, 0])]
    return listed, differ, attempts
