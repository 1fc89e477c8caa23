"""The case table of the spectral pass's tests (tests/test_gpu_spectral_pass.py: lentil_hip_redistribute with a wavelength per
visit, lentil_hip_set_visit_lambdas, against the oracle; tests/test_spectral_pass_cases.py: the expectation itself, no GPU).
A plain module: no fixtures, fixed seeds; what it computes is computed once per process and never written to.

A case is (kind, name, assignment): a case of tests/list_draw_spectral_cases.py -- its frames, 32x24 and 48x32 with 9 visits per
pixel and 4-130 draws, are the smallest at which the pass's solve kernel can go wrong: tasks of fewer than 64 seeds, of exactly
64, several tasks per item, items of a 64-visit group at different wavelengths -- with one of that module's two assignments of
a wavelength to every visit.

The expectation.  orc_redistribute takes a visit range and accumulates into the frame it is given, so the oracle's
single-threaded pass in which visit v is at lam[v] is the stream run in runs of equal entries, with the frame's parameters'
lambda_bw set to the run's wavelength (an entry of 0: the context's lambda_bw): one frame -- log, accumulators, weights,
counters.  The probed cases run under the analytic sphere."""
import ctypes as C

import numpy as np

import list_draw_cases as lc
import list_draw_probe_cases as pc
import list_draw_spectral_cases as ls
import oracle_lib

ASSIGNMENTS = ("random", "blocks")
ALL = [(kind, name, a) for kind, name in ls.ALL for a in ASSIGNMENTS]
IDS = ["%s/%s/%s" % c for c in ALL]
PLAIN = [c for c in ALL if c[0] == "plain"]
PROBED = [c for c in ALL if c[0] == "probed"]

_frames = {}


def ids(cases):
    return ["%s/%s/%s" % c for c in cases]


def runs(lam):
    """the runs of equal entries of a column -> [(v0, v1, entry)]"""
    lam = np.asarray(lam, np.float64)
    if lam.size == 0:
        return []
    cut = np.flatnonzero(lam[1:] != lam[:-1]) + 1
    begin = np.concatenate([[0], cut])
    end = np.concatenate([cut, [lam.size]])
    return [(int(a), int(b), float(lam[a])) for a, b in zip(begin, end)]


def oracle_run(orc, p, table, visits, lam, n_aovs=1, kinds=None, bokeh=None, keys=None, probe=None):
    """the oracle's single-threaded pass over `visits` with visit v at lam[v] (0: p.lambda_bw), run by run into one
    oracle_lib.Frame with the draw log kept.  p is copied; bokeh: a case of tests/bokeh_tables.py or None; keys: camera motion
    keys or None; probe: (sphere float32 [4], camera_to_world or None) or None.  The caller closes the frame."""
    assert len(lam) == int(visits.n)
    own = lc._copy_params(p)
    bw = float(p.lambda_bw)
    lens = orc.orc_lens_create(C.byref(table)) if table is not None else None
    ob = None
    if bokeh:
        import bokeh_tables
        ob = bokeh_tables.oracle_bokeh(orc, bokeh)
    fr = oracle_lib.Frame(orc, own, n_aovs=n_aovs, kinds=kinds, keep_log=True)
    try:
        if keys is not None:
            fr.set_camera_motion(keys)
        if probe is not None:
            sphere, c2w = probe
            fr._recorder = pc.Recorder(oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
            fr.set_probe(fr._recorder.address, None, c2w)
        for v0, v1, entry in runs(lam):
            fr.params.lambda_bw = bw if entry == 0.0 else entry
            assert float(fr.params.lambda_bw) == (bw if entry == 0.0 else entry)      # a float32 value: held exactly
            fr.run(lens, ob, visits, v0, v1)
        fr.params.lambda_bw = bw
    except Exception:
        fr.close()
        raise
    finally:
        if lens:
            orc.orc_lens_destroy(lens)
        if ob:
            orc.orc_bokeh_destroy(ob)
    return fr


def column(case):
    kind, name, assignment = case
    return ls.lambdas(kind, name, assignment)


def oracle_frame(orc, case, n_aovs=1, kinds=None, lam=None):
    """the oracle's frame of a case (kept for the process; nobody closes or writes to it).  lam: another column than the
    case's own (not kept: the caller closes that frame)."""
    kind, name, assignment = case
    s = ls.setup(kind, name)
    key = (case, n_aovs, tuple(kinds) if kinds else None)
    if lam is None and key in _frames:
        return _frames[key]
    fr = oracle_run(orc, s["p"], s["table"], s["visits"], column(case) if lam is None else lam, n_aovs=n_aovs, kinds=kinds,
                    bokeh=s["bokeh"], keys=s["keys"], probe=(s["sphere"], s["c2w"]) if kind == "probed" else None)
    if lam is None:
        _frames[key] = fr
    return fr


def alternating(n):
    """a column at one effective wavelength that cuts the stream into single visits: 0 and LAMBDA_BW in turn"""
    lam = np.zeros(n)
    lam[1::2] = ls.LAMBDA_BW
    return lam
