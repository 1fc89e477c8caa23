#!/usr/bin/env python3
"""What occlusion probes cost a thin-lens abb_chromatic > 0 pass (tl_chroma_probe in pota_amd/csrc/lentil_hip.hip): per frame
and pass the turns of the probe loop (= callbacks), the segments asked about against the attempts the pass makes (the
reference probes each attempt it makes once: the counters' attempted_draws, which the tests pin to the oracle's), the wall
time of the pass and the part of it spent inside the callback -- the oracle's analytic sphere, the host's time, not the
library's -- beside the same frame's unprobed chromatic pass and its probed abb_chromatic = 0 pass.  No communicator.
A run is recorded in profiles/tl_chroma_probe.txt.

    python3 tools/tl_chroma_probe_timing.py [--oracle]      (--oracle: also run the single-threaded oracle on every frame)
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import common
import oracle_lib
from pota_amd import capi

orc = oracle_lib.load()
SPHERE = np.array([6.0, 2.0, -70.0, 9.0], np.float32)
FN_T = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)
inner = FN_T(oracle_lib.sphere_occluder(orc))
spent = [0.0]


def timed_cb(user, n, seg, occ):
    t = time.perf_counter()
    inner(user, n, seg, occ)
    spent[0] += time.perf_counter() - t


CB = FN_T(timed_cb)
PROBE = (C.cast(CB, C.c_void_p).value, SPHERE.ctypes.data)


def passes(p, visits, probe, label, n=3):
    c = capi.Context(0)
    c.set_params(p); c.set_bokeh(None); c.alloc_frame(1)
    if probe:
        c.set_occlusion_probe(*probe)
    c.upload_visits(visits)
    for k in range(n):
        before, spent[0] = c.probe_stats(), 0.0
        c.clear_frame(); c.sync()
        t = time.perf_counter()
        c.redistribute(); c.sync()
        wall = (time.perf_counter() - t) * 1e3
        asked, occluded, calls = (a - b for a, b in zip(c.probe_stats(), before))
        ct = c.counters()
        line = "  %-28s pass %d: %9.2f ms wall" % (label, k, wall)
        if probe:
            line += ", %8.2f ms in the callback; %3d callbacks, %9d segments asked (%d occluded)" % (spent[0] * 1e3, calls, asked, occluded)
            line += "; attempts made %d, accepted %d, asked / attempts %.5f" % (ct.attempted_draws, ct.accepted_draws,
                                                                             asked / max(1, ct.attempted_draws))
        else:
            line += "; attempts made %d, accepted %d" % (ct.attempted_draws, ct.accepted_draws)
        print(line, flush=True)
    c.close()


def frame(name, W, H, with_oracle, n=3, **kw):
    M = 9
    p = common.tl_setup(W, H, samples_override=48, abb_chromatic=0.6, **kw)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)
    print("%s (%dx%d, %d visits per pixel, samples_override 48)" % (name, W, H, M), flush=True)
    if with_oracle:
        ref = oracle_lib.Frame(orc, p, n_aovs=1, keep_log=False)
        ref.set_probe(oracle_lib.sphere_occluder(orc), SPHERE.ctypes.data)
        t = time.perf_counter()
        ref.run(None, None, visits)
        rc = ref.counters()
        print("  oracle, single-threaded, probed: %d probe calls (attempted_draws), %d accepted, %.1f s" %
              (rc.attempted_draws, rc.accepted_draws, time.perf_counter() - t), flush=True)
        ref.close()
    passes(p, visits, PROBE, "chromatic, probed", n)
    passes(p, visits, None, "chromatic, no probe", n)
    p0 = common.tl_setup(W, H, samples_override=48, **{k: v for k, v in kw.items() if k != "abb_chromatic_type"})
    passes(p0, visits, PROBE, "abb_chromatic = 0, probed", n)


if __name__ == "__main__":
    with_oracle = "--oracle" in sys.argv[1:]
    frame("green-magenta", 96, 64, with_oracle, abb_chromatic_type=0)
    frame("red-cyan + coma + vignetting", 96, 64, with_oracle, abb_chromatic_type=1, abb_coma=0.35, optical_vignetting_distance=2.0,
          optical_vignetting_radius=1.5)
    frame("green-magenta 1080p", 1920, 1080, with_oracle, n=2, abb_chromatic_type=0)
