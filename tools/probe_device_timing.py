#!/usr/bin/env python3
"""What occlusion probes cost a chunked pass under the host callback and under the device callback:
a 1920x1080 polynomial-optics frame, 9 visits per pixel, samples_override = 256, 2 % highlights, behind the tests' sphere.
Times the second and later passes (the first sizes the buffers): mean, min, max and standard deviation of the wall time of
clear + redistribute + sync, segments per pass, lentil_hip_probe_device_stats, and for the host form the time spent inside
the callback.  The host callback is the test oracle's analytic sphere, the device callback the library's own.  A run is
recorded in profiles/probe_device.txt.

    python3 tools/probe_device_timing.py --mode host|device [--passes 24] [--label TEXT]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(q, "pota_amd")) for q in sys.path if q):
    sys.path.insert(0, ROOT)
from pota_amd import capi  # noqa: E402  (before tests/common puts the repository's root in front)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import common  # noqa: E402

W, H, M, S = 1920, 1080, 9, 256
SPHERE = np.array([6.0, 2.0, -70.0, 9.0], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["host", "device"], required=True)
    ap.add_argument("--passes", type=int, default=24)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    p, model, table, keep = common.po_setup(W, H, samples_override=S)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)
    ctx = capi.Context(0)
    ctx.set_params(p); ctx.set_lens(table); ctx.set_bokeh(None); ctx.alloc_frame(1)
    spent = [0.0]
    if a.mode == "host":
        import oracle_lib          # (the host "renderer" is the test oracle's analytic sphere; the device mode needs no oracle)
        orc = oracle_lib.load()
        fn_t = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)
        inner = fn_t(oracle_lib.sphere_occluder(orc))

        def timed(user, n, seg, occluded):
            t = time.perf_counter()
            inner(user, n, seg, occluded)
            spent[0] += time.perf_counter() - t

        cb = fn_t(timed)
        ctx.set_occlusion_probe(C.cast(cb, C.c_void_p).value, SPHERE.ctypes.data)
    else:
        ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), SPHERE.ctypes.data)
    ctx.upload_visits(visits)
    ms, inside, seg = [], [], []
    for k in range(a.passes + 1):
        before, spent[0] = ctx.probe_stats(), 0.0
        ctx.sync()
        t = time.perf_counter()
        ctx.clear_frame(); ctx.redistribute(); ctx.sync()
        dt = (time.perf_counter() - t) * 1e3
        c = ctx.counters()
        assert c.worklist_overflow == 0 and c.streamed == 0
        if k:
            ms.append(dt); inside.append(spent[0] * 1e3); seg.append(ctx.probe_stats()[0] - before[0])
        else:
            print("first pass %.1f ms (sizes the buffers; not in the mean)" % dt, flush=True)
    ms = np.array(ms)
    dev = ctx.probe_device_stats() if hasattr(ctx, "probe_device_stats") else None
    print("%s%s: %d passes: %.2f ms per pass (min %.2f max %.2f sd %.2f) | segments per pass %d | occluded of all %d / %d | callbacks %d | "
          "inside the host callback %.2f ms per pass | blind chunks %d fallback chunks %d | probe_device_stats %s | accepted %d" %
          (a.mode, " " + a.label if a.label else "", len(ms), ms.mean(), ms.min(), ms.max(), ms.std(), int(np.mean(seg)),
           ctx.probe_stats()[1], ctx.probe_stats()[0], ctx.probe_stats()[2], float(np.mean(inside)), c.blind_chunks, c.fallback_chunks, dev,
           c.accepted_draws), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
