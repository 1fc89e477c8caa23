#!/usr/bin/env python3
"""What LENTIL_DRAWS_PROBED costs: lentil_hip_list_draws over one stream without the flag, with it
under a host callback and with it under a device callback -- the analytic sphere of the tests both times
(orc_sphere_occluder on the CPU, lentil_hip_test_sphere_occluder_device on the GPU).  96 x 64 frame, 9 visits per pixel, 2 %
highlights, polynomial-optics double gauss, samples_override = 130.  Device pointers for the records, the list sized from
the plan's totals[2].  Every figure: one warm-up call, then the median of --repeats calls, wall time around the call (it
returns when the list is complete).  The turns and the length of every turn's list come from one more, untimed call under a
recording host callback.

    python3 tools/list_draws_probed_timing.py [--repeats 6] [--out profiles/list_draws_probed.txt]
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
from pota_amd import capi  # noqa: E402
sys.path.insert(1, os.path.join(ROOT, "tests"))
import common  # noqa: E402
import oracle_lib  # noqa: E402

W, H, M, S = 96, 64, 9, 130
SPHERE = np.array([6.0, 2.0, -70.0, 9.0], np.float32)
PROBE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)


def timed(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    orc = oracle_lib.load()
    p, model, table, keep = common.po_setup(W, H, samples_override=S)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)
    ctx = capi.Context(0)
    ctx.set_params(p)
    ctx.set_lens(table)
    ctx.upload_visits(visits)
    plan, totals = ctx.plan_visits()
    cap = totals[2]
    lines = ["list_draws with and without LENTIL_DRAWS_PROBED: %d x %d, %d visits per pixel, samples_override %d; %d visits, %d redistributed, "
             "totals[2] = %d; median of %d (min-max), ms" % (W, H, M, S, totals[0], totals[1], totals[2], a.repeats)]

    def row(tag, probed):
        before = ctx.probe_stats()
        got = ctx.list_draws(capacity=cap, device=True, probed=probed)
        after = ctx.probe_stats()
        med, lo, hi = timed(lambda: ctx.list_draws(capacity=cap, device=True, probed=probed), a.repeats)
        d = tuple(x - y for x, y in zip(after, before))
        lines.append("%-28s %9.3f (%.3f-%.3f)   draws %d attempts %d   segments %d occluded %d turns %d"
                     % (tag, med, lo, hi, got[1], got[2], d[0], d[1], d[2]))
        return med, d

    free_ms, _ = row("unprobed", False)
    ctx.set_occlusion_probe(oracle_lib.sphere_occluder(orc), SPHERE.ctypes.data)
    host_ms, d = row("probed, host callback", True)
    ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), SPHERE.ctypes.data)
    dev_ms, _ = row("probed, device callback", True)
    lines.append("host / unprobed %.1f x, device / unprobed %.1f x; over PCIe per call under the host callback: %d B out, %d B back"
                 % (host_ms / free_ms, dev_ms / free_ms, 24 * d[0], d[0]))
    # the turns: one untimed call under a callback that notes every list's length
    inner, seen = PROBE_FN(oracle_lib.sphere_occluder(orc)), []

    def note(user, n, seg, occ):
        inner(SPHERE.ctypes.data, n, seg, occ)
        seen.append(int(n))

    fn = PROBE_FN(note)
    ctx.set_occlusion_probe(C.cast(fn, C.c_void_p).value, None)
    ctx.list_draws(capacity=cap, device=True, probed=True)
    lines.append("list lengths by turn: %s" % seen)
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
