#!/usr/bin/env python3
"""lentil_hip_last_timing of the thin-lens abb_chromatic > 0 pass (1920x1080, 9 visits per pixel, 256 draws, f_hi = 0.02) in
its two walks: no communicator (tl_chroma_walk_kernel, one block over every item in visit order) and with the library's
communicator (tl_chroma_walk_par_kernel, lentil_tl_chroma_mgpu.h) at world 1, 2 and 4 in bands.  The ranks are threads of
this process on ONE GPU, tests/fake_rccl/libfake_rccl.so standing in for RCCL: at world > 1 they share the device, so their
pass times say nothing about scaling.  Every line carries tl_chroma_stats (items, dependent items, bytes received) and the
generator state after the pass, which must be the same in every mode.  A run is recorded in profiles/tl_chroma_walk_timing.txt.

    python3 tools/tl_chroma_timing.py
"""
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["LENTIL_RCCL_LIB"] = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
import numpy as np
import common
from pota_amd import capi, distributed

W, H, M = 1920, 1080, 9
p = common.tl_setup(W, H, samples_override=256, abb_chromatic=0.6)
t0 = time.time()
visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)
print("stream %.1f s" % (time.time() - t0), flush=True)

def ctx_for(vis):
    c = capi.Context(0)
    c.set_params(p); c.set_bokeh(None); c.alloc_frame(1); c.upload_visits(vis)
    return c

def timed(c, step):
    t = time.time(); step(c); c.sync(); wall = (time.time() - t) * 1e3
    return c.last_timing(), wall

c = ctx_for(visits)
for k in range(2):
    c.clear_frame()
    (ms, wall) = timed(c, lambda x: x.redistribute())
    print("none    pass %d: last_timing %s wall %.1f ms stats %s xor %s" % (k, ms, wall, c.tl_chroma_stats(), c.get_xor128_state()), flush=True)
ref_state = c.get_xor128_state()
c.close()

def slice_cols(idx):
    return {k: ([None if e is None else np.ascontiguousarray(e[idx]) for e in v] if k == "extra" else
                (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v)) for k, v in cols.items()}

for world in (1, 2, 4):
    ctxs, keep = [], []
    for r in range(world):
        b_lo, b_hi = distributed.band_of(r, world, H, p.yres, None)
        sc = slice_cols(slice(b_lo * W * M, min(b_hi, H) * W * M))
        v, kv = capi.make_visits(sc, visits_per_pixel=M, pixels_per_row=W, pixel_y0=b_lo)
        ctxs.append(ctx_for(v)); keep.append((sc, v, kv))
    uid = capi.Context.comm_unique_id()
    res = {}
    def run(r):
        c = ctxs[r]
        c.comm_init(uid, r, world)
        res[r] = []
        for k in range(2):
            t = time.time()
            distributed.frame_step_bands_native(c, H)
            c.sync()
            res[r].append((c.last_timing(), (time.time() - t) * 1e3, c.tl_chroma_stats(), c.get_xor128_state()))
        c.comm_destroy()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th: t.start()
    for t in th: t.join(600)
    for r in range(world):
        for k, (ms, wall, st, xs) in enumerate(res[r]):
            print("world %d rank %d pass %d: last_timing %s step wall %.1f ms stats %s xor %s" % (world, r, k, ms, wall, st, xs), flush=True)
    for c in ctxs: c.close()
