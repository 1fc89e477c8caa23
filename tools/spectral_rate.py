#!/usr/bin/env python3
"""What the spectral batch calls cost beside the scalar ones: recorded, not gated.

Rays: the batch of tools/camera_rays_rate.py (3840 x 2160 uniformly random camera samples, double gauss, device-resident),
through the table interpreter and through the compiled-in kernel (a context created with LENTIL_RAYS_COMPILED=1).
Points: the batch of tools/trace_points_timing.py (the 1920 x 1080 frame of DESIGN.md 4.7: every visit a one-sample pass logs
a draw for, K = 256 attempts, out_pixel + out_xy, device pointers), through the compiled-in lens and the table interpreter.
Each is timed three ways: the scalar call, the spectral call with every wavelength equal to the scalar one, the spectral
call with wavelengths uniform in [0.40, 0.70] um.  One process, one box; events on the context's stream around each call;
one warm-up call, then the median of six.

    python3 tools/spectral_rate.py [--out profiles/spectral_rate.txt] [--rays-only | --points-only]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(q, "pota_amd")) for q in sys.path if q):
    sys.path.insert(0, ROOT)
from pota_amd import camera, capi, lens_io  # noqa: E402
sys.path.insert(1, os.path.join(ROOT, "tests"))
import common  # noqa: E402

RAYS_W, RAYS_H = 3840, 2160
W, H, M, K = 1920, 1080, 9, 256
WARMUP, REPS = 1, 6
SEED = 0x5EED
LAM = float(np.float32(550.0)) * 0.001
LAM_RANGE = (0.40, 0.70)


def timed(torch, ctx, call):
    """median, min, max ms of REPS calls after WARMUP, by events on the context's stream"""
    stream = torch.cuda.ExternalStream(ctx.stream())
    for _ in range(WARMUP):
        call()
    ctx.sync()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = call()
        b.record(stream)
        ctx.sync()
        ms.append(a.elapsed_time(b))
        del out
    ms.sort()
    return (ms[REPS // 2 - 1] + ms[REPS // 2]) / 2, ms[0], ms[-1]


def three_ways(torch, say, ctx, what, unit, count, scalar, spectral, n):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    equal = torch.full((n,), LAM, dtype=torch.float64, device=dev)
    spread = (torch.rand((n,), dtype=torch.float64, device=dev, generator=g) * (LAM_RANGE[1] - LAM_RANGE[0]) + LAM_RANGE[0]).contiguous()
    torch.cuda.synchronize()
    base = None
    for name, call in (("scalar call", scalar), ("spectral, every wavelength %.2f" % LAM, lambda: spectral(equal)),
                       ("spectral, wavelengths uniform in [%.2f, %.2f]" % LAM_RANGE, lambda: spectral(spread))):
        med, lo, hi = timed(torch, ctx, call)
        base = base or med
        say("%-46s %-44s %9.2f ms (min %.2f max %.2f)  %8.2f M %s/s  x %.3f of the scalar call"
            % (what, name, med, lo, hi, count / med / 1e3, unit, med / base))


def rays(torch, say):
    n = RAYS_W * RAYS_H
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    u = torch.rand((n, 4), device=dev, generator=g)
    inp = torch.stack([u[:, 0] * 2 - 1, (u[:, 1] * 2 - 1) * (RAYS_H / RAYS_W), torch.full((n,), 2.0 / RAYS_W, device=dev),
                       torch.full((n,), 2.0 / RAYS_W, device=dev), u[:, 2], u[:, 3]], 1).contiguous()
    p = camera.setup_filter(camera.default_params(), RAYS_W, RAYS_H)
    p, model = camera.setup_po(p, "double_gauss_50mm", focus_dist=150.0)
    table, keep = lens_io.make_lens_table(model.spec)
    results = {}
    for compiled, label in (("0", "interpreter"), ("1", "compiled-in")):
        os.environ["LENTIL_RAYS_COMPILED"] = compiled          # (read when the context is created)
        ctx = capi.Context(0)
        ctx.set_params(p)
        ctx.set_lens(table)
        three_ways(torch, say, ctx, "rays %dx%d, double gauss, %s" % (RAYS_W, RAYS_H, label), "rays", n,
                   lambda: ctx.camera_rays(inp, lam=LAM, seed=SEED), lambda lam: ctx.camera_rays(inp, seed=SEED, lambdas=lam), n)
        say("  (path %d)" % ctx.camera_rays_path())
        results[label] = (ctx.camera_rays(inp, lam=LAM, seed=SEED), ctx.camera_rays(inp, seed=SEED, lambdas=torch.full((n,), LAM, dtype=torch.float64, device=dev)))
        ctx.sync()
        ctx.close()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in results.values())
    say("  equal wavelengths give the scalar call's rays, word for word, on both paths: %s" % same)
    os.environ.pop("LENTIL_RAYS_COMPILED", None)


def points(torch, say):
    p, model, table, keep = common.po_setup(W, H, samples_override=1)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)
    ctx = capi.Context(0)
    ctx.set_params(p)
    ctx.set_lens(table)
    ctx.set_bokeh(None)
    ctx.alloc_frame(1)
    ctx.upload_visits(visits)
    ctx.set_draw_log(1 << 22)
    ctx.clear_frame()
    ctx.redistribute()
    ctx.sync()
    vis = np.unique(ctx.draw_log()[:, 0])
    ctx.close()
    say("points: frame %dx%d, %d visits per pixel, %d points (the visits a one-sample pass logs a draw for) x %d attempts" % (W, H, M, vis.size, K))
    pos = np.asarray(cols["pos_z"], np.float32).reshape(-1, 4)
    pix = vis // M
    t_cs = torch.from_numpy(np.ascontiguousarray(pos[vis, :3])).cuda()
    t_px = torch.from_numpy(((pix % W) | ((pix // W) << 16)).astype(np.uint32).view(np.int32)).cuda()
    n = int(vis.size)
    p.samples_override = 256
    ctx = capi.Context(0)
    ctx.set_params(p)
    ctx.set_lens(table)
    for mode, label in ((0, "compiled-in"), (1, "interpreter")):
        ctx.set_lens_mode(mode)
        three_ways(torch, say, ctx, "points %d x %d, double gauss, %s" % (n, K, label), "queries", n * K,
                   lambda: ctx.trace_points(t_cs, t_px, K, lam=LAM), lambda lam: ctx.trace_points(t_cs, t_px, K, lambdas=lam), n)
        say("  (path %d)" % ctx.trace_points_path())
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_rate.txt"))
    ap.add_argument("--rays-only", action="store_true")
    ap.add_argument("--points-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spectral_rate.py measures on the GPU: none here")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("tools/spectral_rate.py: %d warm-up, median of %d, events on the context's stream; %s" % (WARMUP, REPS, torch.cuda.get_device_name(0)))
    if not a.points_only:
        rays(torch, say)
    if not a.rays_only:
        points(torch, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
