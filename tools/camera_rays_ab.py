"""Forward camera rays, compiled lens against the table interpreter: tools/camera_rays_rate.py's recipe
-- one batch of 3840x2160 rays resident on the device, timed with events on the context's stream, 20 repetitions after 5
untimed ones -- for two contexts per lens in ONE process on ONE box, one created with LENTIL_RAYS_COMPILED=1 and one with =0 in the
environment, their timed calls alternating (as tools/ab_inproc.py alternates its settings: boxes differ by a few per cent,
calls a moment apart do not).  Lenses: double_gauss_50mm and petzval_58mm (compiled in), anamorphic_petzval_58mm (compiled at
run time: waited for first), and the thin lens, whose kernel neither setting touches, as the control.  The two contexts'
outputs are compared word for word.  Writes profiles/camera_rays_rate_compiled.json.  usage: camera_rays_ab.py [W H]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pota_amd import camera, capi, lens_io

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
WARMUP, REPS = 5, 20
SEED = 0x5EED
LAM = float(np.float32(550.0)) * 0.001


def context(p, table, compiled):
    # (the library reads LENTIL_RAYS_COMPILED once, when a context is created: set around lentil_hip_create, restored after)
    old = os.environ.get("LENTIL_RAYS_COMPILED")
    os.environ["LENTIL_RAYS_COMPILED"] = "1" if compiled else "0"
    try:
        ctx = capi.Context(0)
    finally:
        if old is None:
            os.environ.pop("LENTIL_RAYS_COMPILED", None)
        else:
            os.environ["LENTIL_RAYS_COMPILED"] = old
    ctx.set_params(p)
    if table is not None:
        ctx.set_lens(table)
        ctx.lens_jit_wait(600.0)
    return ctx


def stats(ms):
    ms = sorted(ms)
    return {"kernel_ms_median": round(ms[len(ms) // 2], 4), "kernel_ms_min": round(ms[0], 4), "kernel_ms_max": round(ms[-1], 4)}


def measure(p, table):
    n = W * H
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    u = torch.rand((n, 4), device=dev, generator=g)
    inp = torch.stack([u[:, 0] * 2 - 1, (u[:, 1] * 2 - 1) * (H / W), torch.full((n,), 2.0 / W, device=dev),
                       torch.full((n,), 2.0 / W, device=dev), u[:, 2], u[:, 3]], 1).contiguous()
    torch.cuda.synchronize()
    sides = {"compiled": context(p, table, True), "interpreter": context(p, table, False)}
    res, outs, times = {}, {}, {k: [] for k in sides}
    for k, ctx in sides.items():
        for _ in range(WARMUP):
            outs[k] = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
        ctx.sync()
        res[k] = {"path": ctx.camera_rays_path()}
    for _ in range(REPS):
        for k, ctx in sides.items():
            stream = torch.cuda.ExternalStream(ctx.stream())
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            outs[k] = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
            b.record(stream)
            ctx.sync()
            times[k].append(a.elapsed_time(b))
    for k in sides:
        res[k].update(stats(times[k]))
        res[k]["gpu_rays_per_s"] = round(n / (res[k]["kernel_ms_median"] * 1e-3))
    res["rays"] = n
    res["interpreter_over_compiled"] = round(res["interpreter"]["kernel_ms_median"] / res["compiled"]["kernel_ms_median"], 3)
    res["outputs_identical"] = bool(torch.equal(outs["compiled"][0].view(torch.int32), outs["interpreter"][0].view(torch.int32)) and
                                    torch.equal(outs["compiled"][1], outs["interpreter"][1]))
    for ctx in sides.values():
        ctx.close()
    return res


def main():
    if not torch.cuda.is_available():
        raise SystemExit("camera_rays_ab.py measures on the GPU: none here")
    out = {"frame": "%dx%d" % (W, H), "warmup": WARMUP, "repetitions": REPS,
           "paths": "0 thin lens, 1 table interpreter, 2 compiled-in lens, 3 run-time kernel"}
    for lens in ("double_gauss_50mm", "petzval_58mm", "anamorphic_petzval_58mm"):
        p = camera.setup_filter(camera.default_params(), W, H)
        p, model = camera.setup_po(p, lens, focus_dist=150.0)
        table, keep = lens_io.make_lens_table(model.spec)
        out[lens] = measure(p, table)
        print(lens, json.dumps(out[lens]), flush=True)
    tl = camera.setup_thinlens(camera.setup_filter(camera.default_params(), W, H))
    tl.optical_vignetting_distance = 2.0          # (as tools/camera_rays_rate.py: so that the thin lens retries too)
    out["thin_lens"] = measure(tl, None)
    s = json.dumps(out, indent=1)
    print(s)
    open(os.path.join(ROOT, "profiles", "camera_rays_rate_compiled.json"), "w").write(s + "\n")


if __name__ == "__main__":
    main()
