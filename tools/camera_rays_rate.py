"""Rate of forward camera rays in batches (lentil_hip_camera_rays): one batch of 3840x2160 rays, input and output resident
on the device, timed with events on the context's stream (20 repetitions after 5 untimed ones) -- for the double-gauss
polynomial-optics lens and for the thin lens.  Beside it the only way to get these rays without the batch call:
lentil_host_camera_create_ray, one ray per call, on 16 threads of the same machine (a C++ loop compiled here against
liblentil_host.so; the same batch, each ray from the same per-ray xor128 state, so the two produce the same rays --
the first 65 536 are compared).  A development aid, not part of bench.py.
Writes profiles/camera_rays_rate.json, and a copy to the path given as a third argument.  usage: camera_rays_rate.py [W H [copy.json]]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pota_amd import _abi, camera, capi, hostlib, lens_io

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
WARMUP, REPS, THREADS = 5, 20, 16
SEED = 0x5EED
LAM = float(np.float32(550.0)) * 0.001
HBM_PEAK = 8.0e12         # B/s, the spec figure the write floor is taken against
BYTES_PER_RAY = (_abi.RAY_IN_FLOATS + _abi.RAY_OUT_FLOATS) * 4

HOST_LOOP = r'''
#include <cstdint>
#include <thread>
#include <vector>
#include "lentil_host.h"
static uint32_t tea8(uint32_t v0, uint32_t v1) {
  uint32_t s0 = 0;
  for (int n = 0; n < 8; ++n) {
    s0 += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xA341316Cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xC8013EA4u);
    v1 += ((v0 << 4) + 0xAD90777Du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7E95761Eu);
  }
  return v0;
}
extern "C" void host_rays(const lentil_params *P, const lentil_host_lens *L, double lambda, float exposure, uint32_t seed,
                          uint64_t n, const float *in, float *out, int threads) {
  std::vector<std::thread> ts;
  for (int t = 0; t < threads; ++t)
    ts.emplace_back([=] {
      for (uint64_t i = n * t / threads; i < n * (t + 1) / threads; ++i) {
        uint32_t s[4];
        s[0] = tea8((uint32_t)i, seed); s[1] = tea8((uint32_t)i, s[0]); s[2] = tea8((uint32_t)i, s[1]); s[3] = tea8((uint32_t)i, s[2]);
        if (!(s[0] | s[1] | s[2] | s[3])) lentil_host_xor128_init(s);
        lentil_host_camera_create_ray(P, L, nullptr, s, lambda, exposure, in + i * 6, (lentil_host_camera_ray *)(out + i * 21));
      }
    });
  for (auto &t : ts) t.join();
}
'''


def build_host_loop(tmp):
    src = os.path.join(tmp, "host_rays.cpp")
    so = os.path.join(tmp, "libhost_rays.so")
    open(src, "w").write(HOST_LOOP)
    pkg = os.path.join(ROOT, "pota_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so, src,
                           "-L", pkg, "-llentil_host", "-Wl,-rpath," + os.path.abspath(pkg), "-lpthread"])
    lib = C.CDLL(so)
    lib.host_rays.restype = None
    lib.host_rays.argtypes = [C.POINTER(_abi.Params), C.c_void_p, C.c_double, C.c_float, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def measure(name, p, table, host_lens, host_loop):
    n = W * H
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    u = torch.rand((n, 4), device=dev, generator=g)
    aspect = H / W
    inp = torch.stack([u[:, 0] * 2 - 1, (u[:, 1] * 2 - 1) * aspect, torch.full((n,), 2.0 / W, device=dev),
                       torch.full((n,), 2.0 / W, device=dev), u[:, 2], u[:, 3]], 1).contiguous()
    ctx = capi.Context(0)
    ctx.set_params(p)
    if table is not None:
        ctx.set_lens(table)
    stream = torch.cuda.ExternalStream(ctx.stream())
    torch.cuda.synchronize()
    for _ in range(WARMUP):
        out, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
    ctx.sync()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(stream)
        out, tries = ctx.camera_rays(inp, lam=LAM, seed=SEED, want_tries=True)
        b.record(stream)
    ctx.sync()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    med = ms[len(ms) // 2]
    hist = torch.bincount(tries.to(torch.int64)).cpu().tolist()
    res = {"rays": n, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(ms[0], 4), "kernel_ms_max": round(ms[-1], 4),
           "gpu_rays_per_s": round(n / (med * 1e-3)), "write_floor_ms": round(n * BYTES_PER_RAY / HBM_PEAK * 1e3, 4),
           "share_of_write_floor": round(n * BYTES_PER_RAY / HBM_PEAK * 1e3 / med, 4), "tries_histogram": hist,
           "weight_zero_rays": int((out[:, 6] == 0).sum().item())}
    # the host library, one ray per call, THREADS threads
    m = n
    h_in = inp[:m].cpu().numpy()
    h_out = np.zeros((m, _abi.RAY_OUT_FLOATS), np.float32)
    host_loop.host_rays(C.byref(p), host_lens, LAM, 1.0, SEED, min(m, 4096), h_in.ctypes.data, h_out.ctypes.data, THREADS)   # warm
    t0 = time.perf_counter()
    host_loop.host_rays(C.byref(p), host_lens, LAM, 1.0, SEED, m, h_in.ctypes.data, h_out.ctypes.data, THREADS)
    t1 = time.perf_counter()
    res["host_threads"] = THREADS
    res["host_rays_timed"] = m
    res["host_seconds"] = round(t1 - t0, 4)
    res["host_rays_per_s"] = round(m / (t1 - t0))
    res["gpu_over_host"] = round(res["gpu_rays_per_s"] / res["host_rays_per_s"], 1)
    k = min(m, 1 << 16)
    g_out = out[:k].cpu().numpy()
    res["sample_compared"] = k
    res["sample_rays_differing_from_host"] = int((g_out.view(np.uint32) != h_out[:k].view(np.uint32)).any(1).sum())
    ctx.close()
    return res


def main():
    if not torch.cuda.is_available():
        raise SystemExit("camera_rays_rate.py measures on the GPU: none here")
    out = {"frame": "%dx%d" % (W, H), "warmup": WARMUP, "repetitions": REPS, "bytes_per_ray": BYTES_PER_RAY, "hbm_peak_Bps": HBM_PEAK}
    with tempfile.TemporaryDirectory() as tmp:
        host_loop = build_host_loop(tmp)
        p = camera.setup_filter(camera.default_params(), W, H)
        p, model = camera.setup_po(p, "double_gauss_50mm", focus_dist=150.0)
        table, keep = lens_io.make_lens_table(model.spec)
        hl = hostlib.HostLens(model.spec)
        out["double_gauss_50mm"] = measure("po", p, table, hl.h, host_loop)
        hl.close()
        tl = camera.setup_thinlens(camera.setup_filter(camera.default_params(), W, H))
        tl.optical_vignetting_distance = 2.0          # (so that the thin lens retries too)
        out["thin_lens"] = measure("tl", tl, None, None, host_loop)
    s = json.dumps(out, indent=1)
    print(s)
    paths = [os.path.join(ROOT, "profiles", "camera_rays_rate.json")] + sys.argv[3:4]
    for path in paths:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        open(path, "w").write(s + "\n")


if __name__ == "__main__":
    main()
