"""Development aid: the headline frame of bench.py (double gauss, 3840x2160, 9 visits per pixel, 1024 draws, f_hi 2^-16, beauty)
through one form of the pass per process, one resident stream: time per step (clear, pass, resolve) and the solve counters.
    spectral   a wavelength column of the constant lambda_bw (lentil_hip_set_visit_lambdas, bound device memory):
               solve_po_spectral_kernel, chunked
    chunked    the scalar pass forced into the chunked form (LENTIL_STREAM=0): solve_po_kernel
    streamed   the scalar pass as it runs by default
usage: python3 tools/spectral_pass_rate.py FORM [steps] [warmup]     (LENTIL_HIP_LIB: another build of the library)
Prints one JSON line.  From lentil_counters: iterations per try, lane rounds per try (64 slots per iteration the kernel
offered), and the share of slots no lane used -- in solve_po_spectral_kernel the lanes that wait for their task's slowest."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
form = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
assert form in ("spectral", "chunked", "streamed")
if form == "chunked":
    os.environ["LENTIL_STREAM"] = "0"          # (read when the context is created)
import torch  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda:0")
b = bench.Bench(torch, None, dev, 0, 1, 0, 3840, 2160, 2160, 9, "double_gauss_50mm", 1024, 0, 2.0 ** -16, False, same_frame=True)
b.generate(2.0 ** -16)
ctx = b.ctx
cols, v, kv = b.streams[0]
ctx.bind_visits(v, kv)
lam = None
if form == "spectral":
    lam = torch.full((int(v.n),), float(b.p.lambda_bw), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_visit_lambdas(lam, device=True)


def step():
    ctx.clear_frame(); ctx.redistribute(); ctx.resolve()


for _ in range(warmup):
    step()
ctx.sync()
ctx.pass_totals(reset=True)
ms = []
for _ in range(steps):
    t0 = time.perf_counter()
    step()
    ctx.sync()
    ms.append((time.perf_counter() - t0) * 1e3)
t = ctx.pass_totals()
c = ctx.counters()
ms.sort()
tries = max(int(t.tries), 1)
out = {"form": form, "lib": os.environ.get("LENTIL_HIP_LIB", "this tree's"), "steps": steps,
       "ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
       "passes": int(t.passes), "streamed": int(t.streamed), "accepted_per_pass": int(c.accepted_draws), "attempted_per_pass": int(c.attempted_draws),
       "tries_per_pass": int(t.tries) // max(int(t.passes), 1),
       "iterations_per_try": round(int(t.newton_iterations) / tries, 3), "lane_rounds_per_try": round(int(t.lane_rounds) / tries, 3),
       "idle_slot_share": round(1.0 - int(t.newton_iterations) / max(int(t.lane_rounds), 1), 4),
       "slow_solves": int(t.slow_solves), "draw_ms_mean": round(t.draw_ms / max(int(t.passes), 1), 4), "scan_ms_mean": round(t.scan_ms / max(int(t.passes), 1), 4)}
if form == "spectral":
    out["spectral_pass_stats"] = ctx.spectral_pass_stats()
print(json.dumps(out))
