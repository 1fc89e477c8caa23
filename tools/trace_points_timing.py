#!/usr/bin/env python3
"""What a batch of lentil_hip_trace_points costs per try, beside the pass's own draw: a 1920x1080
polynomial-optics double-gauss frame, 9 visits per pixel, 2 % highlights, samples_override = 256.

(a) The batch: lentil_hip_trace_points with device pointers, out_pixel + out_xy, K = 256 attempts for every redistributed
    visit of that frame (the visits with a draw in the log of a samples_override = 1 pass), through the compiled-in lens and
    through the table interpreter, alternating.  Wall time around the call and a synchronise, over the tries the batch made
    (counted by one untimed call with out_tries).
(b) The yardstick: the chunked pass (LENTIL_STREAM=0) over the same frame, its draw time lentil_hip_last_timing ms[1] over
    lentil_counters.tries -- and its newton_iterations / lane_rounds: the share of its lanes' rounds that advance a solve.
The pass refills a lane whose solve is done; the batch's wave runs until its slowest lane is.

    python3 tools/trace_points_timing.py [--repeats 6] [--out profiles/trace_points.txt]
    python3 tools/trace_points_timing.py --lane-use        (no GPU: the lanes' share of their waves' time, from the oracle)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(q, "pota_amd")) for q in sys.path if q):
    sys.path.insert(0, ROOT)
os.environ["LENTIL_STREAM"] = "0"          # (read when a context is created: the yardstick is the chunked pass)
from pota_amd import capi  # noqa: E402  (before tests/common puts the repository's root in front)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import common  # noqa: E402

W, H, M, S, K = 1920, 1080, 9, 256, 256


def lane_use():
    """No GPU: how busy the lanes of the batch's waves are, counted with the oracle.  The points of the tests' 96 x 64 pass
    case (the same stream generator, lens and focus as the timed frame), one slab each: attempts 0 ... 63.  A wave's try
    round lasts as long as the most Newton iterations any of its trying lanes needs; a lane is busy for its own."""
    import ctypes as C
    import oracle_lib
    import trace_point_cases as tc
    orc = oracle_lib.load()
    r = tc.pass_case(orc, "pass-po")
    p = r["p"]
    lens = orc.orc_lens_create(C.byref(r["table"]))
    k_bfl, k_ipr = r["table"].lens_back_focal_length, r["table"].lens_inner_pupil_radius
    ap2, sensor, out, it = (C.c_double * 2)(), (C.c_double * 5)(), (C.c_double * 5)(), C.c_int()
    busy = span = rounds = tries = 0
    for i in range(r["cs"].shape[0]):
        cs = r["cs"][i]
        target = oracle_lib.darr(-float(cs[0]) * 10.0, -float(cs[1]) * 10.0, -float(cs[2]) * 10.0)
        px, py = int(r["pixel"][i]) & 0xFFFF, int(r["pixel"][i]) >> 16
        trying = list(range(64))
        for t in range(int(p.vignetting_retries) + 1):
            if not trying:
                break
            its, still = [], []
            for m in trying:
                orc.orc_po_aperture_sample(C.byref(p), None, px * py + px, m + t, ap2)
                T = orc.orc_lt_sample_aperture(lens, target, ap2, sensor, out, p.lambda_bw, C.byref(it))
                its.append(it.value)
                ipx, ipy = sensor[0] + sensor[2] * k_bfl, sensor[1] + sensor[3] * k_bfl
                if np.float32(T) <= 0 or ipx * ipx + ipy * ipy > k_ipr * k_ipr:
                    still.append(m)
            busy += sum(its); span += 64 * max(its); rounds += 1; tries += len(its)
            trying = still
    orc.orc_lens_destroy(lens)
    print("lane use of the batch's waves, counted with the oracle over %d slabs (%d try rounds, %d tries): %d Newton iterations in "
          "%d lane-iterations of wave time = %.3f" % (r["cs"].shape[0], rounds, tries, busy, span, busy / span), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_points.txt"))
    ap.add_argument("--lane-use", action="store_true", help="no GPU: count the lanes' share of their waves' time with the oracle, and stop")
    a = ap.parse_args()
    if a.lane_use:
        return lane_use()
    import torch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    p, model, table, keep = common.po_setup(W, H, samples_override=1)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)
    ctx = capi.Context(0)
    ctx.set_params(p); ctx.set_lens(table); ctx.set_bokeh(None); ctx.alloc_frame(1)
    ctx.upload_visits(visits)

    # the redistributed visits: those with a draw in the log of a one-sample pass
    ctx.set_draw_log(1 << 22)
    ctx.clear_frame(); ctx.redistribute(); ctx.sync()
    c = ctx.counters()
    log = ctx.draw_log()
    vis = np.unique(log[:, 0])
    say("frame %dx%d, %d visits per pixel: %d visits, %d redistributed, %d of them with a logged draw (the batch's points)"
        % (W, H, M, c.visits, c.redistributed_visits, vis.size))
    ctx.close()

    # (b) the yardstick: the chunked pass at samples_override = 256, in a context of its own
    p.samples_override = S
    ctx = capi.Context(0)
    ctx.set_params(p); ctx.set_lens(table); ctx.set_bokeh(None); ctx.alloc_frame(1)
    ctx.upload_visits(visits)
    draw_ms, tries, newton, rounds = [], [], [], []
    for k in range(a.repeats + 1):
        ctx.clear_frame(); ctx.redistribute(); ctx.sync()
        c = ctx.counters()
        assert c.worklist_overflow == 0 and c.streamed == 0
        if k:          # (the first pass sizes the buffers)
            draw_ms.append(float(ctx.last_timing()[1])); tries.append(int(c.tries))
            newton.append(int(c.newton_iterations)); rounds.append(int(c.lane_rounds))
    draw_ms = np.array(draw_ms)
    pass_ns = draw_ms.mean() * 1e6 / np.mean(tries)
    say("(b) chunked pass, samples_override %d: draw %.2f ms (min %.2f max %.2f, %d passes), %d tries, %d attempted draws -> %.3f ns per try; "
        "newton_iterations / lane_rounds = %d / %d = %.3f"
        % (S, draw_ms.mean(), draw_ms.min(), draw_ms.max(), len(draw_ms), tries[-1], c.attempted_draws, pass_ns, newton[-1], rounds[-1],
           newton[-1] / max(rounds[-1], 1)))

    # (a) the batch
    pos = np.asarray(cols["pos_z"], np.float32).reshape(-1, 4)
    pix = vis // M
    t_cs = torch.from_numpy(np.ascontiguousarray(pos[vis, :3])).cuda()
    t_px = torch.from_numpy(((pix % W) | ((pix // W) << 16)).astype(np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    ns = {}
    made = {}
    for mode in (0, 1):          # one untimed call each: warms the kernel up and counts the tries
        ctx.set_lens_mode(mode)
        out = ctx.trace_points(t_cs, t_px, K, want_xy=False, want_tries=True)
        ctx.sync()
        through = out["pixel"] != -1          # (int32 bits of LENTIL_POINT_VIGNETTED)
        made[mode] = int(out["tries"].sum(dtype=torch.int64)) + int(through.sum())
        say("batch, lens mode %d (path %d): %d points x %d attempts = %d queries, %d tries, %d vignetted, %d outside the frame"
            % (mode, ctx.trace_points_path(), vis.size, K, out["pixel"].numel(), made[mode], int((~through).sum()), int((out["pixel"] == -2).sum())))
        del out, through
        out = ctx.trace_points(t_cs, t_px, K)          # (... and the timed form once: its buffers come from torch's cache afterwards)
        ctx.sync()
        del out
    times = {0: [], 1: []}
    for _ in range(a.repeats):
        for mode in (0, 1):
            ctx.set_lens_mode(mode)
            ctx.sync()
            t = time.perf_counter()
            out = ctx.trace_points(t_cs, t_px, K)
            ctx.sync()
            times[mode].append((time.perf_counter() - t) * 1e3)
            del out
    for mode, name in ((0, "compiled-in lens"), (1, "table interpreter")):
        ms = np.array(times[mode])
        ns[mode] = ms.mean() * 1e6 / made[mode]
        say("(a) batch, %s, out_pixel + out_xy: %.2f ms (min %.2f max %.2f, %d calls) -> %.3f ns per try; over the pass's %.3f: x %.2f"
            % (name, ms.mean(), ms.min(), ms.max(), len(ms), ns[mode], pass_ns, ns[mode] / pass_ns))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/trace_points_timing.py --repeats %d\n" % a.repeats + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
