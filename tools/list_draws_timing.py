#!/usr/bin/env python3
"""What lentil_hip_list_draws and lentil_hip_plan_visits cost, beside the pass's own draw and beside doing the selection on
the caller's side: the frame of tools/trace_points_timing.py -- 1920x1080 polynomial-optics
double-gauss, 9 visits per pixel, 2 % highlights, samples_override = 256.

(a) list_draws with device pointers over the whole stream, the list sized from the plan's totals[2].  Wall time around the
    call (it returns when the list is complete), over the tries of the attempts the reference's loop makes: counted by one
    untimed trace_points call with out_tries over all 5 * samples attempts of every redistributed visit, cut per visit at
    the attempts list_draws reports through the list (the last record's attempt + 1 for a visit with all its draws, else
    5 * samples).
(b) The yardstick: the chunked pass (LENTIL_STREAM=0) over the same frame in the same run, its draw time
    lentil_hip_last_timing ms[1] over lentil_counters.tries.
(c) The caller's side of the same question without list_draws: trace_points asked for all 5 * samples attempts of every
    redistributed visit (out_pixel + out_xy), before any selection.
(d) plan_visits with device pointers and totals, in GB/s of column traffic: five 16-byte columns read, 32 bytes written.
(e) The same frame with abb_chromatic = 0.5: list_draws with LENTIL_DRAWS_CHANNELS (three traces per attempt, the list
    sized by a counting call) beside the chunked pass's draw of that mode and beside (a).
Every figure: one warm-up call, then the median of --repeats calls.

    python3 tools/list_draws_timing.py [--repeats 6] [--out profiles/list_draws.txt]
    python3 tools/list_draws_timing.py --lane-use     (no GPU: the lanes' share of their waves' time, from the oracle)
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
from pota_amd import _abi, capi  # noqa: E402  (before tests/common puts the repository's root in front)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import common  # noqa: E402

W, H, M, S = 1920, 1080, 9, 256


def lane_use(samples=S):
    """No GPU: how busy the lanes of list_draws' waves are while they trace, counted with the oracle as
    tools/trace_points_timing.py --lane-use counts the batch's.  The points of the tests' 96 x 64 pass case (the same stream
    generator, lens and focus as the timed frame), walked as the kernel walks a visit at `samples` draws: slabs of 64
    attempts until `samples` of them landed in the frame or 5 * samples were made; a lane beyond 5 * samples does not try.
    A wave's try round lasts as long as the most Newton iterations any of its trying lanes needs; a lane is busy for its own."""
    import ctypes as C
    import oracle_lib
    import trace_point_cases as tc
    orc = oracle_lib.load()
    r = tc.pass_case(orc, "pass-po")
    p = r["p"]
    lens = orc.orc_lens_create(C.byref(r["table"]))
    k_bfl, k_ipr = r["table"].lens_back_focal_length, r["table"].lens_inner_pupil_radius
    ap2, sensor, out, it = (C.c_double * 2)(), (C.c_double * 5)(), (C.c_double * 5)(), C.c_int()
    busy = span = rounds = tries = slabs = surplus = 0
    for i in range(r["cs"].shape[0]):
        cs = r["cs"][i]
        target = oracle_lib.darr(-float(cs[0]) * 10.0, -float(cs[1]) * 10.0, -float(cs[2]) * 10.0)
        px, py = int(r["pixel"][i]) & 0xFFFF, int(r["pixel"][i]) >> 16
        accepted, k0 = 0, 0
        while k0 < 5 * samples and accepted < samples:
            trying = list(range(k0, min(k0 + 64, 5 * samples)))
            landed = []
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
                    else:
                        sen = np.array([sensor[0] + sensor[2] * -p.sensor_shift, sensor[1] + sensor[3] * -p.sensor_shift])
                        if tc.pixel_mapping(p, sen)[1] < tc.OUTSIDE:
                            landed.append(m)
                busy += sum(its); span += 64 * max(its); rounds += 1; tries += len(its)
                trying = still
            take = min(len(landed), samples - accepted)
            surplus += len(landed) - take
            accepted += take
            slabs += 1
            k0 += 64
    orc.orc_lens_destroy(lens)
    print("lane use of list_draws' waves at %d draws per visit, counted with the oracle over %d visits (%d slabs, %d try rounds, "
          "%d tries, %d landed attempts beyond the last draw): %d Newton iterations in %d lane-iterations of wave time = %.3f"
          % (samples, r["cs"].shape[0], slabs, rounds, tries, surplus, busy, span, busy / span), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_draws.txt"))
    ap.add_argument("--lane-use", action="store_true", help="no GPU: count the lanes' share of their waves' time with the oracle, and stop")
    ap.add_argument("--lane-use-samples", type=int, default=S)
    a = ap.parse_args()
    if a.lane_use:
        return lane_use(a.lane_use_samples)
    assert a.repeats >= 6
    import torch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        """one warm-up call, then the median / min / max of the repeats, ms"""
        fn()
        ctx.sync()
        ms = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            fn()
            ctx.sync()
            ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms)), min(ms), max(ms)

    p, model, table, keep = common.po_setup(W, H, samples_override=S)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02)
    ctx = capi.Context(0)
    ctx.set_params(p); ctx.set_lens(table); ctx.set_bokeh(None); ctx.alloc_frame(1)
    ctx.upload_visits(visits)
    n = int(visits.n)

    # (b) the yardstick: the chunked pass
    draw_ms, tries = [], []
    for k in range(a.repeats + 1):
        ctx.clear_frame(); ctx.redistribute(); ctx.sync()
        c = ctx.counters()
        assert c.worklist_overflow == 0 and c.streamed == 0
        if k:          # (the first pass sizes the buffers)
            draw_ms.append(float(ctx.last_timing()[1])); tries.append(int(c.tries))
    pass_ns = float(np.median(draw_ms)) * 1e6 / np.mean(tries)
    say("frame %dx%d, %d visits per pixel, samples_override %d: %d visits, %d redistributed" % (W, H, M, S, c.visits, c.redistributed_visits))
    say("(b) chunked pass: draw %.2f ms (median; min %.2f max %.2f, %d passes), %d tries, %d attempted draws, %d accepted -> %.3f ns per try"
        % (float(np.median(draw_ms)), min(draw_ms), max(draw_ms), len(draw_ms), tries[-1], c.attempted_draws, c.accepted_draws, pass_ns))

    # (d) the plan
    plan_ms = timed(lambda: ctx.plan_visits(device=True))
    plan, totals = ctx.plan_visits()
    gb = n * (5 * 16 + 32) / 1e9
    say("(d) plan_visits, device pointers + totals: %.3f ms (median; min %.3f max %.3f, %d calls) for %d visits -> %.0f GB/s of column traffic "
        "(80 B read, 32 B written per visit); totals %s" % (plan_ms + (a.repeats, n, gb / (plan_ms[0] * 1e-3), totals)))
    assert totals[0] == c.visits and totals[1] == c.redistributed_visits

    # (a) the list
    cap = totals[2]
    dev, n_draws, attempts = ctx.list_draws(capacity=cap, device=True)
    assert n_draws == c.accepted_draws and attempts == c.attempted_draws, (n_draws, attempts, c.accepted_draws, c.attempted_draws)
    path = ctx.list_draws_path()
    # the attempts each redistributed visit made, from the list: up to its last record if it has all its draws, else 5 * samples
    words = dev.view(torch.int32)[:n_draws]          # [n_draws, 8]: visit, attempt, pixel, tries, xy
    visit, attempt = words[:, 0].long(), words[:, 1].long()
    count = torch.bincount(visit, minlength=n)
    last = torch.zeros(n, dtype=torch.int64, device=visit.device).scatter_reduce_(0, visit, attempt, "amax")
    made_all = torch.where(count == S, last + 1, torch.full_like(last, 5 * S))
    del dev, words, visit, attempt
    list_ms = timed(lambda: ctx.list_draws(capacity=cap, device=True))
    flagged = np.nonzero(plan["flags"] & _abi.PLAN_REDISTRIBUTE)[0]
    t_made = made_all[torch.from_numpy(flagged).cuda()]
    assert int(t_made.sum()) == attempts
    t_cs = torch.from_numpy(np.ascontiguousarray(plan["cs"][flagged])).cuda()
    t_px = torch.from_numpy(np.ascontiguousarray(plan["pixel"][flagged]).view(np.int32)).cuda()
    torch.cuda.synchronize()
    out = ctx.trace_points(t_cs, t_px, 5 * S, want_xy=False, want_tries=True)
    ctx.sync()
    within = torch.arange(5 * S, device=t_made.device)[None, :] < t_made[:, None]
    through = out["pixel"] != -1          # (int32 bits of LENTIL_POINT_VIGNETTED)
    ref_tries = int(out["tries"][within].sum(dtype=torch.int64)) + int((through & within).sum())
    all_tries = int(out["tries"].sum(dtype=torch.int64)) + int(through.sum())
    del out, within, through
    list_ns = list_ms[0] * 1e6 / ref_tries
    say("(a) list_draws (path %d), device pointers, capacity %d: %.2f ms (median; min %.2f max %.2f, %d calls), %d draws listed, %d attempts, "
        "%d tries in them -> %.3f ns per try; over the pass's %.3f: x %.2f"
        % ((path, cap) + list_ms + (a.repeats, n_draws, attempts, ref_tries, list_ns, pass_ns, list_ns / pass_ns)))
    tp_ms = timed(lambda: ctx.trace_points(t_cs, t_px, 5 * S))
    say("(c) trace_points, all %d attempts of the %d redistributed visits, out_pixel + out_xy, before any selection: %.2f ms (median; min %.2f "
        "max %.2f, %d calls), %d tries -> %.3f ns per try made, %.3f ns per try the list needs; over list_draws: x %.2f in time"
        % ((5 * S, flagged.size) + tp_ms + (a.repeats, all_tries, tp_ms[0] * 1e6 / all_tries, tp_ms[0] * 1e6 / ref_tries, tp_ms[0] / list_ms[0])))
    del t_cs, t_px, t_made, made_all, count, last

    # (e) the same frame with abb_chromatic = 0.5: three channels per attempt (LENTIL_DRAWS_CHANNELS), beside the chunked
    # pass's draw of that mode and beside the plain list above
    pc = type(p).from_buffer_copy(p)
    pc.abb_chromatic = 0.5
    ctx.set_params(pc)
    cdraw_ms = []
    for k in range(a.repeats + 1):
        ctx.clear_frame(); ctx.redistribute(); ctx.sync()
        cc = ctx.counters()
        assert cc.worklist_overflow == 0 and cc.streamed == 0
        if k:
            cdraw_ms.append(float(ctx.last_timing()[1]))
    none, c_records, c_attempts = ctx.list_draws(capacity=0, channels=True)          # the counting call sizes the list
    assert c_records == cc.accepted_draws and c_attempts == cc.attempted_draws, (c_records, c_attempts, cc.accepted_draws, cc.attempted_draws)
    assert c_records <= 11 * totals[2]
    clist_ms = timed(lambda: ctx.list_draws(capacity=c_records, device=True, channels=True))
    say("(e) abb_chromatic 0.5: chunked pass draw %.2f ms (median; min %.2f max %.2f, %d passes); list_draws with LENTIL_DRAWS_CHANNELS (path %d), "
        "device pointers, capacity %d: %.2f ms (median; min %.2f max %.2f, %d calls), %d records, %d attempts -> x %.2f the pass's draw, "
        "x %.2f the plain list; %.3f ns per record against the plain list's %.3f"
        % ((float(np.median(cdraw_ms)), min(cdraw_ms), max(cdraw_ms), len(cdraw_ms), ctx.list_draws_path(), c_records) + clist_ms
           + (a.repeats, c_records, c_attempts, clist_ms[0] / float(np.median(cdraw_ms)), clist_ms[0] / list_ms[0],
              clist_ms[0] * 1e6 / c_records, list_ms[0] * 1e6 / n_draws)))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/list_draws_timing.py --repeats %d\n" % a.repeats + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
