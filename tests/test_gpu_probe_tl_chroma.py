"""Occlusion probes with the thin lens and abb_chromatic > 0 (redistribute_tl_chroma / tl_chroma_probe in
pota_amd/csrc/lentil_hip.hip; kernels tl_chroma_probe_* in lentil_kernels.h).

The reference probes a thin-lens attempt before its vignetting test and before its xor128 colour draw (src/lentil_filter.cpp:
356-375, then :393-406): an occluded attempt is lost and consumes no generator output.  The HIP path solves every attempt an item
could make, then -- before the walk draws any channel -- asks about the attempts the walk can possibly reach, in a loop whose
bound moves on as occluded attempts fail.  The "scene" is the oracle's analytic sphere on both sides, the oracle single-threaded
(one xor128 stream in visit order).  Tolerances are the suite's own (check_logs: bit-identical; check_frame: 1e-5).
"""
import ctypes as C

import numpy as np
import pytest

import common
import oracle_lib
from pota_amd import _abi, capi
from test_gpu_parity import check_frame, check_logs
from test_native_exchange_tl_chroma import _columns

pytestmark = pytest.mark.gpu

W, H, M = 96, 64, 9
KINDS = [0, 0, 1]
SPHERE = (6.0, 2.0, -70.0, 9.0)          # beside the optical axis, between the lens and the far highlights (cm, camera looks down -z)


def _oracle(orc, p, visits, probe, start=None, kinds=KINDS, motion=None):
    """single-threaded oracle frame (after the pass) and the generator state it ended at"""
    ref = oracle_lib.Frame(orc, p, n_aovs=len(kinds), kinds=kinds, keep_log=True)
    if motion is not None:
        ref.set_camera_motion(motion)
    if probe is not None:
        ref.set_probe(*probe)
    if start is not None:
        orc.orc_frame_set_xor128(ref.h, (C.c_uint32 * 4)(*start))
    ref.run(None, None, visits)
    st = (C.c_uint32 * 4)()
    orc.orc_frame_get_xor128(ref.h, st)
    return ref, list(st)


def _setup(ctx, p, visits, probe, kinds=KINDS, log=1 << 22):
    ctx.set_params(p)
    ctx.set_bokeh(None)
    ctx.alloc_frame(len(kinds), kinds)
    ctx.set_draw_log(log)
    ctx.set_occlusion_probe(*probe)
    ctx.upload_visits(visits)


def _pass(ctx):
    ctx.clear_frame(); ctx.redistribute(); ctx.resolve(); ctx.sync()
    c = ctx.counters()
    assert c.worklist_overflow == 0 and c.streamed == 0
    return c


def _same_counters(c, rc):
    assert (c.redistributed_visits, c.attempted_draws, c.accepted_draws) == (rc.redistributed_visits, rc.attempted_draws, rc.accepted_draws)


@pytest.mark.parametrize("ctype,coma,vignetting", [(0, 0.0, 0.0), (1, 0.35, 2.0)], ids=["green-magenta", "red-cyan+coma+vignetting"])
def test_occluder_with_chromatic_aberration(orc, ctype, coma, vignetting):
    """The frame of test_thinlens_chromatic_aberration behind a sphere: counters, accepted (visit, attempt | channel, pixel)
    lists and the generator state after every pass are the oracle's -- over a second pass that continues the stream and a third
    from a chosen state -- and the sphere bites."""
    p = common.tl_setup(W, H, samples_override=48, abb_chromatic=0.6, abb_chromatic_type=ctype, abb_coma=coma,
                        optical_vignetting_distance=vignetting, optical_vignetting_radius=1.5)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02, n_extra=2)
    sphere = np.array(SPHERE, np.float32)
    probe = (oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
    ctx = capi.Context(0)
    try:
        _setup(ctx, p, visits, probe)
        start = None
        for frame in range(3):
            if frame == 2:                                   # a starting state of the host's choosing
                start = [0x12345678, 0x9ABCDEF0, 0x0F1E2D3C, 0x4B5A6978]
                ctx.set_xor128_state(start)
            ref, end = _oracle(orc, p, visits, probe, start)
            free, _ = _oracle(orc, p, visits, None, start)
            rc = ref.counters()
            assert rc.redistributed_visits > 100 and rc.accepted_draws > 5000
            before = ctx.probe_stats()
            c = _pass(ctx)
            _same_counters(c, rc)
            check_logs(ctx, ref)
            assert set(np.unique(ctx.draw_log()[:, 1] >> 30)) == {0, 1, 2}
            assert ctx.get_xor128_state() == end
            check_frame(ctx, ref, n_aovs=3, kinds=KINDS)
            probed, occluded, calls = (a - b for a, b in zip(ctx.probe_stats(), before))
            print("pass %d: attempted %d accepted %d | segments asked %d occluded %d callbacks %d" %
                  (frame, rc.attempted_draws, rc.accepted_draws, probed, occluded, calls))
            assert 0 < occluded < probed
            # (every attempt the reference makes is probed there; here those that got through the vignetting test are asked about)
            assert probed >= rc.accepted_draws and calls >= 1
            # ... and the occluder changed something
            fl, rl = common.sort_log(free.log()), common.sort_log(ref.log())
            assert fl.shape != rl.shape or not np.array_equal(fl, rl)
            assert free.counters().attempted_draws != rc.attempted_draws
            start = end                                      # the next pass continues the stream
            ref.close(); free.close()
        # probing off again: the unoccluded frame
        ctx.set_occlusion_probe(None)
        free, end = _oracle(orc, p, visits, None, start)
        _same_counters(_pass(ctx), free.counters())
        check_logs(ctx, free)
        assert ctx.get_xor128_state() == end
        free.close()
    finally:
        ctx.close()


def test_nothing_is_asked_beyond_what_the_reference_could_reach(orc):
    """A probe that never occludes, no vignetting, highlights only in the frame's centre: every attempt lands inside the frame in
    all three channels, so the reference makes exactly `samples` attempts per item (attempted == accepted, checked on the
    oracle) and probes each once.  The loop's bound is then exact: the library asks about just as many segments, in one call."""
    p = common.tl_setup(W, H, samples_override=48, abb_chromatic=0.6, abb_chromatic_type=0)
    cols = _columns(p, lambda px, py: (px >= 24) & (px < W - 24) & (py >= 16) & (py < H - 16))
    visits, keep = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    sphere = np.array([0.0, 0.0, 1.0e6, 1.0], np.float32)        # far behind the camera
    probe = (oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
    ref, end = _oracle(orc, p, visits, probe)
    rc = ref.counters()
    assert rc.redistributed_visits > 0 and rc.attempted_draws == rc.accepted_draws > 0
    ctx = capi.Context(0)
    try:
        _setup(ctx, p, visits, probe)
        _same_counters(_pass(ctx), rc)
        check_logs(ctx, ref)
        assert ctx.get_xor128_state() == end
        probed, occluded, calls = ctx.probe_stats()
        print("attempted %d | segments asked %d callbacks %d" % (rc.attempted_draws, probed, calls))
        assert probed == rc.attempted_draws
        assert occluded == 0 and calls == 1
    finally:
        ctx.close()
        ref.close()


def test_moved_and_moving_camera(orc):
    """A camera away from the origin, AiCameraToWorldMatrix given explicitly (test_probe_with_a_given_camera_to_world_and_a_
    moved_camera, with the chromatic thin lens); then the same context with motion keys over the shutter and a time per sample:
    the segments end at the blended inverse keys' image of the lens point, on both sides."""
    p = common.tl_setup(W, H, samples_override=32, abb_chromatic=0.6, abb_chromatic_type=1, abb_coma=0.35)
    a = np.float32(0.1)
    rot = np.array([[np.cos(a), 0, -np.sin(a), 0], [0, 1, 0, 0], [np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], np.float64)
    tr = np.eye(4); tr[3, :3] = (5.0, -3.0, 20.0)
    c2w = (rot @ tr).astype(np.float32)                       # row-vector convention: p_world = p_cam @ c2w
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    for r in range(4):
        for c in range(4):
            p.world_to_camera[r][c] = float(w2c[r, c])
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02, n_extra=2)
    pos = cols["pos_z"]
    ph = np.concatenate([pos[:, :3].astype(np.float64), np.ones((pos.shape[0], 1))], axis=1) @ c2w.astype(np.float64)
    pos[:, :3] = ph[:, :3].astype(np.float32)
    sw = np.array([SPHERE[0], SPHERE[1], SPHERE[2], 1.0]) @ c2w.astype(np.float64)
    sphere = np.array([sw[0], sw[1], sw[2], SPHERE[3]], np.float32)
    probe = (oracle_lib.sphere_occluder(orc), sphere.ctypes.data, c2w)
    ctx = capi.Context(0)
    try:
        _setup(ctx, p, visits, probe)
        ref, end = _oracle(orc, p, visits, probe)
        assert ref.counters().redistributed_visits > 100
        _same_counters(_pass(ctx), ref.counters())
        check_logs(ctx, ref)
        assert ctx.get_xor128_state() == end
        check_frame(ctx, ref, n_aovs=3, kinds=KINDS)
        assert ctx.probe_stats()[1] > 0
        ref.close()
        # the camera moves over the shutter: world-to-camera keys that start at the static matrix, every sample at its own time
        keys = []
        for k in range(3):
            t = k / 2.0
            m = np.eye(4, dtype=np.float64); m[3, :3] = (8.0 * t, -2.0 * t * t, 3.0 * t)
            keys.append((w2c.astype(np.float64) @ m).astype(np.float32))
        keys = np.stack(keys)
        cols["raydir_time"][:, 3] = np.random.default_rng(5).uniform(-0.1, 1.1, visits.n).astype(np.float32)
        visits, keepv = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
        start = ctx.get_xor128_state()
        ref, end = _oracle(orc, p, visits, probe, start, motion=keys)
        still, _ = _oracle(orc, p, visits, probe, start)
        assert not np.array_equal(common.sort_log(ref.log()), common.sort_log(still.log()))
        ctx.set_camera_motion(keys)
        ctx.upload_visits(visits)
        before = ctx.probe_stats()
        _same_counters(_pass(ctx), ref.counters())
        check_logs(ctx, ref)
        assert ctx.get_xor128_state() == end
        check_frame(ctx, ref, n_aovs=3, kinds=KINDS)
        assert ctx.probe_stats()[1] > before[1]
        ref.close(); still.close()
    finally:
        ctx.close()


def test_negative_abb_chromatic_is_probed_round_by_round(orc):
    """abb_chromatic < 0 is not chromatic on the thin lens (`> 0.0`, src/lentil_filter.cpp:393): the ordinary probed pass."""
    p = common.tl_setup(W, H, samples_override=48, abb_chromatic=-0.5)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02, n_extra=2)
    sphere = np.array(SPHERE, np.float32)
    probe = (oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
    ref, end = _oracle(orc, p, visits, probe)
    plain = common.tl_setup(W, H, samples_override=48)
    same, _ = _oracle(orc, plain, visits, probe)
    assert np.array_equal(common.sort_log(ref.log()), common.sort_log(same.log()))       # (and no channel bits)
    ctx = capi.Context(0)
    try:
        _setup(ctx, p, visits, probe)
        for _ in range(2):
            _same_counters(_pass(ctx), ref.counters())
            check_logs(ctx, ref)
            check_frame(ctx, ref, n_aovs=3, kinds=KINDS)
        probed, occluded, calls = ctx.probe_stats()
        assert 0 < occluded < probed
    finally:
        ctx.close()
        ref.close(); same.close()


def test_polynomial_optics_with_chromatic_aberration_stays_refused(orc):
    p, model, table, keep = common.po_setup(32, 24, samples_override=16, abb_chromatic=0.5)
    visits, cols = common.make_stream(p, 32, 24, M, f_hi=0.05)
    sphere = np.array([0, 0, -70.0, 5.0], np.float32)
    ctx = capi.Context(0)
    try:
        ctx.set_params(p); ctx.set_lens(table); ctx.alloc_frame(1)
        ctx.set_occlusion_probe(oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
        ctx.upload_visits(visits)
        ctx.clear_frame()
        with pytest.raises(capi.LentilError) as e:
            ctx.redistribute()
        assert e.value.code == _abi.ERR_UNSUPPORTED
        assert "polynomial optics" in str(e.value)
        assert ctx.probe_stats() == (0, 0, 0)
    finally:
        ctx.close()


def test_a_pass_run_again_does_not_ask_again(orc):
    """A closest-AOV candidate at depth 0 in a context without a draw log: the pass is run twice (closest_rerun_with_log).  The
    second run fails the attempts the first found occluded and asks the renderer nothing: the callback -- counted here -- sees
    what one run asks, and so does lentil_hip_probe_stats; the draws are still the oracle's."""
    p = common.tl_setup(W, H, samples_override=48, abb_chromatic=0.6, abb_chromatic_type=1, abb_coma=0.35,
                        optical_vignetting_distance=2.0, optical_vignetting_radius=1.5)
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02, n_extra=2)
    sphere = np.array(SPHERE, np.float32)
    plain = (oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
    ref, _ = _oracle(orc, p, visits, plain)
    v0 = int(common.sort_log(ref.log())[0, 0])                # a redistributed visit with accepted draws
    ref.close()
    cols["pos_z"][v0, 3] = np.float32(0.0)
    visits, keepv = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    ref, end = _oracle(orc, p, visits, plain)

    asked = []
    fn_t = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)
    inner = fn_t(plain[0])

    def counting(user, n, seg, occluded):
        asked.append(int(n))
        inner(user, n, seg, occluded)

    cb = fn_t(counting)
    probe = (C.cast(cb, C.c_void_p).value, sphere.ctypes.data)
    once = capi.Context(0)                                     # a draw log from the start: one run
    twice = capi.Context(0)                                    # none: the pass is run again with one
    try:
        _setup(once, p, visits, plain)
        _same_counters(_pass(once), ref.counters())
        assert once.degenerate_stats()[0] and once.degenerate_stats()[4] == 0
        check_logs(once, ref)
        _setup(twice, p, visits, probe, log=0)
        _same_counters(_pass(twice), ref.counters())
        assert twice.degenerate_stats()[0] and twice.degenerate_stats()[4] == 1
        check_logs(twice, ref)
        assert twice.get_xor128_state() == end
        assert twice.probe_stats()[1] > 0
        assert twice.probe_stats() == once.probe_stats()
        assert sum(asked) == twice.probe_stats()[0] and len(asked) == twice.probe_stats()[2]
    finally:
        once.close(); twice.close()
        ref.close()
