"""Occlusion probes answered on the GPU (include/lentil_hip.h: lentil_hip_set_occlusion_probe_device).

A renderer whose scene lives in device memory answers a round's segments where they are written: no list over PCIe, no host
wait in the round.  The "scene" is the analytic sphere -- the library's lentil_hip_test_sphere_occluder_device on the GPU, the
oracle's orc_sphere_occluder on the CPU, the same fp64 operations in the same order -- and the bar is the suite's own:
accepted-draw lists bit for bit (check_logs), radiance at 1e-5 (check_frame), counters equal.  The cases are those of
tests/probe_device_cases.py, which tests/test_probe_device_cases.py holds to "the sphere bites" on the oracle alone; the
oracle's runs are shared (probe_device_cases.oracle).
"""
import ctypes as C

import numpy as np
import pytest

import common
import oracle_lib
import probe_device_cases as pc
from pota_amd import _abi, capi
from test_gpu_parity import check_frame, check_logs

pytestmark = pytest.mark.gpu


def _context(monkeypatch, case):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    return capi.Context(0)


def _setup(ctx, case, ref, log=1 << 22):
    p, table, visits, sphere, c2w, keep = pc.setup(case)
    ctx.keep = (p, table, visits, sphere, c2w, keep)
    ctx.set_params(p)
    if table is not None:
        ctx.set_lens(table)
    ctx.set_bokeh(None)
    ctx.alloc_frame(pc.n_aovs(case), pc.kinds(case))
    ctx.set_draw_log(log)
    ctx.upload_visits(visits)
    return sphere, c2w


def _device(ctx, sphere, c2w=None):
    ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), sphere.ctypes.data, c2w)


def _host(ctx, orc, sphere, c2w=None):
    ctx.set_occlusion_probe(oracle_lib.sphere_occluder(orc), sphere.ctypes.data, c2w)


def _pass(ctx):
    ctx.clear_frame(); ctx.redistribute(); ctx.resolve(); ctx.sync()
    c = ctx.counters()
    assert c.worklist_overflow == 0 and c.streamed == 0
    return c


def _same_counters(c, rc):
    assert (c.redistributed_visits, c.attempted_draws, c.accepted_draws) == (rc.redistributed_visits, rc.attempted_draws, rc.accepted_draws)


def _is_the_oracles(ctx, case, ref, c):
    _same_counters(c, ref.counters())
    check_logs(ctx, ref)
    check_frame(ctx, ref, n_aovs=pc.n_aovs(case), kinds=pc.kinds(case))


def _bites(orc, case, stats):
    """what every parity case asserts beside parity: the sphere occluded some segments and not all, and the oracle's probed
    list is not its unprobed one"""
    probed, occluded = stats[:2]
    assert 0 < occluded < probed, (probed, occluded)
    fl, rl = pc.sorted_log(pc.oracle(orc, case, "free")), pc.sorted_log(pc.oracle(orc, case, "probed"))
    assert fl.shape != rl.shape or not np.array_equal(fl, rl)


@pytest.mark.parametrize("name", ["po", "tl"])
def test_two_passes_are_the_oracles_and_the_second_has_no_host_wait(orc, monkeypatch, name):
    """Three chunk streams probe side by side.  The first pass of a context reads every chunk's scan back and sizes the lists
    from it; the second is enqueued blind, sized from the first's figures -- and the library waits for nothing on behalf of the
    probes in either (the lists are made with the capacity of the chunk's result pool, which bounds every round's).  The list is the host form's list: a second context under the host callback (whose chunks now have
    list buffers of their own, too) counts the same segments and the same occluded answers."""
    case = pc.BY_NAME[name]
    ref = pc.oracle(orc, case)
    dev, host = _context(monkeypatch, case), capi.Context(0)
    try:
        sphere, _ = _setup(dev, case, ref)
        _device(dev, sphere)
        _is_the_oracles(dev, case, ref, _pass(dev))
        first = dev.probe_device_stats()
        assert first[0] >= 3 and first[1] == 0 and first[2] == 0 and first[3] > 1000, first
        c = _pass(dev)
        _is_the_oracles(dev, case, ref, c)
        second = dev.probe_device_stats()
        print("%s: probe_stats %s device stats %s -> %s, blind chunks %d, fallback chunks %d" %
              (name, dev.probe_stats(), first, second, c.blind_chunks, c.fallback_chunks))
        assert second[1] == first[1] and c.blind_chunks > 0
        assert second[2] == 0 and c.fallback_chunks == 0
        assert dev.probe_stats()[2] == second[0] > first[0]
        hs, _ = _setup(host, case, ref)
        _host(host, orc, hs)
        for _ in range(2):
            _is_the_oracles(host, case, ref, _pass(host))
        assert dev.probe_stats()[:2] == host.probe_stats()[:2]
        assert host.probe_device_stats() == (0, 0, 0, 0)
        _bites(orc, case, dev.probe_stats())
    finally:
        dev.close(); host.close()


def test_a_list_longer_than_the_apply_grid(orc, monkeypatch):
    """Round 0 of this case lists more segments than probe_apply_device_kernel's grid has lanes (num_cu * 4 * 256), so its lanes
    go round the grid-stride loop more than once and the last turn is a partial one.  samples_override = 254 is the smallest
    that gets there at 96 x 64 with one chunk: measured on an MI355X (256 CUs: 262 144 lanes), the longest list has 261 792
    segments at 253, 262 700 at 254, 263 630 at 255 and 264 530 at 256."""
    import torch
    case = pc.BY_NAME["po-long"]
    ref = pc.oracle(orc, case)
    ctx = _context(monkeypatch, case)
    try:
        sphere, _ = _setup(ctx, case, ref)
        _device(ctx, sphere)
        _is_the_oracles(ctx, case, ref, _pass(ctx))
        lanes = torch.cuda.get_device_properties(0).multi_processor_count * pc.APPLY_GRID_LANES_PER_CU
        longest = ctx.probe_device_stats()[3]
        print("longest list %d, apply grid %d lanes" % (longest, lanes))
        assert longest > lanes, (longest, lanes)
        _is_the_oracles(ctx, case, ref, _pass(ctx))             # (blind)
        assert ctx.probe_device_stats()[1:3] == (0, 0)
        _bites(orc, case, ctx.probe_stats())
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["no-highlights", "radius-0", "lens-swallowed"])
def test_degenerate_lists(orc, monkeypatch, name):
    """Nothing to list; a list nothing of which is occluded; a list all of which is."""
    case = pc.BY_NAME[name]
    ref, free = pc.oracle(orc, case), pc.oracle(orc, case, "free")
    ctx = _context(monkeypatch, case)
    try:
        sphere, _ = _setup(ctx, case, ref)
        _device(ctx, sphere)
        for _ in range(2):
            c = _pass(ctx)
            _is_the_oracles(ctx, case, ref, c)
            assert c.accepted_draws == ref.counters().accepted_draws
        probed, occluded, calls = ctx.probe_stats()
        if name == "no-highlights":
            assert (probed, occluded) == (0, 0) and ref.counters().redistributed_visits == 0
            check_frame(ctx, free, n_aovs=pc.n_aovs(case))
        elif name == "radius-0":
            assert occluded == 0 and probed > 1000
            check_logs(ctx, free)
            check_frame(ctx, free, n_aovs=pc.n_aovs(case))
        else:
            assert occluded == probed > 1000 and c.accepted_draws == 0 and free.counters().accepted_draws > 0
    finally:
        ctx.close()


def test_a_list_that_does_not_fit(orc, monkeypatch):
    """LENTIL_PROBE_DEVICE_CAP=64: the blind pass's lists may hold 64 segments and round 0 lists thousands.  The apply kernel
    sees it, nothing of the round is accepted, the chunks' draws are redone with each list counted on the host first -- the
    frame is still the oracle's, and the pass says what happened."""
    case = pc.BY_NAME["overflow"]
    ref = pc.oracle(orc, case)
    ctx = _context(monkeypatch, case)
    try:
        sphere, _ = _setup(ctx, case, ref)
        _device(ctx, sphere)
        _is_the_oracles(ctx, case, ref, _pass(ctx))             # (sized from the scan's read-back: the cap is a blind pass's)
        first = ctx.probe_device_stats()
        assert first[1] == 0 and first[2] == 0
        c = _pass(ctx)
        _is_the_oracles(ctx, case, ref, c)
        second = ctx.probe_device_stats()
        print("device stats %s -> %s; fallback chunks %d; note: %s" % (first, second, c.fallback_chunks, ctx.last_redo_note()))
        assert c.blind_chunks > 0 and c.fallback_chunks >= 1 and c.worklist_overflow == 0
        assert second[2] > 0 and second[1] > first[1] and second[3] > 64
        assert "occlusion probes" in ctx.last_redo_note()
        hs = capi.Context(0)
        try:
            s2, _ = _setup(hs, case, ref)
            _host(hs, orc, s2)
            for _ in range(2):
                _pass(hs)
            assert ctx.probe_stats()[:2] == hs.probe_stats()[:2]         # (the overflowed lists were not counted twice)
        finally:
            hs.close()
        _bites(orc, case, ctx.probe_stats())
    finally:
        ctx.close()


def test_sub_batches_under_the_device_callback(orc, monkeypatch):
    """LENTIL_MAX_POOL_UNITS=20000 with five chunks: every chunk's draws exceed the result pool and go through the sub-batch
    loop of enqueue_chunk_draws.  That the loop ran is read off the second pass: a chunk that fits its pool is enqueued blind
    there (an unconstrained context's chunks are), a chunk in sub-batches never is."""
    case = pc.BY_NAME["sub-batches"]
    ref = pc.oracle(orc, case)
    ctx = _context(monkeypatch, case)
    try:
        sphere, _ = _setup(ctx, case, ref)
        _device(ctx, sphere)
        for _ in range(2):
            c = _pass(ctx)
            _is_the_oracles(ctx, case, ref, c)
        assert c.blind_chunks == 0, c.blind_chunks
        assert ctx.probe_device_stats()[1:3] == (0, 0)
        _bites(orc, case, ctx.probe_stats())
    finally:
        ctx.close()
    monkeypatch.delenv("LENTIL_MAX_POOL_UNITS")
    free = capi.Context(0)
    try:
        sphere, _ = _setup(free, case, ref)
        _device(free, sphere)
        for _ in range(2):
            c = _pass(free)
        assert c.blind_chunks > 0
    finally:
        free.close()


def test_the_occluder_changes_between_passes_of_one_context(orc, monkeypatch):
    """The sphere is read at call time, so a renderer's scene may change from pass to pass.  Radius 0, then a sphere that swallows
    the lens, then radius 0 again, on one context whose second and third passes are enqueued blind: with nothing occluded
    every item is done after round 0; with everything occluded every item goes on to its remaining 4 x samples attempts and a
    later round lists several times what any list of the pass before held.  The lists are made with the result pool's capacity,
    which bounds every round's: nothing overflows, no host wait is made, and each frame is the oracle's for its sphere."""
    none, every = pc.BY_NAME["radius-0"], pc.BY_NAME["lens-swallowed"]
    assert pc.stream_key(none)[:4] == pc.stream_key(every)[:4]           # (one stream, two spheres)
    ctx = _context(monkeypatch, none)
    try:
        sphere, _ = _setup(ctx, none, None)
        _device(ctx, sphere)
        longest = []
        for k, case in enumerate((none, every, none, every)):
            sphere[:] = np.array(case["sphere"], np.float32)
            before = ctx.probe_device_stats()
            c = _pass(ctx)
            _is_the_oracles(ctx, case, pc.oracle(orc, case), c)
            after = ctx.probe_device_stats()
            longest.append(after[3])
            print("pass %d (%s): blind chunks %d, fallback chunks %d, device stats %s" % (k, case["name"], c.blind_chunks, c.fallback_chunks, after))
            assert after[1] == before[1] and after[2] == 0 and c.fallback_chunks == 0
            assert (c.blind_chunks > 0) == (k > 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["moved-given", "moved-null"])
def test_a_camera_away_from_the_origin(orc, monkeypatch, name):
    case = pc.BY_NAME[name]
    ref = pc.oracle(orc, case)
    ctx = _context(monkeypatch, case)
    try:
        sphere, c2w = _setup(ctx, case, ref)
        assert (c2w is not None) == (name == "moved-given")
        _device(ctx, sphere, c2w)
        for _ in range(2):
            _is_the_oracles(ctx, case, ref, _pass(ctx))
        _bites(orc, case, ctx.probe_stats())
    finally:
        ctx.close()


def _tlc_oracle_from(orc, case, start):
    p, table, visits, sphere, c2w, keep = pc.setup(case)
    ref = oracle_lib.Frame(orc, p, n_aovs=pc.n_aovs(case), kinds=pc.kinds(case), keep_log=True)
    ref.set_probe(oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
    orc.orc_frame_set_xor128(ref.h, (C.c_uint32 * 4)(*start))
    ref.run(None, None, visits)
    st = (C.c_uint32 * 4)()
    orc.orc_frame_get_xor128(ref.h, st)
    return ref, list(st)


def test_thin_lens_with_chromatic_aberration(orc, monkeypatch):
    """abb_chromatic = 0.6: the loop of tl_chroma_probe keeps two 4-byte read-backs per turn, the segments stay on the device.
    Two passes, the second continuing the generator: logs, frame and xor128 state are the oracle's; the segments asked about
    are the host form's, turn for turn."""
    case = pc.BY_NAME["tlc"]
    ref = pc.oracle(orc, case)
    dev, host = _context(monkeypatch, case), capi.Context(0)
    try:
        sphere, _ = _setup(dev, case, ref)
        _device(dev, sphere)
        _is_the_oracles(dev, case, ref, _pass(dev))
        assert dev.get_xor128_state() == ref.xor128_end
        ref2, end2 = _tlc_oracle_from(orc, case, ref.xor128_end)
        _is_the_oracles(dev, case, ref2, _pass(dev))
        assert dev.get_xor128_state() == end2
        ref2.close()
        hs, _ = _setup(host, case, ref)
        _host(host, orc, hs)
        for _ in range(2):
            _pass(host)
        assert host.get_xor128_state() == end2
        assert dev.probe_stats() == host.probe_stats()
        lists, waits, overflows, longest = dev.probe_device_stats()
        assert lists == dev.probe_stats()[2] and waits >= 2 * lists and overflows == 0 and longest > 1000
        _bites(orc, case, dev.probe_stats())
    finally:
        dev.close(); host.close()


def test_a_pass_run_again_does_not_call_back_again(orc, monkeypatch):
    """test_a_pass_run_again_does_not_ask_again under the device callback: a closest-AOV candidate at depth 0 in a context
    without a draw log has the pass run twice; the second run fails what the first found occluded and calls nothing."""
    case = pc.BY_NAME["tlc-rerun"]
    p, table, visits, sphere, c2w, keep = pc.setup(case)
    cols = keep[2]
    v0 = int(pc.sorted_log(pc.oracle(orc, case))[0, 0])                # a redistributed visit with accepted draws
    cols["pos_z"][v0, 3] = np.float32(0.0)
    visits, keepv = capi.make_visits(cols, visits_per_pixel=pc.M, pixels_per_row=pc.W)
    ref = oracle_lib.Frame(orc, p, n_aovs=3, kinds=pc.KINDS_TLC, keep_log=True)
    ref.set_probe(oracle_lib.sphere_occluder(orc), sphere.ctypes.data)
    ref.run(None, None, visits)
    once, twice = capi.Context(0), capi.Context(0)
    try:
        for ctx, log in ((once, 1 << 22), (twice, 0)):
            ctx.set_params(p); ctx.set_bokeh(None); ctx.alloc_frame(3, pc.KINDS_TLC); ctx.set_draw_log(log)
            _device(ctx, sphere)
            ctx.upload_visits(visits)
            _same_counters(_pass(ctx), ref.counters())
            check_logs(ctx, ref)
        assert once.degenerate_stats()[0] and once.degenerate_stats()[4] == 0
        assert twice.degenerate_stats()[0] and twice.degenerate_stats()[4] == 1
        assert twice.probe_stats()[1] > 0
        assert twice.probe_stats() == once.probe_stats()                # (segments, occluded answers and callback calls of ONE run)
        assert twice.probe_device_stats()[0] == once.probe_device_stats()[0]
    finally:
        once.close(); twice.close()
        ref.close()


def test_switching_between_device_host_and_none(orc, monkeypatch):
    case = pc.BY_NAME["po"]
    ref, free = pc.oracle(orc, case), pc.oracle(orc, case, "free")
    ctx = capi.Context(0)
    try:
        sphere, _ = _setup(ctx, case, ref)
        _device(ctx, sphere)
        _is_the_oracles(ctx, case, ref, _pass(ctx))
        lists = ctx.probe_device_stats()[0]
        _host(ctx, orc, sphere)                                       # replaces the device callback
        _is_the_oracles(ctx, case, ref, _pass(ctx))
        assert ctx.probe_device_stats()[0] == lists
        _device(ctx, sphere)                                          # ... and back: the answer bytes the host form left are wiped
        _is_the_oracles(ctx, case, ref, _pass(ctx))
        assert ctx.probe_device_stats()[0] > lists
        ctx.set_occlusion_probe_device(None)
        before = ctx.probe_stats()
        for _ in range(2):
            ctx.clear_frame(); ctx.redistribute(); ctx.resolve(); ctx.sync()
        check_logs(ctx, free)
        check_frame(ctx, free, n_aovs=pc.n_aovs(case))
        assert ctx.probe_stats() == before
    finally:
        ctx.close()


def test_a_callback_that_fails_fails_the_pass_and_the_context_stays_usable(orc):
    case = pc.BY_NAME["po"]
    ref = pc.oracle(orc, case)
    ctx = capi.Context(0)
    try:
        sphere, _ = _setup(ctx, case, ref)
        ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), None)      # user == NULL: returns 1, enqueues nothing
        ctx.clear_frame()
        with pytest.raises(capi.LentilError) as e:
            ctx.redistribute()
        assert e.value.code == _abi.ERR_INVALID
        assert "returned 1" in str(e.value)
        _device(ctx, sphere)
        for _ in range(2):
            _is_the_oracles(ctx, case, ref, _pass(ctx))
    finally:
        ctx.close()


def test_polynomial_optics_with_chromatic_aberration_stays_refused(orc):
    p, model, table, keep = common.po_setup(32, 24, samples_override=16, abb_chromatic=0.5)
    visits, cols = common.make_stream(p, 32, 24, pc.M, f_hi=0.05)
    sphere = np.array([0, 0, -70.0, 5.0], np.float32)
    ctx = capi.Context(0)
    try:
        ctx.set_params(p); ctx.set_lens(table); ctx.alloc_frame(1)
        _device(ctx, sphere)
        ctx.upload_visits(visits)
        ctx.clear_frame()
        with pytest.raises(capi.LentilError) as e:
            ctx.redistribute()
        assert e.value.code == _abi.ERR_UNSUPPORTED
        assert "polynomial optics" in str(e.value)
        assert ctx.probe_stats() == (0, 0, 0) and ctx.probe_device_stats() == (0, 0, 0, 0)
    finally:
        ctx.close()
