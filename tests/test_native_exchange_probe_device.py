"""Thin lens with abb_chromatic > 0 under a DEVICE occlusion callback, across ranks (tl_chroma_probe before
tl_chroma_across_ranks in pota_amd/csrc/lentil_hip.hip).

tests/test_native_exchange_tl_chroma_probe.py with lentil_hip_set_occlusion_probe_device on every rank: each rank asks its own
callback about its own items -- on its own stream, no collective --, and the ranks' draws, mapped to frame-wide visit ids, are
the whole-frame context's record for record, every rank ends at the whole frame's generator state, and the whole-frame context
is the single-threaded oracle's.  Ranks run as threads on the one GPU (tests/fake_rccl).
"""
import ctypes as C

import numpy as np
import pytest

import common
import oracle_lib
import probe_device_cases as pc
from pota_amd import capi, distributed
from test_gpu_parity import _compare_with_whole
from test_native_exchange import fake_rccl  # noqa: F401  (fixture)
from test_native_exchange_tl_chroma import H, KINDS, M, PASSES, W, _band_ranks, _check, _columns, _params, _run_native

pytestmark = pytest.mark.gpu

CASE = pc.BY_NAME["tlc-ranks"]
SPHERE = np.array(CASE["sphere"], np.float32)


def _device(ctx):
    ctx.set_occlusion_probe_device(capi.sphere_occluder_device(), SPHERE.ctypes.data)


def test_two_bands_under_the_device_callback(orc, fake_rccl):
    world, bounds = 2, [0, 23, 64]
    p = _params()
    cols = _columns(p)
    visits, keep = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    whole = capi.Context(0)
    whole.set_params(p); whole.set_bokeh(None); whole.alloc_frame(3, KINDS); whole.set_draw_log(1 << 22)
    _device(whole)
    whole.upload_visits(visits)
    wl, ws = [], []
    start = None
    for k in range(PASSES):
        whole.clear_frame(); whole.redistribute(); whole.resolve(); whole.sync()
        assert whole.counters().worklist_overflow == 0 and whole.counters().streamed == 0
        wl.append(common.sort_log(whole.draw_log()))
        ws.append(whole.get_xor128_state())
        # ... which is the single-threaded oracle's under the same sphere
        ref = oracle_lib.Frame(orc, p, n_aovs=3, kinds=KINDS, keep_log=True)
        ref.set_probe(oracle_lib.sphere_occluder(orc), SPHERE.ctypes.data)
        if start is not None:
            orc.orc_frame_set_xor128(ref.h, (C.c_uint32 * 4)(*start))
        ref.run(None, None, visits)
        st = (C.c_uint32 * 4)()
        orc.orc_frame_get_xor128(ref.h, st)
        assert np.array_equal(wl[k], common.sort_log(ref.log()))
        assert ws[k] == list(st)
        if k == 0:                  # (the table's case is this stream: what tests/test_probe_device_cases.py checked bites)
            assert np.array_equal(wl[0], pc.sorted_log(pc.oracle(orc, CASE)))
        start = list(st)
        ref.close()
    whole.P = p
    probed, occluded, calls = whole.probe_stats()
    assert 0 < occluded < probed
    ctxs, ck, bands, gid = _band_ranks(p, cols, world, bounds)
    for ctx in ctxs:
        _device(ctx)
    out = _run_native(ctxs, world, lambda ctx: distributed.frame_step_bands_native(ctx, H, bounds), gid)
    _check(out, world, wl, ws)
    asked = [ctxs[r].probe_stats() for r in range(world)]
    print("whole frame asked %d (occluded %d); ranks %s; device stats %s" % (probed, occluded, asked, [c.probe_device_stats() for c in ctxs]))
    assert sum(a[0] for a in asked) == probed and sum(a[1] for a in asked) == occluded
    for rank in range(world):
        assert ctxs[rank].counters().streamed == 0
        assert ctxs[rank].probe_device_stats()[0] == asked[rank][2] > 0
        _compare_with_whole(ctxs[rank], whole, KINDS, rows=bands[rank])
        ctxs[rank].close()
    whole.close()
