"""Thin lens with abb_chromatic > 0 under an occlusion probe, across ranks (tl_chroma_probe before tl_chroma_across_ranks in
pota_amd/csrc/lentil_hip.hip).

Every rank asks the renderer about its own items' attempts -- no collective -- and fails the occluded ones before the ranks agree
on the generator's course, so the ranks' draws, mapped to frame-wide visit ids, are a whole-frame context's under the same
occluder record for record, every rank ends at the whole frame's generator state, and the ranks together ask exactly what the
one context asks.  Ranks run as threads on the one GPU (tests/fake_rccl); helpers from test_native_exchange_tl_chroma.
"""
import numpy as np
import pytest

import common
import oracle_lib
from pota_amd import capi, distributed
from test_gpu_parity import _compare_with_whole
from test_native_exchange import fake_rccl  # noqa: F401  (fixture)
from test_native_exchange_tl_chroma import (H, KINDS, M, PASSES, W, _band_ranks, _check, _columns, _interleaved_ranks, _params,
                                            _run_native)

pytestmark = pytest.mark.gpu

SPHERE = np.array([6.0, 2.0, -70.0, 9.0], np.float32)


def _probe(orc):
    return (oracle_lib.sphere_occluder(orc), SPHERE.ctypes.data)


def _whole_probed(orc, p, cols):
    """one context over the whole frame behind the sphere: logs and generator states after every pass, segments asked"""
    visits, keep = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    ctx = capi.Context(0)
    ctx.set_params(p); ctx.set_bokeh(None); ctx.alloc_frame(3, KINDS); ctx.set_draw_log(1 << 22)
    ctx.set_occlusion_probe(*_probe(orc))
    ctx.upload_visits(visits)
    logs, states = [], []
    for _ in range(PASSES):
        ctx.clear_frame(); ctx.redistribute(); ctx.resolve(); ctx.sync()
        assert ctx.counters().worklist_overflow == 0 and ctx.counters().streamed == 0
        logs.append(common.sort_log(ctx.draw_log()))
        states.append(ctx.get_xor128_state())
    ctx.P = p
    return ctx, logs, states, keep


def _compare(orc, world, ranks, step, rows=True):
    p = _params()
    cols = _columns(p)
    whole, wl, ws, wk = _whole_probed(orc, p, cols)
    probed, occluded, calls = whole.probe_stats()
    assert 0 < occluded < probed
    ctxs, ck, bands, gid = ranks(p, cols)
    for ctx in ctxs:
        ctx.set_occlusion_probe(*_probe(orc))
    out = _run_native(ctxs, world, step, gid)
    _check(out, world, wl, ws)
    asked = [ctxs[r].probe_stats() for r in range(world)]
    print("whole frame asked %d (occluded %d); ranks %s" % (probed, occluded, asked))
    assert sum(a[0] for a in asked) == probed
    assert sum(a[1] for a in asked) == occluded
    for rank in range(world):
        assert ctxs[rank].counters().streamed == 0
        _compare_with_whole(ctxs[rank], whole, KINDS, rows=bands[rank] if rows else None)
        ctxs[rank].close()
    whole.close()


@pytest.mark.parametrize("world,bounds", [(2, [0, 23, 64]), (3, [0, 5, 40, 64])], ids=["bands-2", "bands-3"])
def test_probed_bands_match_the_whole_frame(orc, fake_rccl, world, bounds):
    _compare(orc, world, lambda p, cols: _band_ranks(p, cols, world, bounds),
             lambda ctx: distributed.frame_step_bands_native(ctx, H, bounds))


def test_probed_interleaved_rows_match_the_whole_frame(orc, fake_rccl):
    _compare(orc, 2, lambda p, cols: _interleaved_ranks(p, cols, 2), distributed.frame_step_native, rows=False)


def test_the_whole_frame_context_is_the_oracles(orc):
    """... and that whole-frame context is pinned to the single-threaded oracle under the same sphere."""
    import ctypes as C
    p = _params()
    cols = _columns(p)
    whole, wl, ws, wk = _whole_probed(orc, p, cols)
    visits, keep = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    start = None
    for k in range(PASSES):
        ref = oracle_lib.Frame(orc, p, n_aovs=3, kinds=KINDS, keep_log=True)
        ref.set_probe(*_probe(orc))
        if start is not None:
            orc.orc_frame_set_xor128(ref.h, (C.c_uint32 * 4)(*start))
        ref.run(None, None, visits)
        st = (C.c_uint32 * 4)()
        orc.orc_frame_get_xor128(ref.h, st)
        assert np.array_equal(wl[k], common.sort_log(ref.log()))
        assert ws[k] == list(st)
        start = list(st)
        ref.close()
    whole.close()
