"""The scan kernels across visit counts, widths, stream tails and regions (tests/scan_shapes.py), against the oracle.

Each case: which kernel the pass started in (lentil_hip_debug_last_scan) is the one the shape is there to select; counters
and accepted-draw lists equal the oracle's; the frame is within the 1e-5 bar of the fp64 shadows; and on every pixel no draw
reaches -- most of them, tests/test_scan_shape_cases.py -- accumulators, weight and resolved image of every AOV are the
oracle's bit for bit (compared as uint32: a pixel there holds the fp32 sum of its own visits in their order, or nothing at
all).  Twice on one context: the first pass runs in chunks, the second blind, and streamed where the library streams it."""
import ctypes as C

import numpy as np
import pytest

import common
import scan_shapes
from pota_amd import capi
from test_gpu_parity import check_frame, check_logs

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set_up(ctx, case, p, table):
    ctx.set_params(p)
    ctx.set_lens_mode(case["lens_mode"])
    if table is not None:
        ctx.set_lens(table)
        assert ctx.lens_is_compiled()          # (the shipped lenses; lens_mode = 1 runs their tables all the same)
    ctx.set_bokeh(None)
    ctx.alloc_frame(case["K"] + 1, case["kinds"])


def _pass(ctx, visits, clear=True):
    ctx.set_draw_log(1 << 20)
    ctx.upload_visits(visits)
    if clear:
        ctx.clear_frame()
    ctx.redistribute()
    ctx.resolve()
    ctx.sync()
    c = ctx.counters()
    assert c.worklist_overflow == 0
    return c


def _same_counters(c, ref):
    rc = ref.counters()
    assert (c.visits, c.redistributed_visits, c.attempted_draws, c.accepted_draws) == (
        rc.visits, rc.redistributed_visits, rc.attempted_draws, rc.accepted_draws)


def _ran(ctx, case):
    ls = ctx.last_scan()
    assert ls[0] == case["expect_kernel"], "%s ran scan_%s_kernel, the shape is there for scan_%s_kernel (%s)" % (
        case["name"], capi.SCAN_NAMES.get(ls[0]), capi.SCAN_NAMES[case["expect_kernel"]], ls)
    if case["ppt"] is not None:
        assert ls[1] == case["ppt"], ls
    assert ls[3] >= 1


def _bit_exact(ctx, n_aovs, undrawn, want, outside=None, kinds=None):
    """undrawn: pixels no draw reaches; want(a) -> (buffer, weight, image) they must equal bit for bit; outside: pixels that
    must hold nothing at all (the image of a closest-filtered AOV is (r, g, b, 1) everywhere: there, nothing but that alpha)"""
    rec = ctx.download_records()
    for a in range(n_aovs):
        buf, w, img = want(a)
        got = rec[:, 4 * a:4 * a + 4]
        bad = np.flatnonzero((_bits(got)[undrawn] != _bits(buf)[undrawn]).any(axis=1))
        assert bad.size == 0, "AOV %d: accumulators of %d undrawn pixels differ, first pixel %d: %s against %s" % (
            a, bad.size, undrawn[bad[0]], got[undrawn[bad[0]]], buf[undrawn[bad[0]]])
        gimg = ctx.download_aov(a)
        bad = np.flatnonzero((_bits(gimg)[undrawn] != _bits(img)[undrawn]).any(axis=1))
        assert bad.size == 0, "AOV %d: the image differs at %d undrawn pixels, first pixel %d: %s against %s" % (
            a, bad.size, undrawn[bad[0]], gimg[undrawn[bad[0]]], img[undrawn[bad[0]]])
        if a == 0:
            gw = rec[:, 4 * n_aovs]
            bad = np.flatnonzero(_bits(gw)[undrawn] != _bits(w)[undrawn])
            assert bad.size == 0, "the weights of %d undrawn pixels differ, first pixel %d: %r against %r" % (
                bad.size, undrawn[bad[0]], gw[undrawn[bad[0]]], w[undrawn[bad[0]]])
        if outside is not None and outside.size:
            empty = np.zeros(4, np.float32)
            if kinds is not None and kinds[a] != 0:
                empty[3] = 1.0
            assert not _bits(got)[outside].any() and (_bits(gimg)[outside] == _bits(empty)).all(), "AOV %d: pixels outside the stream's region hold something" % a
    if outside is not None and outside.size:
        assert not _bits(rec[:, 4 * n_aovs])[outside].any()


def _undrawn(n_pixels, *logs):
    m = np.ones(n_pixels, bool)
    for log in logs:
        m[log[:, 2]] = False
    return np.flatnonzero(m)


def _check_against(ctx, case, cols, ref):
    n_aovs = case["K"] + 1
    check_logs(ctx, ref)
    check_frame(ctx, ref, n_aovs=n_aovs, kinds=case["kinds"])
    n_pixels = int(np.prod(scan_shapes.frame_shape(case)))
    assert n_pixels == ctx.n_pixels
    undrawn = _undrawn(n_pixels, ref.log())
    held = np.zeros(n_pixels, bool)
    held[scan_shapes.stream_pixels(case, cols)] = True
    rw = ref.weight()
    _bit_exact(ctx, n_aovs, undrawn, lambda a: (ref.buffer(a), rw, ref.resolve(a)), outside=undrawn[~held[undrawn]], kinds=case["kinds"])
    assert 2 * np.count_nonzero(held[undrawn]) >= np.count_nonzero(held)


@pytest.mark.parametrize("case", scan_shapes.CASES, ids=[c["name"] for c in scan_shapes.CASES])
def test_scan_shape(orc, gpu_ctx_factory, monkeypatch, case):
    if case["runs_env"] is None:
        monkeypatch.delenv("LENTIL_SCAN_RUNS", raising=False)
    else:
        monkeypatch.setenv("LENTIL_SCAN_RUNS", case["runs_env"])
    built = scan_shapes.build(case)
    p, table, visits, cols = built
    ref = scan_shapes.oracle(orc, case, built)
    try:
        assert np.isin(cols["planted"], ref.log()[:, 0]).all()
        ctx = gpu_ctx_factory()
        _set_up(ctx, case, p, table)
        for again in (0, 1):
            c = _pass(ctx, visits)
            _ran(ctx, case)
            _same_counters(c, ref)
            if again == 0:
                assert c.streamed == 0 and c.blind_chunks == 0
            elif case["lens_mode"] == 1:
                assert c.streamed == 1 and c.fallback_chunks == 0, ctx.last_redo_note()
            _check_against(ctx, case, cols, ref)
    finally:
        ref.close()


def test_buckets_into_one_frame(orc, gpu_ctx_factory):
    """Four unequal buckets of a 64 x 48 frame, redistributed one after the other into one frame without a clear: the frame
    is the four oracle frames added, and a pixel no draw reaches belongs to one bucket and holds that bucket's oracle value
    bit for bit.  (Each pass after the first finds the direct sums of the one before in FrameDev::dir: fold_direct.)"""
    cases = [scan_shapes.BY_NAME[b] for b in scan_shapes.BUCKETS]
    builts = [scan_shapes.build(c) for c in cases]
    refs = [scan_shapes.oracle(orc, c, b) for c, b in zip(cases, builts)]
    p, table = builts[0][0], builts[0][1]
    # ... added: the oracle over the four streams into one frame (its fp64 shadows are what the 1e-5 bar is taken against)
    whole = common.run_oracle(orc, p, table, builts[0][2], threads=1)
    lens = orc.orc_lens_create(C.byref(table))
    try:
        for b in builts[1:]:
            whole.run(lens, None, b[2])
        ctx = gpu_ctx_factory()
        _set_up(ctx, cases[0], p, table)
        for k, (case, b, ref) in enumerate(zip(cases, builts, refs)):
            c = _pass(ctx, b[2], clear=(k == 0))
            _ran(ctx, case)
            _same_counters(c, ref)
            check_logs(ctx, ref)
        check_frame(ctx, whole)
        n_pixels = ctx.n_pixels
        undrawn = _undrawn(n_pixels, *[r.log() for r in refs])
        assert 2 * undrawn.size >= n_pixels
        buf, w, img = np.zeros((n_pixels, 4), np.float32), np.zeros(n_pixels, np.float32), np.zeros((n_pixels, 4), np.float32)
        for case, b, ref in zip(cases, builts, refs):
            own = np.unique(scan_shapes.stream_pixels(case, b[3]))
            buf[own], w[own], img[own] = ref.buffer(0)[own], ref.weight()[own], ref.resolve(0)[own]
        _bit_exact(ctx, 1, undrawn, lambda a: (buf, w, img))
    finally:
        orc.orc_lens_destroy(lens)
        whole.close()
        for r in refs:
            r.close()


@pytest.mark.parametrize("K", sorted(scan_shapes.STALE))
def test_region_that_changes_between_passes(orc, gpu_ctx_factory, K):
    """A pass over one sub-rectangle, a clear, a pass over another (other x0, y0 and pixels per row) on the same context: the
    frame is the second stream's alone -- what the first left in FrameDev::dir is wiped (prepare_direct), not folded in."""
    ca, cb = (scan_shapes.BY_NAME[n] for n in scan_shapes.STALE[K])
    assert ca["region"][:3] != cb["region"][:3] and all(x != y for x, y in zip(ca["region"][:3], cb["region"][:3]))
    ba, bb = scan_shapes.build(ca), scan_shapes.build(cb)
    ra, rb = scan_shapes.oracle(orc, ca, ba), scan_shapes.oracle(orc, cb, bb)
    try:
        ctx = gpu_ctx_factory()
        _set_up(ctx, ca, ba[0], ba[1])
        for case, b, ref in ((ca, ba, ra), (cb, bb, rb), (ca, ba, ra)):
            c = _pass(ctx, b[2])
            _ran(ctx, case)
            _same_counters(c, ref)
            _check_against(ctx, case, b[3], ref)
    finally:
        ra.close()
        rb.close()
