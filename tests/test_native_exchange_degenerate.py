"""Closest-filtered AOVs with candidates at depth (Z) 0 or NaN across ranks (lentil_closest_replay.h, degenerate_exchange in
pota_amd/csrc/lentil_comm.h).

src/lentil.h:832-845 uses a z-buffer value of 0 as "empty", so at a pixel that sees such a candidate the outcome depends on the
ORDER of the candidates there -- on every rank.  The native exchanges replay those pixels over every rank's candidates in
frame-wide visit order; each band / frame must equal a whole-frame context (which test_degenerate_depths_and_closest_aovs pins
to the single-threaded oracle) bit for bit on the closest and lentil_debug planes.  The torch forms cannot replay and must
refuse such a frame on every rank at once.  Ranks run as threads on the one GPU (tests/fake_rccl), as in test_native_exchange.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import common
import oracle_lib
from pota_amd import _abi, capi, distributed, workload
from test_gpu_parity import _compare_with_whole, _InProcessDist, gpu_run
from test_native_exchange import _threads, fake_rccl  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

W, H, M = 64, 45, 9
KINDS = [_abi.FILTER_GAUSSIAN, _abi.FILTER_CLOSEST, _abi.FILTER_CLOSEST_DEBUG]
DEG_ROWS = 22          # degenerate depths only in visit rows below this: the last rank of every partition below has none
BOUNDARIES = (2, 4, 9, 15, 22)       # the band boundaries below it


def _columns(p):
    cols = workload.generate(np, 0, W * H * M, W, H, M, f_hi=0.03, focus_dist=150.0, tan_half_fov=common.tan_half_fov(p), n_extra=2)
    cols["extra"][1] = None                # lentil_debug has no visit column
    return cols


def _degenerate_visits(cols, p, table, gpu_ctx_factory):
    """Visits to give depth 0 / -0 / NaN, chosen from a whole-frame context's draw log: at pixels whose candidates come from
    rows on both sides of DEG_ROWS the earliest candidate is degenerate (a zero a later rank must override, a NaN that keeps
    the pixel against later positive depths), one such pixel gets 0 / NaN / -0 on its first three candidates, and visits that
    stay in their own pixel are degenerate beside redistributed ones."""
    visits, keep = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    ctx = gpu_ctx_factory()
    gpu_run(ctx, p, table, visits, n_aovs=3, kinds=KINDS)
    log = ctx.draw_log()
    ctx.close()
    row_of = lambda v: int(v) // (W * M)
    by_pixel = {}
    for v, _, px in log:
        by_pixel.setdefault(int(px), set()).add(int(v))
    low = lambda vs: [v for v in sorted(vs) if row_of(v) < DEG_ROWS]
    kinds_cycle = [np.float32(0.0), np.float32(np.nan), np.float32(-0.0)]
    depth, used = {}, set()
    # the mixture: 0 / NaN / -0 on the first three candidates of one pixel, which later rows reach too
    mixed = [px for px, vs in sorted(by_pixel.items()) if len(low(vs)) >= 3 and max(vs) >= DEG_ROWS * W * M] or \
        [px for px, vs in sorted(by_pixel.items()) if len(low(vs)) >= 3]
    for v, d in zip(low(by_pixel[mixed[0]])[:3], kinds_cycle):
        depth[v] = d
        used.add(v)
    # at every band boundary of the partitions below: the earliest candidate of pixels that rows on both sides reach -- a zero
    # a later rank overrides, a NaN that keeps the pixel against the later ranks' depths
    k = 0
    for b in BOUNDARIES:
        crossing = [px for px, vs in sorted(by_pixel.items()) if min(vs) < b * W * M <= max(vs) and px != mixed[0]]
        assert len(crossing) >= 2, "too few pixels with candidates from both sides of row %d" % b
        for px in crossing[:4]:
            v = sorted(by_pixel[px])[0]
            if v in used:
                continue
            depth[v] = kinds_cycle[k % 3]
            used.add(v)
            k += 1
    redistributed = set(int(v) for v in log[:, 0])
    direct = [v for v in range(0, DEG_ROWS * W * M, 97) if v not in redistributed][:6]
    for i, v in enumerate(direct):                          # visits that stay in their own pixel
        depth[v] = kinds_cycle[i % 2]
    assert direct
    return depth


@pytest.fixture(scope="module")
def frame(orc):
    """(params, table, keepalive, columns with the degenerate depths, columns with every depth positive)"""
    p, model, table, keep = common.po_setup(W, H, samples_override=48)
    clean = _columns(p)
    factory = lambda: capi.Context(0)
    depth = _degenerate_visits(clean, p, table, factory)
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in clean.items()}
    for v, d in depth.items():
        bad["pos_z"][v, 3] = d
    return p, table, keep, bad, clean


def _whole(p, table, cols):
    visits, keep = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    whole = capi.Context(0)
    gpu_run(whole, p, table, visits, n_aovs=3, kinds=KINDS)
    whole.P = p
    return whole, keep


def _slice(cols, idx):
    out = {}
    for k, v in cols.items():
        if k == "extra":
            out[k] = [None if e is None else np.ascontiguousarray(e[idx]) for e in v]
        elif isinstance(v, np.ndarray):
            out[k] = np.ascontiguousarray(v[idx])
        else:
            out[k] = v
    return out


def _context(p, table, cols, kinds=KINDS, **layout):
    v, kv = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W, **layout)
    ctx = capi.Context(0)
    ctx.set_params(p); ctx.set_lens(table); ctx.set_bokeh(None)
    ctx.alloc_frame(3, kinds)
    ctx.upload_visits(v)            # (no draw log: a rank that needs one runs its first pass again)
    return ctx, (cols, v, kv)


def _band_ranks(p, table, cols, world, bounds, kinds=KINDS):
    ctxs, keep, bands = [], [], []
    for rank in range(world):
        b_lo, b_hi = distributed.band_of(rank, world, H, p.yres, bounds)
        ctx, k = _context(p, table, _slice(cols, slice(b_lo * W * M, min(b_hi, H) * W * M)), kinds, pixel_y0=b_lo)
        ctxs.append(ctx); keep.append(k); bands.append((b_lo, b_hi))
    return ctxs, keep, bands


def _interleaved_ranks(p, table, cols, world, kinds=KINDS):
    ctxs, keep = [], []
    for rank in range(world):
        rows = np.arange(rank, H, world)
        idx = (rows[:, None] * (W * M) + np.arange(W * M)[None, :]).reshape(-1)
        ctx, k = _context(p, table, _slice(cols, idx), kinds, pixel_y0=rank, pixel_row_stride=world)
        ctxs.append(ctx); keep.append(k)
    return ctxs, keep


def _run_native(ctxs, world, step):
    uid = capi.Context.comm_unique_id()
    stats = {}

    def rank_fn(rank):
        ctx = ctxs[rank]
        ctx.comm_init(uid, rank, world)
        stats[rank] = []
        for _ in range(2):                      # the second pass keeps a draw log from its start: nothing runs twice
            step(ctx)
            ctx.sync()
            stats[rank].append((ctx.degenerate_stats(), ctx.exchange_stats()))
        ctx.comm_destroy()

    _threads(rank_fn, world)
    return stats


def _check_stats(stats, world, bands):
    first = [stats[r][0][0] for r in range(world)]
    second = [stats[r][1][0] for r in range(world)]
    assert any(s[0] for s in first)                           # some rank met a degenerate depth ...
    if bands:
        assert not first[-1][0]                               # ... the last band's did not, and still holds candidates
    assert all(s[1] > 0 for s in first + second)              # flagged pixels, the same count on every rank
    assert len(set(s[1] for s in first)) == 1
    assert any(s[2] > 0 for s in first) and any(s[3] > 0 for s in first)     # nodes did cross ranks
    assert sum(s[2] for s in first) == sum(s[3] for s in first)
    assert all(s[4] == 1 for s in first)                      # no rank had a log: every one ran its pass again ...
    assert all(s[4] == 0 for s in second)                     # ... once


@pytest.mark.parametrize("world,bounds,sparse", [(2, None, True), (3, [0, 9, 31, 45], True), (4, [0, 2, 4, 30, 45], True),
                                                 (3, None, False)],
                         ids=["fixed-2", "fixed-3-unequal", "fixed-4-thin-bands", "sized-3"])
def test_bands_replay_degenerate_depths(frame, fake_rccl, monkeypatch, world, bounds, sparse):
    """lentil_hip_exchange_bands (fixed-capacity and sized form): every band equals the same rows of the whole frame."""
    p, table, keep, bad, clean = frame
    monkeypatch.setattr(distributed, "SPARSE_EXCHANGE", sparse)
    whole, wk = _whole(p, table, bad)
    ctxs, ck, bands = _band_ranks(p, table, bad, world, bounds)
    stats = _run_native(ctxs, world, lambda ctx: distributed.frame_step_bands_native(ctx, H, bounds))
    _check_stats(stats, world, True)
    for rank in range(world):
        _compare_with_whole(ctxs[rank], whole, [0, 1, 1], rows=bands[rank])
        ctxs[rank].close()
    whole.close()


@pytest.mark.parametrize("world", [2, 3])
def test_interleaved_replay_degenerate_depths(orc, frame, fake_rccl, world):
    """lentil_hip_allreduce: every rank holds the whole frame, equal to the whole-frame context and, on the closest planes,
    to the single-threaded oracle bit for bit."""
    p, table, keep, bad, clean = frame
    whole, wk = _whole(p, table, bad)
    ctxs, ck = _interleaved_ranks(p, table, bad, world)
    stats = _run_native(ctxs, world, distributed.frame_step_native)
    _check_stats(stats, world, False)
    ocols = dict(bad); ocols["extra"] = [bad["extra"][0], np.zeros_like(bad["rgba"])]
    ovisits, okeep = capi.make_visits(ocols, visits_per_pixel=M, pixels_per_row=W)
    lens = orc.orc_lens_create(C.byref(table))
    ref = oracle_lib.Frame(orc, p, n_aovs=3, kinds=KINDS, keep_log=True)
    ref.run(lens, None, ovisits)
    orc.orc_lens_destroy(lens)
    for rank in range(world):
        _compare_with_whole(ctxs[rank], whole, [0, 1, 1])
        for a in (1, 2):
            assert np.array_equal(ctxs[rank].download_aov(a).view(np.uint32), ref.resolve(a).view(np.uint32))
        ctxs[rank].close()
    ref.close()
    whole.close()


@pytest.mark.parametrize("partition", ["bands", "interleaved"])
def test_clean_frames_cost_nothing_extra(frame, fake_rccl, partition):
    """The same frames with every depth positive: no pixel flagged, no node sent, no pass run twice, and the exchange's
    bytes are those of the frame alone."""
    p, table, keep, bad, clean = frame
    world = 3
    whole, wk = _whole(p, table, clean)
    if partition == "bands":
        ctxs, ck, bands = _band_ranks(p, table, clean, world, None)
        step = lambda ctx: distributed.frame_step_bands_native(ctx, H)
    else:
        ctxs, ck = _interleaved_ranks(p, table, clean, world)
        bands = [None] * world
        step = distributed.frame_step_native
    stats = _run_native(ctxs, world, step)
    for rank in range(world):
        for deg, xch in stats[rank]:
            assert deg == (0, 0, 0, 0, 0)
        if partition == "interleaved":
            np_ = p.xres * p.yres
            stride = (4 * 3 + 1 + 7) // 8 * 8
            body = np_ * stride * 4 + 2 * np_ * 8
            assert stats[rank][1][1] == (body * 2 * (world - 1) // world,) * 2
        _compare_with_whole(ctxs[rank], whole, [0, 1, 1], rows=bands[rank])
        ctxs[rank].close()
    whole.close()


def _torch_ranks(fn, world, timeout=240):
    """fn(rank, dist) on one thread per rank; -> {rank: exception or None}.  A rank still running after `timeout` (left in a
    collective) fails the test."""
    shared = _InProcessDist._Shared(world)
    result = {}

    def run(rank):
        try:
            fn(rank, _InProcessDist(shared, rank))
            result[rank] = None
        except Exception as e:
            result[rank] = e

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in th), "a rank is left waiting in a collective"
    return result


@pytest.mark.parametrize("form", ["bands", "interleaved"])
def test_torch_forms_refuse_on_every_rank(frame, form):
    """distributed.frame_step_bands / frame_step cannot replay: a degenerate frame raises on EVERY rank, none hangs, none
    returns a frame (the tiled form used to return a silently wrong one)."""
    p, table, keep, bad, clean = frame
    world = 3
    # (without the library's communicator lentil_debug cannot travel at all: a gaussian AOV in its place)
    kinds = [_abi.FILTER_GAUSSIAN, _abi.FILTER_CLOSEST, _abi.FILTER_GAUSSIAN]
    bad, clean = dict(bad), dict(clean)
    bad["extra"] = [bad["extra"][0], bad["extra"][0]]
    clean["extra"] = [clean["extra"][0], clean["extra"][0]]
    ranks = (lambda cols: _band_ranks(p, table, cols, world, None, kinds)) if form == "bands" else \
        (lambda cols: _interleaved_ranks(p, table, cols, world, kinds))
    ctxs = ranks(bad)[0]
    engines = [distributed.HipEngine(c, rows=p.yres) for c in ctxs]

    def step(rank, dist):
        if form == "bands":
            distributed.frame_step_bands(engines[rank], dist, H, p.yres)
        else:
            distributed.frame_step(engines[rank], dist)
        engines[rank].ctx.sync()

    result = _torch_ranks(step, world)
    for rank in range(world):
        assert isinstance(result[rank], capi.LentilError), "rank %d: %r" % (rank, result[rank])
        assert result[rank].code == _abi.ERR_UNSUPPORTED
    # the same frame with every depth positive goes through
    cctxs = ranks(clean)[0]
    cengines = [distributed.HipEngine(c, rows=p.yres) for c in cctxs]
    engines[:] = cengines
    result = _torch_ranks(step, world)
    assert all(result[r] is None for r in range(world)), result
    for c in ctxs + cctxs:
        c.close()
