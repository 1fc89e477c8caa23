"""Thin lens with abb_chromatic > 0 across ranks (lentil_tl_chroma_mgpu.h, tl_chroma_across_ranks in pota_amd/csrc/lentil_comm.h).

Every attempt that survives the optical vignetting test draws its colour channel from ONE xor128 stream (src/lentil_filter.cpp:
393-406), so the channels of an item depend on every earlier item of the frame.  With the library's communicator each rank
walks its own items in parallel from the states the whole frame's order gives them.  The ranks' draw logs, mapped to frame-wide
visit ids, must equal a whole-frame context's record for record (visit, attempt, channel bits, pixel), the frames must match
within the suite's 1e-5, and every rank must end at the whole frame's generator state.  Ranks run as threads on the one GPU
(tests/fake_rccl), as in test_native_exchange.
"""
import ctypes as C

import numpy as np
import pytest

import common
import oracle_lib
from pota_amd import _abi, capi, distributed
from test_gpu_parity import _compare_with_whole, gpu_run
from test_native_exchange import _threads, fake_rccl  # noqa: F401  (fixture)
from test_native_exchange_degenerate import _slice

pytestmark = pytest.mark.gpu

W, H, M = 96, 64, 9
KINDS = [0, 0, 1]                 # RGBA, a gaussian and a closest extra AOV
PASSES = 2                        # the second pass continues the stream where the first left it


def _params(ctype=0, chroma=0.6):
    return common.tl_setup(W, H, samples_override=48, abb_chromatic=chroma, abb_chromatic_type=ctype, abb_coma=0.35,
                           optical_vignetting_distance=2.0, optical_vignetting_radius=1.5)


def _columns(p, keep=None):
    """the stream; keep(px, py) -> bool: highlights elsewhere become a copy of an ordinary visit of their pixel"""
    visits, cols = common.make_stream(p, W, H, M, f_hi=0.02, n_extra=2)
    if keep is not None:
        v = np.arange(W * H * M)
        px, py = (v // M) % W, (v // M) // W
        hi = cols["rgba"][:, 0] > 2.0
        for d in np.nonzero(hi & ~keep(px, py))[0]:
            first = d - d % M
            donor = next(u for u in range(first, first + M) if not hi[u])
            for k in ("rgba", "pos_z", "raydir_time"):
                cols[k][d] = cols[k][donor]
    return cols


def _log_of(ctx, to_gid):
    log = ctx.draw_log()
    if to_gid is not None and log.shape[0]:
        log = log.copy()
        log[:, 0] = to_gid(log[:, 0].astype(np.int64)).astype(np.uint32)
    return log


def _whole(p, cols, passes=PASSES, bokeh=None):
    """one context over the whole frame: its logs and generator states after every pass; the context holds the last frame"""
    visits, keep = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    ctx = capi.Context(0)
    logs, states = [], []
    for _ in range(passes):
        gpu_run(ctx, p, None, visits, n_aovs=3, kinds=KINDS, bokeh_tables=bokeh)
        logs.append(common.sort_log(ctx.draw_log()))
        states.append(ctx.get_xor128_state())
    ctx.P = p
    return ctx, logs, states, keep


def _context(p, cols, log=True, bokeh=None, **layout):
    v, kv = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W, **layout)
    ctx = capi.Context(0)
    ctx.set_params(p)
    ctx.set_bokeh(bokeh)
    ctx.alloc_frame(3, KINDS)
    if log:
        ctx.set_draw_log(1 << 22)
    ctx.upload_visits(v)
    return ctx, (cols, v, kv)


def _log_for(log, rank):
    """log: one flag for every rank, or a list of them"""
    return log[rank] if isinstance(log, (list, tuple)) else log


def _band_ranks(p, cols, world, bounds, log=True, bokeh=None):
    ctxs, keep, bands, gid = [], [], [], []
    for rank in range(world):
        b_lo, b_hi = distributed.band_of(rank, world, H, p.yres, bounds)
        ctx, k = _context(p, _slice(cols, slice(b_lo * W * M, min(b_hi, H) * W * M)), _log_for(log, rank), bokeh=bokeh, pixel_y0=b_lo)
        ctxs.append(ctx); keep.append(k); bands.append((b_lo, b_hi))
        gid.append(lambda v, b=b_lo: v + b * W * M)
    return ctxs, keep, bands, gid


def _interleaved_ranks(p, cols, world, log=True):
    ctxs, keep, gid = [], [], []
    rv = W * M
    for rank in range(world):
        rows = np.arange(rank, H, world)
        idx = (rows[:, None] * rv + np.arange(rv)[None, :]).reshape(-1)
        ctx, k = _context(p, _slice(cols, idx), _log_for(log, rank), pixel_y0=rank, pixel_row_stride=world)
        ctxs.append(ctx); keep.append(k)
        gid.append(lambda v, r=rank: ((v // rv) * world + r) * rv + v % rv)
    return ctxs, keep, [None] * world, gid


def _run_native(ctxs, world, step, gid, passes=PASSES, steps=None):
    """every rank's (frame-wide draw log, xor128 state, tl_chroma_stats, degenerate_stats) after every pass (steps: one
    step function per rank instead of `step`)"""
    uid = capi.Context.comm_unique_id()
    out = {}

    def rank_fn(rank):
        ctx = ctxs[rank]
        ctx.comm_init(uid, rank, world)
        out[rank] = []
        for _ in range(passes):
            (steps[rank] if steps else step)(ctx)
            ctx.sync()
            out[rank].append((_log_of(ctx, gid[rank]), ctx.get_xor128_state(), ctx.tl_chroma_stats(), ctx.degenerate_stats()))
        ctx.comm_destroy()

    _threads(rank_fn, world)
    return out


def _check(out, world, whole_logs, whole_states, passes=PASSES):
    for k in range(passes):
        merged = common.sort_log(np.concatenate([out[r][k][0] for r in range(world)]))
        assert merged.shape == whole_logs[k].shape, "pass %d: %d draws against %d" % (k, merged.shape[0], whole_logs[k].shape[0])
        assert np.array_equal(merged, whole_logs[k]), "pass %d: the draw logs differ" % k
        assert set(np.unique(merged[:, 1] >> 30)) == {0, 1, 2}
        for r in range(world):
            assert out[r][k][1] == whole_states[k], "pass %d, rank %d: xor128 state" % (k, r)
        items = [out[r][k][2][0] for r in range(world)]
        deps = [out[r][k][2][1] for r in range(world)]
        assert len(set(items)) == 1 and items[0] > 50           # the frame's items, the same on every rank
        assert len(set(deps)) == 1
    return out[0][0][2]


@pytest.mark.parametrize("world,bounds", [(2, [0, 23, 64]), (3, [0, 5, 40, 64]), (4, [0, 2, 17, 50, 64])],
                         ids=["bands-2", "bands-3", "bands-4"])
def test_bands_match_the_whole_frame(fake_rccl, world, bounds):
    """lentil_hip_exchange_bands with uneven bounds: draws, generator states and every band's rows as one context's."""
    p = _params()
    cols = _columns(p)
    whole, wl, ws, wk = _whole(p, cols)
    ctxs, ck, bands, gid = _band_ranks(p, cols, world, bounds)
    out = _run_native(ctxs, world, lambda ctx: distributed.frame_step_bands_native(ctx, H, bounds), gid)
    _check(out, world, wl, ws)
    for rank in range(world):
        _compare_with_whole(ctxs[rank], whole, KINDS, rows=bands[rank])
        ctxs[rank].close()
    whole.close()


@pytest.mark.parametrize("world", [2, 3])
def test_interleaved_matches_the_whole_frame(fake_rccl, world):
    """lentil_hip_allreduce: every rank holds the whole frame, as one context's."""
    p = _params()
    cols = _columns(p)
    whole, wl, ws, wk = _whole(p, cols)
    ctxs, ck, bands, gid = _interleaved_ranks(p, cols, world)
    out = _run_native(ctxs, world, distributed.frame_step_native, gid)
    _check(out, world, wl, ws)
    for rank in range(world):
        _compare_with_whole(ctxs[rank], whole, KINDS)
        ctxs[rank].close()
    whole.close()


def test_world_one_communicator(fake_rccl):
    """World size 1 with a communicator takes the parallel walk too: the same draws and state as no communicator."""
    p = _params()
    cols = _columns(p)
    whole, wl, ws, wk = _whole(p, cols)
    ctxs, ck, bands, gid = _band_ranks(p, cols, 1, None)
    out = _run_native(ctxs, 1, lambda ctx: distributed.frame_step_bands_native(ctx, H), gid)
    _check(out, 1, wl, ws)
    _compare_with_whole(ctxs[0], whole, KINDS)
    ctxs[0].close()
    whole.close()


@pytest.mark.parametrize("ctype", [0, 1])
@pytest.mark.parametrize("where", ["border", "centred"])
def test_border_and_centred_highlights(fake_rccl, ctype, where):
    """Highlights only at the frame's border with a strong chromatic shift: some items' generator use depends on the
    channels drawn (walked in order by the chain).  Highlights only well inside: none does."""
    p = _params(ctype, chroma=0.8)
    if where == "border":
        keep = lambda px, py: (px < 3) | (px >= W - 3) | (py < 3) | (py >= H - 3)
    else:
        keep = lambda px, py: (px >= 16) & (px < W - 16) & (py >= 12) & (py < H - 12)
    cols = _columns(p, keep)
    whole, wl, ws, wk = _whole(p, cols)
    ctxs, ck, bands, gid = _interleaved_ranks(p, cols, 3)
    out = _run_native(ctxs, 3, distributed.frame_step_native, gid)
    items, dep, _ = _check(out, 3, wl, ws)
    if where == "border":
        assert 0 < dep < items
    else:
        assert dep == 0
    for rank in range(3):
        _compare_with_whole(ctxs[rank], whole, KINDS)
        ctxs[rank].close()
    whole.close()


def test_bands_match_the_oracle(orc, fake_rccl):
    """Three bands against the single-threaded oracle: the merged accepted-draw lists bit-identical (channels included), the
    generator state after the pass identical."""
    p = _params(1, chroma=0.7)
    cols = _columns(p)
    visits, vk = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    ref = oracle_lib.Frame(orc, p, n_aovs=3, kinds=KINDS, keep_log=True)
    ref.run(None, None, visits)
    st = (C.c_uint32 * 4)()
    orc.orc_frame_get_xor128(ref.h, st)
    ctxs, ck, bands, gid = _band_ranks(p, cols, 3, None)
    out = _run_native(ctxs, 3, lambda ctx: distributed.frame_step_bands_native(ctx, H), gid, passes=1)
    merged = common.sort_log(np.concatenate([out[r][0][0] for r in range(3)]))
    assert np.array_equal(merged, common.sort_log(ref.log()))
    for r in range(3):
        assert out[r][0][1] == list(st)
        ctxs[r].close()
    ref.close()


def test_bands_with_an_aperture_image_match_the_oracle(orc, fake_rccl):
    """bokeh_enable_image on two uneven bands, the table one whose clamps bite (tests/bokeh_tables.py: cdfRow ends at 0.75, every
    cdfColumn at 0.5): the per-rank kernels form every attempt's aperture point from the image.  The merged accepted-draw
    lists and the generator state are the single-threaded oracle's, a whole-frame context is the oracle's within 1e-5, and
    every band's rows are that context's."""
    import bokeh_tables
    from test_gpu_parity import check_frame, check_logs
    p = _params(0, chroma=0.5)
    p.bokeh_enable_image = 1
    tables = bokeh_tables.tables("clamp16")
    ob = bokeh_tables.oracle_bokeh(orc, "clamp16")
    cols = _columns(p)
    visits, vk = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=W)
    ref = oracle_lib.Frame(orc, p, n_aovs=3, kinds=KINDS, keep_log=True)
    plain = oracle_lib.Frame(orc, _params(0, chroma=0.5), n_aovs=3, kinds=KINDS, keep_log=True)
    try:
        ref.run(None, ob, visits)
        plain.run(None, None, visits)
        assert ref.counters().accepted_draws > 5000
        assert not np.array_equal(common.sort_log(ref.log()), common.sort_log(plain.log()))       # the image changes the draws
        st = (C.c_uint32 * 4)()
        orc.orc_frame_get_xor128(ref.h, st)
        bounds = [0, 23, 64]
        ctxs, ck, bands, gid = _band_ranks(p, cols, 2, bounds, bokeh=tables)
        out = _run_native(ctxs, 2, lambda ctx: distributed.frame_step_bands_native(ctx, H, bounds), gid, passes=1)
        merged = common.sort_log(np.concatenate([out[r][0][0] for r in range(2)]))
        assert np.array_equal(merged, common.sort_log(ref.log()))
        assert set(np.unique(merged[:, 1] >> 30)) == {0, 1, 2}
        whole, wl, ws, wk = _whole(p, cols, passes=1, bokeh=tables)
        check_logs(whole, ref)
        check_frame(whole, ref, n_aovs=3, kinds=KINDS)
        assert ws[0] == list(st)
        for r in range(2):
            assert out[r][0][1] == list(st)
            _compare_with_whole(ctxs[r], whole, KINDS, rows=bands[r])
            ctxs[r].close()
        whole.close()
    finally:
        ref.close()
        plain.close()
        orc.orc_bokeh_destroy(ob)


@pytest.mark.parametrize("partition", ["bands", "interleaved"])
def test_rank_local_rerun(fake_rccl, partition):
    """A closest-AOV candidate at depth 0: rank 1 has no draw log and runs its pass again on its own, inside the exchange,
    while rank 0 (which has one) waits there.  That run walks the rank's items from the entry states the first run kept and
    starts no collective: nothing hangs, and the frame, the draws and the generator state are still the whole frame's."""
    p = _params()
    cols = _columns(p)
    whole, wl, ws, wk = _whole(p, cols, passes=1)
    v0 = int(wl[0][0, 0])                        # a redistributed visit: its draws and its own pixel see depth 0
    whole.close()
    cols["pos_z"][v0, 3] = np.float32(0.0)
    whole, wl, ws, wk = _whole(p, cols, passes=1)
    if partition == "bands":
        ctxs, ck, bands, gid = _band_ranks(p, cols, 2, [0, 30, 64], log=[True, False])
        step = lambda ctx: distributed.frame_step_bands_native(ctx, H, [0, 30, 64])
    else:
        ctxs, ck, bands, gid = _interleaved_ranks(p, cols, 2, log=[True, False])
        step = distributed.frame_step_native
    out = _run_native(ctxs, 2, step, gid, passes=1)
    _check(out, 2, wl, ws, passes=1)
    assert any(out[r][0][3][0] for r in range(2))                     # a rank met the candidate at depth 0 ...
    assert [out[r][0][3][4] for r in range(2)] == [0, 1]              # ... rank 1 alone ran its pass again
    for rank in range(2):
        _compare_with_whole(ctxs[rank], whole, KINDS, rows=bands[rank])
        ctxs[rank].close()
    whole.close()


def test_rank_without_items(fake_rccl):
    """Highlights only well inside the frame, and a top band with none: that rank has visits but no item -- no count or walk
    kernel, an empty list -- and still takes part in the pass's exchange and ends at the whole frame's state."""
    p = _params(0, chroma=0.8)
    cols = _columns(p, lambda px, py: (px >= 16) & (px < W - 16) & (py >= 12) & (py < H - 12))
    whole, wl, ws, wk = _whole(p, cols)
    bounds = [0, 6, 40, 64]
    ctxs, ck, bands, gid = _band_ranks(p, cols, 3, bounds)
    out = _run_native(ctxs, 3, lambda ctx: distributed.frame_step_bands_native(ctx, H, bounds), gid)
    _check(out, 3, wl, ws)
    assert ctxs[0].counters().redistributed_visits == 0 and out[0][-1][0].shape[0] == 0
    for rank in range(3):
        _compare_with_whole(ctxs[rank], whole, KINDS, rows=bands[rank])
        ctxs[rank].close()
    whole.close()


def _ragged(cols, lo, hi):
    """visits [lo, hi) of the stream as a ragged one: each visit's pixel in its own column"""
    out = _slice(cols, slice(lo, hi))
    pix = np.arange(lo, hi) // M
    out["pixel"] = ((pix % W) | ((pix // W) << 16)).astype(np.uint32)
    return out


def _ragged_ranks(p, cols, cuts, bases):
    ctxs, keep = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v, kv = capi.make_visits(_ragged(cols, lo, hi))
        ctx = capi.Context(0)
        ctx.set_params(p)
        ctx.set_bokeh(None)
        ctx.alloc_frame(3, KINDS)
        ctx.set_draw_log(1 << 22)
        ctx.upload_visits(v)
        ctxs.append(ctx); keep.append(kv)
    # (interleaved-style: every rank's whole frame summed; the visit ids of a ragged stream start at visit_id_base)
    steps = [lambda ctx, b=b: (ctx.set_closest_exchange(True, b), ctx.clear_frame(), ctx.redistribute(), ctx.allreduce(),
                               ctx.resolve()) for b in bases]
    return ctxs, keep, steps


def test_ragged_stream_with_visit_id_base(fake_rccl):
    """A ragged stream cut into three contiguous ranges, each rank numbering its visits from its range's start: the same draws,
    frame and generator states as one context over the whole ragged stream."""
    p = _params()
    cols = _columns(p)
    n = W * H * M
    v, kv = capi.make_visits(_ragged(cols, 0, n))
    whole = capi.Context(0)
    wl, ws = [], []
    for _ in range(PASSES):
        gpu_run(whole, p, None, v, n_aovs=3, kinds=KINDS)
        wl.append(common.sort_log(whole.draw_log()))
        ws.append(whole.get_xor128_state())
    whole.P = p
    cuts = [0, 9000, 20000, n]
    ctxs, keep, steps = _ragged_ranks(p, cols, cuts, cuts[:-1])
    out = _run_native(ctxs, 3, None, [lambda u, b=b: u + b for b in cuts[:-1]], steps=steps)
    _check(out, 3, wl, ws)
    for rank in range(3):
        _compare_with_whole(ctxs[rank], whole, KINDS)
        ctxs[rank].close()
    whole.close()


def test_ragged_stream_with_one_id_range_is_refused(fake_rccl):
    """The same ranges all numbered from 0: items of two ranks share visit ids, which gives no order.  Every rank refuses the
    pass alike (none waits in a collective the others left), instead of ranks ordering the ties differently."""
    p = _params()
    cols = _columns(p)
    n = W * H * M
    cuts = [0, n // 2, n]
    ctxs, keep, steps = _ragged_ranks(p, cols, cuts, [0, 0])
    uid = capi.Context.comm_unique_id()
    errors = {}

    def rank_fn(rank):
        ctxs[rank].comm_init(uid, rank, 2)
        try:
            steps[rank](ctxs[rank])
            errors[rank] = None
        except capi.LentilError as e:
            errors[rank] = e
        ctxs[rank].comm_destroy()

    _threads(rank_fn, 2)
    for rank in range(2):
        assert isinstance(errors[rank], capi.LentilError), "rank %d: %r" % (rank, errors[rank])
        assert errors[rank].code == _abi.ERR_INVALID
        ctxs[rank].close()


def _xor128_steps(s, k):
    x, y, z, w = s
    for _ in range(k):
        t = (x ^ (x << 11)) & 0xFFFFFFFF
        x, y, z = y, z, w
        w = (w ^ (w >> 19) ^ t ^ (t >> 8)) & 0xFFFFFFFF
    return [x, y, z, w]


def _gf2_jump(s, k):
    """the generator's step matrix over GF(2)^128 (columns: the step applied to unit vectors) to the power k, applied to s"""
    T = np.zeros((128, 128), np.int64)
    for i in range(128):
        e = [0, 0, 0, 0]
        e[i // 32] = 1 << (i % 32)
        o = _xor128_steps(e, 1)
        for r in range(128):
            T[r, i] = (o[r // 32] >> (r % 32)) & 1
    v = np.array([(s[i // 32] >> (i % 32)) & 1 for i in range(128)], np.int64)
    while k:
        if k & 1:
            v = (T @ v) & 1
        T = (T @ T) & 1
        k >>= 1
    return [int(sum(int(v[32 * wd + b]) << b for b in range(32))) for wd in range(4)]


def test_xor128_jump():
    """lentil_hip_test_xor128_jump: k outputs ahead equals k single steps, and a GF(2) matrix power far out."""
    ctx = capi.Context(0)
    for s in ([123456789, 362436069, 521288629, 88675123], [0x12345678, 0x9ABCDEF0, 0x0F1E2D3C, 0x4B5A6978]):
        for k in (0, 1, 2, 63, 64, 1000, (1 << 20) + 7):
            assert ctx.test_xor128_jump(s, k) == _xor128_steps(s, k), k
        k = (1 << 40) + 5
        assert ctx.test_xor128_jump(s, k) == _gf2_jump(s, k)
    ctx.close()
