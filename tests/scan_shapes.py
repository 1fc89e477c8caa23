"""The shapes the scan kernels are tested at (tests/test_scan_shape_cases.py: the table against the oracle, no GPU;
tests/test_gpu_scan_shapes.py: the kernels against the oracle).  A plain module: no fixtures, fixed seeds, nothing random.

A pass starts in one of seven scan kernels (include/lentil_hip.h, LENTIL_SCAN_*; plan_scan in csrc/lentil_scan.h).  Which
one follows from the stream's shape, and each case below names the kernel its shape selects -- `expect` -- and, for the
uniform streams, the pixels per tile or group -- `ppt` (lentil_hip_debug_last_scan reports both).  Where the figures come from
(LDS sizes as plan_scan computes them, wave queues of 4608 B included; a context streams by default, so the two resident solve
blocks' LDS always counts: 2 x 29184 B for a lens with a compiled-in kernel, 2 x 53760 B for the table interpreter and for a
thin lens):
  beauty only, whole pixels   scan_dma_kernel's block is M * 4096 + 30208 B against 80 KiB: M <= 12, else scan_uniform_kernel
                              with tiles of 64 pixels halved until ppt * M * 80 B <= 48 KiB;
                              scan_dma2_kernel's is M * 8192 + 30208 B against 160 KiB less the solve blocks: M in 2 ... 9
                              beside a compiled lens, 2 ... 3 beside the table interpreter or a thin lens, rows of >= 2 pixels
  extras, all gaussian        scan_dma_multi_kernel, M <= 64 (its block, (4 + K) * 8320 + 4608 B, fits for every K <= 15):
                              groups of 64 / M pixels, or of 64 / q where the q = stride / 4 float4 of a pixel record make
                              ppt * q > 64 and 4 * (64 / q) >= 3 * ppt;  M > 64: one column at a time, scan_uniform_kernel
                              (24 KiB of staging)
  a closest-filtered extra, or a last pixel short of visits:  scan_uniform_multi_kernel, groups of 64 / M pixels
  visits_per_pixel == 0       scan_runs_kernel; LENTIL_SCAN_RUNS=0: scan_ragged_kernel

Every stream carries PLANTED highlights: one generated highlight visit (all its columns: a sample behind the middle of the
frame, far out of focus) copied onto the first and the last visit of the stream, the last visit of the first row, the first
visit of the last tile or group, one visit of a pixel whose other visits stay direct and all visits of another pixel -- the
edges a scan kernel can drop.  Their draws land around the middle of the frame; everywhere else a pixel holds the fp32 sum of
its own visits in their order, and the GPU's must be the oracle's bit for bit.
"""
import numpy as np

import common
from pota_amd import capi, workload

SAMPLES = 8            # samples_override: the oracle's solves stay cheap
F_HI = 0.002           # the generator's own highlights, beside the planted ones
SEED = 0x5CA9

DMA2, DMA, DMA_MULTI, UNIFORM, UNIFORM_MULTI, RUNS, RAGGED = (capi.SCAN_DMA2, capi.SCAN_DMA, capi.SCAN_DMA_MULTI, capi.SCAN_UNIFORM,
                                                              capi.SCAN_UNIFORM_MULTI, capi.SCAN_RUNS, capi.SCAN_RAGGED)

# every entry of the list the table is there to cover; each case is the only one to name at least one of them
REQUIRED = (
    ["beauty:M=%d" % m for m in (1, 2, 3, 4, 9, 12, 16, 25, 36, 49, 64, 100, 144)] +
    ["beauty:ppr=1", "beauty:ppr=2"] +
    ["beauty:%s" % s for s in ("64x3", "65x3", "63x1", "37x7", "127x5", "129x17", "331x173")] +
    ["camera:thinlens", "camera:petzval"] +
    ["tables:exact", "tables:tail", "tables:dma2"] +
    ["multi:M=%d,K=%d:%s" % (m, k, t) for (m, k) in ((1, 1), (2, 2), (7, 2), (9, 2), (9, 8), (9, 14), (16, 3), (16, 15), (21, 2), (32, 1))
     for t in ("exact", "tail")] +
    ["multi:M=33,K=2", "multi:M=64,K=1", "multi:M=1,K=15", "multi:M=100,K=2"] +
    ["multi:ppt=%d" % n for n in (64, 32, 9, 7, 4, 3, 2, 1)] +
    ["multi:one-store-pass", "multi:two-store-passes", "multi:reduced-ppt", "multi:K=14", "multi:K=15"] +
    ["closest:M=%d" % m for m in (1, 7, 9, 16, 33, 64)] +
    ["truncated:%s:K=%d" % (t, k) for t in ("n-1", "n-M+1", "tile+1") for k in (0, 2)] +
    ["ragged:n=%d:%s" % (n, r) for n in (1, 63, 65, 257, 4097) for r in ("runs", "atomics")] +
    ["region:x0>0", "region:y0>0", "region:ppr<W", "region:row_stride=2", "region:bucket0", "region:bucket1", "region:bucket2",
     "region:bucket3", "region:K=2:a", "region:K=2:b"]
)

CASES = []


def _case(name, W, H, M, expect, ppt=None, K=0, kinds=None, camera="po", lens="double_gauss_50mm", v_end=None, region=None,
          lens_mode=0, runs_env=None, run_lengths=None, group=None, covers=()):
    """W x H: the frame.  region (x0, y0, pixels_per_row, rows, row_stride): the pixels the stream covers, the whole frame if
    None.  v_end: the stream is cut off behind that many visits.  M == 0: a ragged stream of v_end visits in runs of
    run_lengths (cycled) visits per pixel, the pixels in iterator order from the frame's first.  runs_env: what
    LENTIL_SCAN_RUNS is set to for the passes (None: unset).  group: cases whose bit-exact sets are looked at together."""
    CASES.append(dict(name=name, W=W, H=H, M=M, K=K, kinds=kinds or [0] * (K + 1), camera=camera, lens=lens, v_end=v_end,
                      region=region or (0, 0, W, H, 1), lens_mode=lens_mode, runs_env=runs_env, run_lengths=run_lengths,
                      expect_kernel=expect, ppt=ppt, group=group or name, covers=tuple(covers)))


# ---- beauty only, gaussian, whole pixels ---------------------------------------------------------------------------------
for _m, _k, _p in ((2, DMA2, 64), (3, DMA2, 64), (4, DMA2, 64), (9, DMA2, 64), (12, DMA, 64), (16, UNIFORM, 32), (25, UNIFORM, 16),
                   (36, UNIFORM, 16), (49, UNIFORM, 8), (64, UNIFORM, 8)):
    _case("beauty_m%d" % _m, 48, 40, _m, _k, _p, covers=["beauty:M=%d" % _m])
# (the two large ones: the LDS-DMA kernels have no room for them, the register-staged scan takes tiles of four pixels)
_case("beauty_m100", 24, 20, 100, UNIFORM, 4, covers=["beauty:M=100"])
_case("beauty_m144", 24, 20, 144, UNIFORM, 4, covers=["beauty:M=144"])
_case("beauty_m1", 48, 40, 1, DMA, 64, covers=["beauty:M=1"])
# (a frame one or two pixels wide is no frame a camera is set up for: a column of one / two pixels of a 16-pixel-wide frame)
_case("beauty_ppr1", 16, 40, 9, DMA, 64, region=(5, 0, 1, 40, 1), covers=["beauty:ppr=1"])
_case("beauty_ppr2", 16, 40, 9, DMA2, 64, region=(7, 0, 2, 40, 1), covers=["beauty:ppr=2"])
# pixel and tile counts.  (The streams of one, three and five rows are the first rows of a 16-row frame: the stream has the
# shape the entry names, the frame keeps room around the middle for the planted highlights' draws.)
_case("beauty_64x3", 64, 16, 9, DMA2, 64, region=(0, 0, 64, 3, 1), covers=["beauty:64x3"])          # 3 full tiles
_case("beauty_65x3", 65, 16, 9, DMA2, 64, region=(0, 0, 65, 3, 1), covers=["beauty:65x3"])          # 3 tiles + 3 pixels
_case("beauty_63x1", 63, 16, 9, DMA2, 64, region=(0, 0, 63, 1, 1), covers=["beauty:63x1"])          # a tail and no full tile
_case("beauty_37x7", 37, 16, 9, DMA2, 64, region=(0, 0, 37, 7, 1), covers=["beauty:37x7"])          # 259 pixels
_case("beauty_127x5", 127, 16, 9, DMA2, 64, region=(0, 0, 127, 5, 1), covers=["beauty:127x5"])      # 9 tiles + 59 pixels
_case("beauty_129x17", 129, 17, 9, DMA2, 64, covers=["beauty:129x17"])                              # 34 tiles + 17 pixels
_case("beauty_331x173", 331, 173, 9, DMA2, 64, covers=["beauty:331x173"])                           # 894 tiles + 47 pixels
_case("beauty_thinlens", 45, 31, 3, DMA2, 64, camera="thinlens", covers=["camera:thinlens"])
_case("beauty_petzval", 50, 30, 9, DMA2, 64, lens="petzval_58mm", covers=["camera:petzval"])

# ---- the table interpreter (lens_mode = 1), second pass streamed: its solve blocks leave scan_dma2_kernel room for M <= 3 ----
_case("tables_exact", 64, 48, 9, DMA, 64, lens_mode=1, covers=["tables:exact"])
_case("tables_tail", 65, 31, 9, DMA, 64, lens_mode=1, covers=["tables:tail"])
_case("tables_m3_tail", 65, 31, 3, DMA2, 64, lens_mode=1, covers=["tables:dma2"])

# ---- extra gaussian AOVs: scan_dma_multi_kernel ---------------------------------------------------------------------------
# (M, K, pixels per group, frame with a whole number of groups, what of the list the pair is there for)
for _m, _kk, _p, _wh, _cov in ((1, 1, 64, (32, 16), ["multi:ppt=64"]), (2, 2, 32, (32, 16), ["multi:ppt=32"]),
                               (7, 2, 9, (27, 20), ["multi:ppt=9", "multi:one-store-pass"]), (9, 2, 7, (28, 20), ["multi:ppt=7"]),
                               (9, 8, 6, (30, 20), ["multi:reduced-ppt"]), (9, 14, 7, (28, 20), ["multi:two-store-passes", "multi:K=14"]),
                               (16, 3, 4, (32, 16), ["multi:ppt=4"]), (16, 15, 3, (30, 20), ["multi:K=15"]),
                               (21, 2, 3, (30, 20), ["multi:ppt=3"]), (32, 1, 2, (32, 16), ["multi:ppt=2"])):
    _case("multi_m%d_k%d_exact" % (_m, _kk), _wh[0], _wh[1], _m, DMA_MULTI, _p, K=_kk, group="multi",
          covers=["multi:M=%d,K=%d:exact" % (_m, _kk)] + _cov)
    # 31 x 17 = 527 pixels: a remainder for every group size from 2 to 64
    _case("multi_m%d_k%d_tail" % (_m, _kk), 31, 17, _m, DMA_MULTI, _p, K=_kk, group="multi", covers=["multi:M=%d,K=%d:tail" % (_m, _kk)])
_case("multi_m33_k2", 31, 17, 33, DMA_MULTI, 1, K=2, group="multi", covers=["multi:M=33,K=2", "multi:ppt=1"])
_case("multi_m64_k1", 31, 17, 64, DMA_MULTI, 1, K=1, group="multi", covers=["multi:M=64,K=1"])
_case("multi_m1_k15", 31, 17, 1, DMA_MULTI, 64, K=15, group="multi", covers=["multi:M=1,K=15"])
_case("multi_m100_k2", 20, 12, 100, UNIFORM, 2, K=2, group="multi", covers=["multi:M=100,K=2"])

# ---- a closest-filtered AOV among the extras: scan_uniform_multi_kernel, tailed pixel counts ------------------------------
for _m in (1, 7, 9, 16, 33, 64):
    _case("closest_m%d" % _m, 31, 17, _m, UNIFORM_MULTI, 64 // _m, K=2, kinds=[0, 1, 0], group="closest", covers=["closest:M=%d" % _m])

# ---- truncated streams: the last pixel holds fewer than M visits ----------------------------------------------------------
for _kk, _k, _p, _grp in ((0, UNIFORM, 64, 64), (2, UNIFORM_MULTI, 7, 7)):
    _n = 40 * 20 * 9
    for _tag, _ve in (("n-1", _n - 1), ("n-M+1", _n - 9 + 1), ("tile+1", 5 * _grp * 9 + 1)):
        _case("truncated_%s_k%d" % (_tag.replace("+", "p"), _kk), 40, 20, 9, _k, _p, K=_kk, v_end=_ve, group="truncated_k%d" % _kk,
              covers=["truncated:%s:K=%d" % (_tag, _kk)])

# ---- ragged streams (visits_per_pixel = 0) --------------------------------------------------------------------------------
# scan_runs_kernel sums a run in its order.  scan_ragged_kernel adds every visit with an atomic of its own, in any order: its
# streams bring at most two visits per pixel, whose fp32 sum is the same in either order (addition commutes), so that the
# bit-for-bit bar holds for it as well.
for _n in (1, 63, 65, 257, 4097):
    _case("ragged_n%d_runs" % _n, 64, 48, 0, RUNS, 0, v_end=_n, run_lengths=(3, 1, 2, 5), covers=["ragged:n=%d:runs" % _n])
    _case("ragged_n%d_atomics" % _n, 64, 48, 0, RAGGED, 0, v_end=_n, run_lengths=(2, 1), runs_env="0", covers=["ragged:n=%d:atomics" % _n])

# ---- sub-rectangles of a larger frame -------------------------------------------------------------------------------------
# four unequal buckets of one 64 x 48 frame (tests/test_gpu_scan_shapes.py also renders them one after the other)
BUCKETS = ("bucket0", "bucket1", "bucket2", "bucket3")
_case("bucket0", 64, 48, 9, DMA2, 64, region=(0, 0, 37, 23, 1), covers=["region:bucket0", "region:ppr<W"])
_case("bucket1", 64, 48, 9, DMA2, 64, region=(37, 0, 27, 23, 1), covers=["region:bucket1", "region:x0>0"])
_case("bucket2", 64, 48, 9, DMA2, 64, region=(0, 23, 37, 25, 1), covers=["region:bucket2", "region:y0>0"])
_case("bucket3", 64, 48, 9, DMA2, 64, region=(37, 23, 27, 25, 1), covers=["region:bucket3"])
_case("rowstride2", 32, 24, 9, DMA2, 64, region=(3, 1, 20, 10, 2), covers=["region:row_stride=2"])
# a region that changes between passes, with extras (beauty only: bucket0 then bucket3)
STALE = {0: ("bucket0", "bucket3"), 2: ("subrect_k2_a", "subrect_k2_b")}
_case("subrect_k2_a", 64, 48, 9, DMA_MULTI, 7, K=2, region=(2, 3, 41, 17, 1), group="subrect_k2", covers=["region:K=2:a"])
_case("subrect_k2_b", 64, 48, 9, DMA_MULTI, 7, K=2, region=(30, 20, 29, 26, 1), group="subrect_k2", covers=["region:K=2:b"])

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def group_pixels(case):
    """pixels per tile or group of the case's scan kernel (what a "last tile" of the stream is)"""
    return case["ppt"] or 64


def setup(case):
    """(params, lens table or None, keepalive)"""
    if case["camera"] == "thinlens":
        return common.tl_setup(case["W"], case["H"], samples_override=SAMPLES), None, None
    p, model, table, keep = common.po_setup(case["W"], case["H"], lens=case["lens"], samples_override=SAMPLES)
    return p, table, (model, keep)


def _generate(p, case, v_begin, v_end, f_hi):
    return workload.generate(np, v_begin, v_end, case["W"], case["H"], max(case["M"], 1), seed=SEED, f_hi=f_hi,
                             focus_dist=float(p.focus_distance) / (10.0 if p.cameraType == 1 else 1.0),
                             tan_half_fov=common.tan_half_fov(p), n_extra=case["K"])


def _columns(cols):
    return [cols[k] for k in ("rgba", "pos_z", "raydir_time", "volume_ignore", "transmission")] + list(cols["extra"])


def is_generated_highlight(cols):
    return cols["rgba"][:, 0] == np.float32(workload.HIGHLIGHT_RADIANCE)


def build(case):
    """(params, lens table, lentil_visits, columns).  columns["planted"]: the visit ids the highlight was copied onto;
    columns["keep"] keeps what the structures point to alive."""
    W, H, M = case["W"], case["H"], case["M"]
    x0, y0, ppr, rows, rs = case["region"]
    assert 0 <= x0 and x0 + ppr <= W and 0 <= y0 and y0 + (rows - 1) * rs < H, "the region leaves the frame"
    p, table, keep = setup(case)
    if M:
        # the whole frame's stream, then the visits of the region's pixels
        full = _generate(p, case, 0, W * H * M, F_HI)
        pix = ((y0 + np.arange(rows) * rs)[:, None] * W + (x0 + np.arange(ppr))[None, :]).ravel()
        vis = (pix[:, None] * M + np.arange(M)[None, :]).ravel()
        if case["v_end"] is not None:
            vis = vis[:case["v_end"]]
        cols = {k: np.ascontiguousarray(full[k][vis]) for k in ("rgba", "pos_z", "raydir_time", "volume_ignore", "transmission")}
        cols["extra"] = [np.ascontiguousarray(e[vis]) for e in full["extra"]]
    else:
        n = case["v_end"]
        cols = _generate(p, case, 0, n, F_HI)
        lengths = case["run_lengths"]
        owner, k = [], 0
        while len(owner) < n:
            owner += [k] * lengths[k % len(lengths)]
            k += 1
        owner = np.asarray(owner[:n], np.int64)
        assert owner[-1] < W * H
        cols["pixel"] = ((owner % W) | ((owner // W) << 16)).astype(np.uint32)
    n = int(cols["rgba"].shape[0])
    # the highlight: the generator's, at the first visit of the frame's middle pixel
    v_src = ((H // 2) * W + W // 2) * max(M, 1)
    src = _generate(p, case, v_src, v_src + 1, 1.0)
    assert bool(is_generated_highlight(src)[0])
    generated = is_generated_highlight(cols)
    planted = set([0, n - 1])
    if M:
        n_pixels = (n + M - 1) // M
        planted.add(min(ppr * M, n) - 1)                                       # the last visit of the first row
        planted.add(((n_pixels - 1) // group_pixels(case)) * group_pixels(case) * M)      # the first visit of the last tile or group
        busy = set(v // M for v in planted)

        def free_pixel(start, whole):
            """the first pixel from `start` on that holds all its visits, nothing planted and (whole: no matter) no highlight"""
            for q in list(range(start, n // M)) + list(range(0, start)):
                if q not in busy and (whole or not generated[q * M:(q + 1) * M].any()):
                    busy.add(q)
                    return q
            return None

        if M >= 2:
            q = free_pixel(n_pixels // 3, False)                                # one highlight among direct visits
            if q is not None:
                planted.add(q * M + M // 2)
        q = free_pixel((2 * n_pixels) // 3, True)                               # nothing but highlights
        if q is not None:
            planted.update(range(q * M, (q + 1) * M))
    else:
        # ragged: a run with one highlight among direct visits and a run of nothing but highlights, where the stream has them
        starts = np.flatnonzero(np.r_[True, cols["pixel"][1:] != cols["pixel"][:-1]])
        ends = np.r_[starts[1:], n]
        runs = [(int(s), int(e)) for s, e in zip(starts, ends) if 0 not in range(s, e) and n - 1 not in range(s, e)]
        longer = [r for r in runs if r[1] - r[0] >= 2 and not generated[r[0]:r[1]].any()]
        if longer:
            one = longer[len(longer) // 3]
            planted.add(one[0] + (one[1] - one[0]) // 2)
            rest = [r for r in longer if r != one]
            if rest:
                planted.update(range(*rest[(2 * len(rest)) // 3]))
    planted = np.asarray(sorted(planted), np.int64)
    for dst, s in zip(_columns(cols), _columns(src)):
        dst[planted] = s[0]
    if M:
        visits, _ = capi.make_visits(cols, visits_per_pixel=M, pixels_per_row=ppr, pixel_x0=x0, pixel_y0=y0, pixel_row_stride=rs)
    else:
        visits, _ = capi.make_visits(cols, visits_per_pixel=0)
    cols["planted"] = planted
    cols["keep"] = keep
    return p, table, visits, cols


def frame_shape(case):
    """(xres, yres) of the frame's buffers: a W x H render accumulates into W + 1 by H + 1 pixels (camera.setup_filter)"""
    return case["W"] + 1, case["H"] + 1


def stream_pixels(case, cols):
    """frame pixel index of every visit of the case's stream"""
    n = int(cols["rgba"].shape[0])
    W = frame_shape(case)[0]
    if not case["M"]:
        return (cols["pixel"] & 0xFFFF).astype(np.int64) + (cols["pixel"] >> 16).astype(np.int64) * W
    x0, y0, ppr, rows, rs = case["region"]
    q = np.arange(n, dtype=np.int64) // case["M"]
    return (y0 + (q // ppr) * rs) * W + x0 + q % ppr


def oracle(lib, case, built):
    p, table, visits, cols = built
    return common.run_oracle(lib, p, table, visits, n_aovs=case["K"] + 1, kinds=case["kinds"])
