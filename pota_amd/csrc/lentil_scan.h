// lentil_scan.h -- host side of a pass's scan: which of the seven scan kernels takes the bound visit stream, with which tile
// size and how much LDS (plan_scan), the grid of one launch (scan_grid) and the launch itself (launch_scan); the depth bands
// scan_dma2_kernel decides by (scan_bands) and the two debug hooks that need no GPU.  Included by lentil_hip.hip; no kernels
// here, and not among the sources the run-time lens compiler sees.
#pragma once

// Where get_coc_thinlens(P, cz) < 0.4f (lentil_device.h; src/lentil.h:674-692, src/lentil_filter.cpp:185-190) is decided by cz
// alone, for scan_dma2_kernel.  The kernel computes, in fp32, ifd = (-f * -fd) / (-f + -fd), isp = (-f * z) / (-f + z),
// coc = |A (isp - ifd) / isp|.  In exact arithmetic 1 / isp = 1 / z - 1 / f, so coc = |A| |c0 - c1 / z| with c0 = 1 + ifd / f,
// c1 = ifd: in u = 1 / z the set {coc < t} is ONE interval around the focus plane.  The fp32 evaluation differs from that by
// a few 1e-7 relative, times |A| / 0.4 near the threshold (the subtraction isp - ifd carries isp's rounding): with
// eps = 1e-3 + 1e-5 |A| the comparison with 0.4 (1 - eps) / 0.4 (1 + eps) is certain, and the strip in between -- a
// few visits in 10^4 -- is left to the function.  Interval ends are rounded towards the uncertain side; |z| > 1e30 (where
// -f * z overflows and the function returns NaN) is never "certainly below".
static ScanBands scan_bands(const lentil_params &P) {
  ScanBands B;
  for (int i = 0; i < 2; ++i) { B.in_lo[i] = 1.0f; B.in_hi[i] = -1.0f; B.out_lo[i] = 1.0f; B.out_hi[i] = -1.0f; }
  B.out_lo[0] = -INFINITY; B.out_hi[0] = INFINITY;       // nothing usable: every finite depth asks the function
  float fd = (float)P.focus_distance, A = (float)P.aperture_radius;
  if (P.cameraType == LENTIL_POLYNOMIAL_OPTICS) fd = (float)((double)fd / 10.0);
  else A = (float)((double)A * 10.0);
  const float f = P.focal_length;
  const float ifd = (-f * -fd) / (-f + -fd);
  const double a = std::fabs((double)A), c0 = 1.0 + (double)ifd / (double)f, c1 = (double)ifd;
  if (!(a > 0.0) || !std::isfinite(a) || !std::isfinite(c0) || !std::isfinite(c1) || c1 == 0.0 || !(f > 0.0f)) return B;
  const double eps = 1e-3 + 1e-5 * a;
  if (!(eps < 0.25)) return B;
  auto up = [](double v) { float r = (float)v; if ((double)r < v) r = std::nextafter(r, INFINITY); return r; };       // smallest float >= v
  auto down = [](double v) { float r = (float)v; if ((double)r > v) r = std::nextafter(r, -INFINITY); return r; };    // largest float <= v
  // z-intervals of {coc <= t}: u in [ua, ub], z = 1 / u
  auto pieces = [&](double t, bool inner, float lo[2], float hi[2]) {
    double ua = (c0 - t / a) / c1, ub = (c0 + t / a) / c1;
    if (ua > ub) std::swap(ua, ub);
    lo[0] = lo[1] = 1.0f; hi[0] = hi[1] = -1.0f;
    const double big = inner ? 1e30 : (double)INFINITY;
    if (ua > 0.0 || ub < 0.0) {
      const double zl = 1.0 / ub, zh = 1.0 / ua;
      lo[0] = inner ? up(std::max(zl, -big)) : down(zl);
      hi[0] = inner ? down(std::min(zh, big)) : up(zh);
    } else {
      // the interval holds u = 0: everything beyond 1 / ua on the negative side, beyond 1 / ub on the positive side
      if (ua < 0.0) { lo[0] = inner ? (float)-big : -INFINITY; hi[0] = inner ? down(1.0 / ua) : up(1.0 / ua); }
      if (ub > 0.0) { lo[1] = inner ? up(1.0 / ub) : down(1.0 / ub); hi[1] = inner ? (float)big : INFINITY; }
      if (!inner && (ua == 0.0 || ub == 0.0)) { lo[0] = -INFINITY; hi[0] = INFINITY; }
    }
  };
  ScanBands R = B;
  pieces(0.4 * (1.0 - eps), true, R.in_lo, R.in_hi);
  pieces(0.4 * (1.0 + eps), false, R.out_lo, R.out_hi);
  for (int i = 0; i < 2; ++i)
    if (std::isnan(R.in_lo[i]) || std::isnan(R.in_hi[i]) || std::isnan(R.out_lo[i]) || std::isnan(R.out_hi[i])) return B;
  return R;
}

// test hook (no GPU needed): the intervals scan_dma2_kernel would use for these parameters -- in_lo[2], in_hi[2], out_lo[2], out_hi[2]
LENTIL_API int lentil_hip_debug_scan_bands(const lentil_params *P, float out[8]) {
  if (!P || !out) return LENTIL_ERR_INVALID;
  const ScanBands B = scan_bands(*P);
  for (int i = 0; i < 2; ++i) { out[i] = B.in_lo[i]; out[2 + i] = B.in_hi[i]; out[4 + i] = B.out_lo[i]; out[6 + i] = B.out_hi[i]; }
  return LENTIL_OK;
}

// test hook (no GPU needed): scan_dma2_kernel's lean ring slots, the open groups that make a tile busy, the quiet tiles before
// a wave returns to the lean body (kLeanRing, kBusyGroups, kQuietTiles)
LENTIL_API int lentil_hip_debug_scan_lean_counts(uint32_t out[3]) {
  if (!out) return LENTIL_ERR_INVALID;
  out[0] = kLeanRing; out[1] = kBusyGroups; out[2] = kQuietTiles;
  return LENTIL_OK;
}

// How the bound visit stream is scanned: kernel, tile size, LDS.
struct ScanPlan {
  ScanArgs sa{};
  size_t lds = 0;
  uint64_t n_tiles = 0;
  uint32_t kind = LENTIL_SCAN_RAGGED;   // LENTIL_SCAN_*, set once by plan_scan (RAGGED: or RUNS, which launch_scan settles -- LENTIL_SCAN_RUNS is read per launch)
  uint32_t M = 0;
};
// the grid of one scan launch: its blocks, and how many CUs a streamed pass's scan leaves alone (scan_cus_pct: those take a
// third resident solve block)
struct ScanGrid { uint64_t blocks = 0; unsigned skipped = 0; };

// slots per wave (LENTIL_DMA_MULTI_RING: 2 or 3; no difference measured, the waves are not short of bytes in flight)
static uint32_t dma_multi_ring(const lentil_hip_ctx *) {
  static const int forced = getenv("LENTIL_DMA_MULTI_RING") ? atoi(getenv("LENTIL_DMA_MULTI_RING")) : 0;
  return forced == 3 ? 3u : 2u;
}
static size_t dma_multi_lds(const lentil_hip_ctx *ctx) {
  return (size_t)4 * dma_multi_wave_f4(ctx->V.n_extra, dma_multi_ring(ctx)) * 16 + 4 * kWaveQueueLds * sizeof(uint2);
}
// blocks per CU (LENTIL_DMA_MULTI_BLOCKS): two where the CU's LDS holds them and two solve blocks beside them
static uint32_t dma_multi_blocks_per_cu(const lentil_hip_ctx *ctx) {
  static const int forced = getenv("LENTIL_DMA_MULTI_BLOCKS") ? atoi(getenv("LENTIL_DMA_MULTI_BLOCKS")) : 0;
  if (forced >= 1 && forced <= 4) return (uint32_t)forced;
  return 2u * dma_multi_lds(ctx) + 2u * 10u * 1024u <= 160u * 1024u ? 2u : 1u;
}

// scan_dma_multi_kernel takes the stream: whole pixels of M <= 64 visits, uniform weights, gaussian AOVs only
static bool dma_multi_applies(const lentil_hip_ctx *ctx) {
  static const bool allowed = !(getenv("LENTIL_SCAN_DMA_MULTI") && getenv("LENTIL_SCAN_DMA_MULTI")[0] == '0');
  const uint32_t M = ctx->V.visits_per_pixel;
  return allowed && ctx->scan_dma && M > 0 && M <= 64 && ctx->V.n_extra > 0 && !ctx->V.inv_density && !ctx->F.zkey && !ctx->F.zkey_dbg &&
         ctx->F.closest_mask == 0 && ctx->V.cam.n < 2 && ctx->V.n % M == 0 && dma_multi_lds(ctx) <= 160u * 1024u;
}

// static LDS of one resident solve block of a streamed pass (solve_po_kernel<.., kStream>; tools/kernel_resources.py): 28.2 KB for a
// lens that runs as straight-line code -- built into the library, or specialised at run time once its code object is there --,
// 52.2 KB with the table interpreter
static size_t solve_block_lds(lentil_hip_ctx *ctx) {
  const bool straight = ctx->use_generated && (lentil_hip_lens_is_compiled(ctx) || jit_function(ctx, false, true) != nullptr);
  return straight ? 29184u : 53760u;
}
// Do a scan block with `scan_lds` bytes of dynamic LDS and n resident solve blocks of a streamed pass fit a CU's 160 KB
// together (solve_lds: solve_block_lds)?  Where they do not, whichever the dispatcher places first keeps the other out, and the pass stalls.
// `slack`: 512 bytes for what a scan block takes beyond its dynamic LDS where the streamed pass asks (its gate, its count of
// solve blocks per CU), none where plan_scan picks scan_dma2_kernel -- the figures that choice was measured and tested with
// (101.5 + 2 x 28.5 KB, tests/scan_shapes.py); the two are kept apart so that neither answer moves.
static bool fits_cu_beside_solves(size_t scan_lds, unsigned n_solve, size_t solve_lds, size_t slack) {
  return scan_lds + slack + (size_t)n_solve * solve_lds <= 160u * 1024u;
}

static int plan_scan(lentil_hip_ctx *ctx, ScanPlan &pl) {
  ScanArgs &sa = pl.sa;
  sa.P = ctx->P;
  sa.lens_length = ctx->have_lens ? ctx->hlens.length : 0.0;
  sa.V = ctx->V;
  sa.F = ctx->F;
  const uint32_t M = ctx->V.visits_per_pixel;
  pl.M = M;
  bool direct = false;       // the kernel adds the pixels' own sums to FrameDev::dir
  if (M) {
    const size_t queues = 4 * kWaveQueueLds * sizeof(uint2);
    // staging: 20 B per visit per wave, 4 waves per block, keep a block under ~48 KiB
    uint32_t ppt = 64;
    // extra AOV columns are streamed one at a time: more, smaller tiles keep enough loads in flight
    // (beauty only: 64-pixel tiles, three blocks per CU.  32-pixel tiles / four blocks per CU are 3 % faster for a
    // scan that has the chip to itself -- 0.946 against 0.972 ms -- and 20 % slower beside the first chunk's solve
    // kernel, which then does not get its wave per SIMD until scan blocks retire)
    uint64_t lds_budget = (ctx->V.n_extra ? 24ull : 48ull) * 1024ull;
    if (const char *e = getenv("LENTIL_SCAN_LDS_KB")) lds_budget = strtoull(e, nullptr, 10) * 1024ull;
    while (ppt > 1 && (uint64_t)ppt * M * 20ull * 4ull > lds_budget) ppt >>= 1;
    if ((uint64_t)ppt * M * 20ull * 4ull > 150ull * 1024ull)
      return fail(ctx, LENTIL_ERR_UNSUPPORTED, "visits_per_pixel too large for the LDS staging area");
    // frames with extra AOVs: all columns of a visit in flight at once, one step = 64 / M whole pixels
    const bool multi = ctx->V.n_extra > 0 && M <= 64 && !getenv("LENTIL_SCAN_SINGLE_COLUMN");
    // ring slots of scan_dma_kernel (LENTIL_DMA_RING; a streamed pass has one scan block per CU and LDS to spare)
    uint32_t dma_ring = kDmaRing;
    if (const char *e = getenv("LENTIL_DMA_RING")) { const int r = atoi(e); if (r >= 2 && r <= 8) dma_ring = (uint32_t)r; }
    const size_t dma_lds = (size_t)4 * dma_wave_f4(M, dma_ring) * 16 + queues;
    const bool dma = ctx->scan_dma && ctx->V.n_extra == 0 && !ctx->V.inv_density && !ctx->F.zkey && !ctx->F.zkey_dbg && ctx->V.cam.n < 2 &&
                     ctx->V.n % M == 0 && dma_lds <= 80u * 1024u;
    if (dma_multi_applies(ctx)) {
      // frames with extra AOVs, all of them gaussian: the LDS-DMA form of the multi-column scan (LENTIL_SCAN_DMA_MULTI=0: never)
      pl.kind = LENTIL_SCAN_DMA_MULTI;
      direct = true;
      ppt = 64 / M;
      // the sum lanes come in passes of 64 float4 of the group's records: a pixel fewer per group where that saves the
      // second pass (nine visits, nine AOVs: 7 x 10 float4 = two passes, 6 x 10 = one; 3.19 against 3.39 ms)
      const uint32_t q = ctx->F.stride / 4;
      if (ppt * q > 64 && 64 / q >= 1 && 4 * (64 / q) >= 3 * ppt) ppt = 64 / q;
      if (const char *e = getenv("LENTIL_DMA_MULTI_PPT")) { const uint32_t f = (uint32_t)atoi(e); if (f >= 1 && f <= 64 / M) ppt = f; }
      pl.lds = dma_multi_lds(ctx);
      sa.dummy = ctx->d_dummy;
      // (the column loads without the nontemporal hint: the 54-visit groups of nine-visit pixels do not end on 128-byte lines,
      // and the line two groups share is then still in L2 for the second -- 3.05 against 3.16 ms alone; LENTIL_DMA_MULTI_NT=1)
      sa.ring = dma_multi_ring(ctx) | ((getenv("LENTIL_DMA_MULTI_NT") && getenv("LENTIL_DMA_MULTI_NT")[0] == '1') ? 0u : 0x100u);
    } else if (dma) {
      // beauty only, uniform weights: scan_dma_kernel, or its pipelined form scan_dma2_kernel -- tiles pipelined into one
      // another (two rgba buffers per wave), one block per CU.  In a streamed pass the block must fit beside the resident solve
      // blocks, or neither it nor they would ever end (LENTIL_SCAN_DMA2=0: never)
      direct = true;
      ppt = 64;
      sa.ring = dma_ring;
      static const bool dma2_allowed = !(getenv("LENTIL_SCAN_DMA2") && getenv("LENTIL_SCAN_DMA2")[0] == '0');
      const size_t dma2_lds = (size_t)4 * dma2_wave_f4(M) * 16 + queues;
      const uint64_t ppr = ctx->V.pixels_per_row;
      const bool dma2 = dma2_allowed && M >= 2 && ppr >= 2 && ppr < (1ull << 31) && ctx->V.n / M < (1ull << 31) &&
                        fits_cu_beside_solves(dma2_lds, ctx->stream_mode ? (unsigned)ctx->stream_blocks : 0u, solve_block_lds(ctx), 0);
      pl.kind = dma2 ? LENTIL_SCAN_DMA2 : LENTIL_SCAN_DMA;
      pl.lds = dma2 ? dma2_lds : dma_lds;
      if (dma2) {
        sa.bands = scan_bands(ctx->P);
        uint32_t sh = 0;
        while ((2ull << sh) < ppr) ++sh;                 // 2^sh < ppr <= 2^(sh+1)
        sa.ppr_shift = sh;
        sa.ppr_magic = (uint32_t)(((1ull << (32 + sh)) + ppr - 1) / ppr);
      }
    } else if (multi) {
      pl.kind = LENTIL_SCAN_UNIFORM_MULTI;
      ppt = 64 / M;
      const size_t wave_f4 = (size_t)ctx->F.n_aovs * kMultiPlane + 16 + (size_t)ppt * (ctx->F.stride / 4);
      pl.lds = 4 * wave_f4 * 16 + queues;
    } else {
      pl.kind = LENTIL_SCAN_UNIFORM;
      pl.lds = (size_t)ppt * M * 20 * 4 + queues;
    }
    sa.ppt = ppt;
    sa.tv_pad = ppt * M;
    const uint64_t n_pixels = (ctx->V.n + M - 1) / M;
    pl.n_tiles = (n_pixels + ppt - 1) / ppt;
  }
  lentil_hip_ctx::DirRegion reg;
  if (direct) {
    reg.x0 = ctx->V.pixel_x0; reg.y0 = ctx->V.pixel_y0; reg.row_stride = ctx->V.pixel_row_stride; reg.ppr = ctx->V.pixels_per_row;
    reg.npix = ctx->V.n / M;
  }
  const int rc = prepare_direct(ctx, direct ? &reg : nullptr);
  if (rc) return rc;
  sa.F = ctx->F;
  return LENTIL_OK;
}

// the grid a launch over a chunk's tiles (visits, where the stream has no whole pixels) gets
static ScanGrid scan_grid(const lentil_hip_ctx *ctx, const ScanPlan &pl, const lentil_hip_ctx::Chunk &ch, bool streamed_pass) {
  const uint64_t tiles = ch.tile_end - ch.tile_begin, cus = (uint64_t)ctx->num_cu;
  auto persistent = [](uint64_t want, uint64_t most) { const uint64_t b = want > most ? most : want; return b < 1 ? (uint64_t)1 : b; };
  ScanGrid g;
  switch (pl.kind) {
  case LENTIL_SCAN_DMA2:
    g.blocks = persistent((tiles + 15) / 16, cus);
    // (a streamed pass may leave some CUs without a scanning block: those take a third resident solve block, scan_cus_pct;
    // the blocks that do not scan are launched all the same and leave at once, see the kernel)
    // (only where the pass is bound by its solves: 1080p with 256 draws -- 73 k draws a frame -- is not, 0.74 against 0.71 ms)
    if (streamed_pass && ctx->scan_cus_pct < 100 && g.blocks == cus && ctx->est_sum_total >= (1ull << 19))
      g.skipped = (unsigned)(g.blocks - (cus * (uint64_t)ctx->scan_cus_pct + 99) / 100);
    break;
  case LENTIL_SCAN_DMA: {
    // persistent, every wave draws four tiles at a time
    // one block per CU: 1.07 ms alone against 0.98 with two, but a CU then has room (registers, LDS) for three solve
    // blocks beside it, and a streamed pass ends when its solves do
    uint64_t per_cu = ctx->stream_mode ? 1 : 2;
    if (const char *e = getenv("LENTIL_DMA_BLOCKS")) per_cu = strtoull(e, nullptr, 10);
    g.blocks = persistent((tiles + 15) / 16, cus * per_cu);
    break;
  }
  case LENTIL_SCAN_DMA_MULTI: {
    // persistent: a wave draws runs of 16 groups
    const uint32_t per_cu = dma_multi_blocks_per_cu(ctx);
    g.blocks = persistent((tiles + 4 * kDmaMultiRun - 1) / (4 * kDmaMultiRun), cus * per_cu);
    // (scan_cus_pct: this kernel's blocks draw all their tiles from one counter, so fewer of them is all it takes -- the CUs
    // left alone hold a third resident solve block)
    if (streamed_pass && ctx->scan_cus_pct_multi < 100 && g.blocks == cus && per_cu == 1) {
      const uint64_t keep = (cus * (uint64_t)ctx->scan_cus_pct_multi + 99) / 100;
      g.skipped = (unsigned)(g.blocks - keep);
      g.blocks = keep;
    }
    break;
  }
  case LENTIL_SCAN_UNIFORM:
  case LENTIL_SCAN_UNIFORM_MULTI:
    g.blocks = std::min((tiles + 3) / 4, cus * 8);
    break;
  default:
    g.blocks = std::min((ch.v_end - ch.v_begin + 255) / 256, cus * 8);
  }
  return g;
}

// (own_events: a streamed pass's single launch is timed by its own dispatch, lentil_hip_last_timing)
static void launch_scan_kernel(lentil_hip_ctx *ctx, void (*kernel)(ScanArgs), uint64_t blocks, size_t lds, bool own_events, const ScanArgs &sa) {
  if (own_events) hipExtLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, ctx->ev_scan_k[0], ctx->ev_scan_k[1], 0, sa);
  else hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, sa);
}

// one scan launch over a chunk's range of the stream (ch.tile_begin/_end, ch.v_begin/_end) on the main stream
static int launch_scan(lentil_hip_ctx *ctx, const ScanPlan &pl, const lentil_hip_ctx::Chunk &ch, DevCounters *ctr, bool streamed_pass = false) {
  ScanArgs sa = pl.sa;
  // (LENTIL_SCAN_OUTSIDE_IN=1: a streamed pass scans the frame from its top and bottom edge inwards.  Measured neutral,
  // 2.32-2.33 ms either way: the parked solves of the edge items then come early, but the straggler kernel only gets its
  // registers when the scan's waves have left, scan_order in lentil_kernels.h)
  const char *oi = getenv("LENTIL_SCAN_OUTSIDE_IN");
  const bool outside_in = oi && oi[0] == '1';
  sa.outside_in = (outside_in && streamed_pass) ? 1u : 0u;
  sa.work = ctx->d_work + ch.v_begin;
  sa.work_cap = ch.v_end - ch.v_begin;
  sa.ctr = ctr;
  sa.tile_begin = ch.tile_begin; sa.tile_end = ch.tile_end;
  sa.v_begin = ch.v_begin; sa.v_end = ch.v_end;
  const ScanGrid g = scan_grid(ctx, pl, ch, streamed_pass);
  uint32_t kind = pl.kind;
  // runs of a pixel's visits are summed in their order (LENTIL_SCAN_RUNS=0: an atomic per visit and float, any order)
  if (kind == LENTIL_SCAN_RAGGED && !(getenv("LENTIL_SCAN_RUNS") && getenv("LENTIL_SCAN_RUNS")[0] == '0')) kind = LENTIL_SCAN_RUNS;   // (read per launch: the tests switch it)
  if (kind == LENTIL_SCAN_DMA2) sa.skip_blocks = g.skipped;
  void (*const kernel)(ScanArgs) = kind == LENTIL_SCAN_DMA2 ? scan_dma2_kernel : kind == LENTIL_SCAN_DMA ? scan_dma_kernel :
                                   kind == LENTIL_SCAN_DMA_MULTI ? scan_dma_multi_kernel : kind == LENTIL_SCAN_UNIFORM ? scan_uniform_kernel :
                                   kind == LENTIL_SCAN_UNIFORM_MULTI ? scan_uniform_multi_kernel : kind == LENTIL_SCAN_RUNS ? scan_runs_kernel : scan_ragged_kernel;
  ctx->scan_kernel_timed = streamed_pass && (kind == LENTIL_SCAN_DMA2 || kind == LENTIL_SCAN_DMA || kind == LENTIL_SCAN_DMA_MULTI);
  launch_scan_kernel(ctx, kernel, g.blocks, pl.lds, ctx->scan_kernel_timed, sa);
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_scan[0] = kind;
  ctx->last_scan[1] = pl.M ? sa.ppt : 0u;
  ctx->last_scan[2] = (uint32_t)pl.lds;
  ctx->last_scan[3] = (uint32_t)g.blocks;
  ctx->last_scan_skipped = g.skipped;
  return LENTIL_OK;
}
