// lentil_stream_pass.h -- host side of the streamed pass (redistribute_streamed): the gates that decide whether a pass streams,
// its form (StreamForm: every decision, made before the first launch), the kernels' arguments, the launches of its head and of
// its three tails, and its end -- deferred, or awaited and looked at by streamed_finish.  Included by lentil_hip.hip (StreamTail
// is defined there, ahead of the context that keeps it while a pass's end is pending); no kernels here, and not among the
// sources the run-time lens compiler sees.
#pragma once

// Streamed pass.  The chunked pass above cannot start a chunk's solves before the chunk's scan has ended, and
// every chunk's first solve kernel brings its own ramp-down; solve kernels of several chunks resident at once take
// the register file from the scan.  Here the whole stream is ONE scan launch that publishes items and first-batch
// tasks as it finds them (publish_item), and the first round is one task queue followed by persistent solve waves:
//   stream A (chunk 0's): solve_po_kernel<.., kStream>, `stream_blocks` blocks per CU, resident beside the scan
//                         from the start of the pass
//   main stream:          scan, then a second launch of the same kernel on the CUs' remaining room, then -- once
//                         both have run dry -- the parked stragglers, the first accept and the later rounds
//                         (ordinary queues written by the accept kernel).
// Nothing on the device waits for a kernel that has not been submitted before it: under a profiler that runs
// kernels one at a time, A starts after the scan and finds the queue complete.
// Buffers are sized from the previous pass (twice what it found); an item that does not fit raises
// DevCounters::fallback, the accept kernel then does nothing and the host redoes the draws with exact sizes.
// ---------------------------------------------------------------------------------------

// The end of a streamed pass: its counters have arrived in `pinned`.  What they say -- everything fitted?  the lean tail's bet
// held?  nobody gave up waiting? -- and, where not, the work that is left (can_fix; false for a pass whose frame has been
// cleared since: its verdict is only counted).  Sizes the next pass from what this one found.
static int streamed_finish(lentil_hip_ctx *ctx, StreamTail &t, const DevCounters *pinned, bool can_fix, bool *streamed) {
  const int C = ctx->n_chunks;
  lentil_hip_ctx::Chunk &ch = ctx->chunks[0];
  int rc;
  ctx->h_ctr.assign(pinned, pinned + C);
  ctx->h_ctr_valid = true;
  ctx->last_streamed = 1;
  const DevCounters c = ctx->h_ctr[0];
  ch.was_blind = true;
  if (c.probe_snap[0]) {
    // LENTIL_DISPATCH_PROBE: the first accept's last item was finished while blocks of its grid had not begun
    char buf[640];
    int n = snprintf(buf, sizeof buf, "[probe] epoch %u: accept blocks begun %u of %u when the last item was done; per XCD begun:", ctx->epoch, c.probe_snap[33], c.probe_snap[34]);
    for (int x = 0; x < 8; ++x) n += snprintf(buf + n, sizeof buf - n, " %u", c.probe_snap[1 + x]);
    const char *kinds[3] = {"second round's solve waves resident", "second round's straggler waves resident", "first round's straggler waves resident"};
    for (int k = 0; k < 3; ++k) {
      n += snprintf(buf + n, sizeof buf - n, " | %s:", kinds[k]);
      for (int x = 0; x < 8; ++x) n += snprintf(buf + n, sizeof buf - n, " %u", c.probe_snap[9 + 8 * k + x]);
    }
    fprintf(stderr, "%s\n", buf);
  }
  if (c.fallback || c.stuck) {
    // what made the pass give up, kept for lentil_hip_last_redo_note(): `fallback` bits 1 items, 2 result pool, 4 task queue,
    // 8 a wave's pending flushes, 16 range queue, 32 the blind preparation's bounds (64, chunked passes only: a list of occlusion probes); `stuck` = (ticket << 2) | who waited (1 a
    // publisher, 2 a resident solve wave, 3 a straggler wave)
    char note[768];
    snprintf(note, sizeof note,
             "epoch %u: fallback 0x%llx stuck 0x%x (timeout %.0f ms)%s%s | items %llu/%u tasks %u/%u pool %llu/%llu ranges %u/%u | "
             "scan blocks done %u publishers done %u rounds_used %llu | first batches %s, margin16 %u, blind passes before %u | "
             "the wave that gave up: round %u parity %u, its queue's n_tasks %u head %u, accept blocks done %u begun %u, slot word 0x%x (epoch tag 0x%x), block %u",
             ctx->epoch, (unsigned long long)c.fallback, c.stuck, (double)t.stuck_ticks * 1.0e-5,
             c.stuck ? " waited: " : "", c.stuck ? ((c.stuck & 3u) == 1 ? "publisher" : (c.stuck & 3u) == 2 ? "resident solve wave" : "straggler wave") : "",
             (unsigned long long)c.work_count, t.item_cap, c.n_tasks[0], t.task_cap, (unsigned long long)c.pool_used[0],
             (unsigned long long)t.pool_cap, c.n_ranges, t.range_cap, c.scan_blocks_done, c.publishers_done,
             (unsigned long long)c.rounds_used, t.predicted ? "modelled" : "plain", ctx->bm_margin16, ctx->last_blind - 1u,
             c.stuck_info[0], c.stuck_info[1], c.stuck_info[2], c.stuck_info[7], c.stuck_info[3], c.stuck_info[4], c.stuck_info[5],
             c.stuck_info[5] >> kTaskTagShift, c.stuck_info[6]);
    ctx->redo_note = note;
    if (c.stuck && (c.stuck & 3u) == 1u && ctx->d_ranges) {
      // a publisher gave up on its range slot: what the slot holds now (every kernel of the pass has left), the slots around the
      // cursor and the queue's counters as the host reads them -- a record that IS there was written and not seen
      const uint32_t tk = c.stuck >> 2;
      uint64_t w[4] = {0, 0, 0, 0};
      if ((uint64_t)tk + 2 < ctx->range_cap)
        (void)hipMemcpy(w, ctx->d_ranges + (tk ? tk - 1 : 0), sizeof w, hipMemcpyDeviceToHost);
      char more[256];
      snprintf(more, sizeof more, " | range slots from %u on (host read-back): %016llx %016llx %016llx %016llx, range_head %u",
               tk ? tk - 1 : 0, (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)w[3], c.range_head);
      ctx->redo_note += more;
    }
    if (getenv("LENTIL_STREAM_DEBUG")) {
      fprintf(stderr, "[stream] note: %s\n", ctx->redo_note.c_str());
      fprintf(stderr, "[stream] redo: who %u ticket %u epoch %u range_head %u pubs_done %u scan_done %u | fallback %llu stuck %u | items %llu (cap %u) tasks %u (cap %u) pool %llu (cap %llu) ranges %u (cap %u)\n",
              c.stuck & 3u, c.stuck >> 2, ctx->epoch, c.range_head, c.publishers_done, c.scan_blocks_done, c.fallback, c.stuck, c.work_count, t.item_cap, c.n_tasks[0], t.task_cap, c.pool_used[0], (unsigned long long)t.pool_cap,
              c.n_ranges, t.range_cap);
      HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      HIP_TRY(ctx, hipEventSynchronize(ctx->ev[2]));
      float ms_scan = 0.f, ms_all = 0.f;
      (void)hipEventElapsedTime(&ms_scan, ctx->ev[0], ctx->ev[1]);
      (void)hipEventElapsedTime(&ms_all, ctx->ev[0], ctx->ev[2]);
      fprintf(stderr, "[stream] scan %.3f ms, pass until the read-back %.3f ms\n", ms_scan, ms_all);
      fprintf(stderr, "[stream] queues: n_tasks %u/%u task_head %u/%u n_active %u/%u active_head %u/%u accept_done %u/%u pool_used %llu/%llu\n",
              c.n_tasks[0], c.n_tasks[1], c.task_head[0], c.task_head[1], c.n_active[0], c.n_active[1], c.active_head[0], c.active_head[1],
              c.accept_done[0], c.accept_done[1], c.pool_used[0], c.pool_used[1]);
      fprintf(stderr, "[stream] stragglers: live %d waves_done %u/%u (round 1: %u) parked %u/%u heads %u/%u cap %u waves %u rounds_used %llu\n", (int)t.live,
              c.waves_done[0], c.waves_started[0], c.waves_done[1], c.n_slow[0], c.n_slow[1], c.slow_head[0], c.slow_head[1],
              t.da.slow_cap, t.da.slow_waves, c.rounds_used);
    }
    if (c.stuck) {
      g_stat_stuck.fetch_add(1, std::memory_order_relaxed);
      if (t.inject) g_stat_stuck_injected.fetch_add(1, std::memory_order_relaxed);
      else {
        std::lock_guard<std::mutex> lock(g_stall_notes_mutex);
        if (g_stall_notes.size() < 8) g_stall_notes.push_back(ctx->redo_note + (t.deferred ? " | end deferred" : " | end awaited") + (can_fix ? "" : ", abandoned") +
                                                              " | frame " + std::to_string(ctx->P.xres) + "x" + std::to_string(ctx->P.yres) + ", " + std::to_string(ctx->V.n) + " visits");
      }
    }
    if (ctx->notes.size() < 8) ctx->notes.push_back(ctx->redo_note);
    if (!can_fix) {
      // abandoned: the frame this pass wrote into has been cleared since; what it lacked is counted, not done
      if (c.stuck) ++ctx->n_stuck;
      ++ctx->last_fallback;
      ++ctx->totals.abandoned_incomplete;
      ctx->last_rounds = (int)c.rounds_used;
      if (!c.stuck) {
        // (the scan and the publishers counted everything they met, whether or not it fitted: the next pass is sized from that)
        const uint64_t n_items = c.work_count < ctx->V.n ? c.work_count : ctx->V.n;
        ctx->have_total_est = true;
        ctx->est_items_total = n_items; ctx->est_sum_total = c.sum_samples;
      }
      for (int ci = 0; ci < C; ++ci) ctx->chunks[ci].have_est = false;
      *streamed = true;
      return LENTIL_OK;
    }
    t.did_more = true;
    if (c.stuck && c.rounds_used) {
      // Stalled with draws already accepted: the frame holds a part of the pass.  It held nothing before (the gate at the
      // top), so lentil_hip_redistribute wipes it and runs the whole pass again in the chunked form.
      ++ctx->n_stuck;
      ctx->stall_redo = true;
      ctx->h_ctr_valid = false;
      ctx->late_resolve_done = false;
      *streamed = true;
      return LENTIL_OK;
    }
    if (c.stuck) {
      ++ctx->n_stuck;
      HIP_TRY(ctx, hipMemsetAsync((char *)ctx->d_ctr + offsetof(DevCounters, stuck), 0, sizeof(unsigned int), ch.stream));
    }
    // did not fit: nothing was accepted.  Fresh queues, then the draws again the plain way, sized from the counters
    ctx->h_ctr_valid = false;
    ctx->late_resolve_done = false;
    ++ctx->last_fallback;
    HIP_TRY(ctx, hipMemsetAsync((char *)ctx->d_ctr + offsetof(DevCounters, n_tasks), 0,
                                offsetof(DevCounters, inv_row_min) - offsetof(DevCounters, n_tasks), ch.stream));
    HIP_TRY(ctx, hipMemsetAsync((char *)ctx->d_ctr + offsetof(DevCounters, fallback), 0, sizeof(unsigned long long), ch.stream));
    DrawArgs db{};
    init_draw_args(ctx, db);
    if ((rc = enqueue_chunk_draws(ctx, 0, db, 3))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ch.stream));
    int rounds = 3;
    if (ch.n_items) { if ((rc = finish_rounds(ctx, 0, db, 3, &rounds))) return rc; }
    ch.est_rounds = rounds;
    ctx->last_rounds = rounds;
  } else {
    const uint64_t n_items = c.work_count < ctx->V.n ? c.work_count : ctx->V.n;
    ch.have_est = true; ch.est_items = n_items; ch.est_sum = c.sum_samples; ch.est_rounds = (int)c.rounds_used;
    if (c.tries) { ctx->mean_iters = (double)c.newton_iters / (double)c.tries; ctx->parked_frac = (double)c.slow_solves / (double)c.tries; }
    int rounds = t.blind_rounds;
    if (t.lean) ++ctx->n_lean;
    // A pass whose first batches came from the model and left an item short all the same: the model's margin widens for the
    // passes that follow (the item is served by further rounds as ever); with the margin at its cap the context stops
    // betting on the lean tail until its camera set-up changes.
    const bool short_after_all = t.predicted && n_items && (c.n_tasks[1] != 0u || (t.lean && c.n_active[t.blind_rounds & 1] != 0u));
    // (an abandoned pass: what it still needed is counted, not done -- nobody can see its frame any more)
    const bool open_end = n_items && ((t.lean && c.n_tasks[1] != 0u) || c.n_active[t.blind_rounds & 1] != 0);
    if (open_end && !can_fix) {
      ++ctx->totals.abandoned_incomplete;
      if (ctx->notes.size() < 8) ctx->notes.push_back("abandoned before its end was looked at: the first accept had scheduled another round (lean tail's bet lost)");
    } else if (open_end) {
      t.did_more = true;
    }
    if (short_after_all) {
      // (a pass that loses only now and then keeps betting: the margin comes back down after 16 passes without a loss)
      ctx->bm_since_loss = 0;
      if (ctx->bm_margin16 >= 4u) ctx->lean_ok = false;
      else ctx->bm_margin16 += 1u;
    }
    if (t.predicted && !short_after_all && ++ctx->bm_since_loss >= 16u && ctx->bm_margin16 > 0u) { --ctx->bm_margin16; ctx->bm_since_loss = 0; }
    if (!can_fix && open_end) {
      if (t.lean) ++ctx->n_lean_lost;
      rounds = (int)c.rounds_used + 1;
    } else
    if (t.lean && n_items && c.n_tasks[1] != 0u) {
      // The lean tail's bet was lost: the first accept scheduled tasks, the accept behind it did nothing.  The round the
      // ordinary way -- its solves (the queue is complete), their stragglers, the accept that was held back -- then whatever
      // rounds follow.  (Rare: an item whose first batch the model sized too small; ~0.3 ms.)
      ctx->h_ctr_valid = false;
      ctx->late_resolve_done = false;
      t.da.parity = 1; t.da.round = 1;
      t.da.producers_done = nullptr; t.da.producers_total = 0;
      t.da.slow_live = 0; t.da.slow_indirect = 0; t.da.slow_q = -1; t.da.slow_round = -1; t.da.slow_close = 1;
      t.da.emit_live = 0; t.da.lean_gate = 0; t.da.no_reset = 1;
      {
        DrawArgs dr = t.da;       // (its parked solves go to the upper half of the records: the lower half holds the first round's results)
        if (dr.slow) { dr.slow = t.slow_base + t.slow_cap_all / 2u; dr.slow_cap = t.slow_cap_all - t.slow_cap_all / 2u; }
        launch_solve(ctx, dr, ch.stream, (unsigned)ctx->num_cu);
      }
      hipLaunchKernelGGL(reset_round_kernel, dim3(1), dim3(1), 0, ch.stream, ctx->d_ctr, 0u, 1u);
      hipLaunchKernelGGL(accept_kernel<2>, dim3(t.accept_blocks), dim3(256), 0, ch.stream, t.da);
      HIP_TRY(ctx, hipGetLastError());
      t.da.no_reset = 0;
      if ((rc = finish_rounds(ctx, 0, t.da, 2, &rounds))) return rc;
      if (rounds > ch.est_rounds) ch.est_rounds = rounds;
      ++ctx->n_lean_lost;
    } else
    if (n_items && c.n_active[t.blind_rounds & 1] != 0) {
      ctx->h_ctr_valid = false;
      ctx->late_resolve_done = false;
      if ((rc = finish_rounds(ctx, 0, t.da, t.blind_rounds, &rounds))) return rc;
      if (rounds > ch.est_rounds) ch.est_rounds = rounds;
      if (t.lean) ++ctx->n_lean_lost;
    } else if (t.lean) {
      rounds = 1;       // one round of solves: the accept behind the first one only waited for that round's parked solves
    }
    ctx->last_rounds = rounds;
  }
  ctx->have_total_est = true;
  ctx->est_items_total = ch.est_items; ctx->est_sum_total = ch.est_sum; ctx->est_rounds_total = ch.est_rounds;
  // (should the next pass run chunked, its chunks look at their scans first: this pass knows nothing about them)
  for (int ci = 0; ci < C; ++ci) ctx->chunks[ci].have_est = false;
  *streamed = true;
  return LENTIL_OK;
}

// ---- gates --------------------------------------------------------------------------------------------------------------
// Does this pass stream?  On true the device's turn is taken, `da` holds the pass's draw arguments as init_draw_args makes
// them, and `items` / `units` what its buffers are sized for.
static bool stream_pass_applies(lentil_hip_ctx *ctx, DeviceTurn &turn, DrawArgs &da, uint64_t &items, uint64_t &units) {
  const lentil_params &P = ctx->P;
  if (!ctx->stream_mode || P.cameraType != LENTIL_POLYNOMIAL_OPTICS || !ctx->have_total_est || ctx->V.n == 0)
    return false;
  if (ctx->V.n > 0xFFFFFFF0ull) return false;
  if (no_tries(P)) return false;         // (vignetting_retries < 0: a scan and a count, enqueue_chunk_draws)
  if (probing(ctx)) return false;      // (occlusion probes, host or device callback: answered between a round's solves and its accept -- the round-by-round form)
  if (ctx->pass_spectral) return false;      // (a wavelength per visit: solve_po_spectral_kernel, launched by the round-by-round form alone)
  // Only into a frame that has been cleared since its last pass (every caller's order: clear, redistribute, resolve): a
  // streamed pass whose waves give up waiting after draws have been accepted is recovered by wiping the frame and running
  // the pass again, which must not cost an earlier pass's sums.  A second pass into the same frame takes the chunked form,
  // whose kernels never wait for one another.
  if (!ctx->cleared_since_pass) return false;
  // A context whose resident waves have given up waiting before (250 ms each time, then the redo) stops trying: at once
  // where lentil_hip_create found its streams sharing hardware queues (GPU_MAX_HW_QUEUES below 4: a kernel then sits behind
  // the one it waits for, every pass), after the third time anywhere else (a profiler that serialises kernels, a crowded GPU).
  if (ctx->n_stuck >= (ctx->streams_concurrent ? 3u : 1u)) return false;
  // Streaming pays where the scan is most of the pass.  With many draws the chunked pass is ahead (highlight-heavy
  // frame: 114 ms against 135 ms; 15 M draws: 16.6 against 18.4 ms -- solve waves placed while the scan's are
  // resident keep running slower long after those have left, see launch_chunk_rounds), and so it is with extra
  // AOVs, whose scan kernel leaves the solve waves less room (config 4: 10.8 against 11.5 ms).
  // (Round 3: ... or below one draw per 24 visits, whichever is more -- what streaming buys is the scan running beside the
  // solves, and a frame whose scan is long against its draws gains most: BASELINE config 5, 8K with 9.3 M draws, 12.9 ms
  // streamed against 16.3 chunked; 4K with 3.1 M draws 4.3 against 4.8 ms, with 6-48 M draws within +-5 % either way.)
  {
    const uint64_t by_visits = ctx->stream_below_set ? 0ull : ctx->V.n / 24ull;
    if (ctx->est_sum_total >= (ctx->stream_below > by_visits ? ctx->stream_below : by_visits)) return false;
  }
  if (ctx->V.n_extra && !dma_multi_applies(ctx)) return false;
  // ... nor where a scan block could not share a CU's LDS with even one resident solve block (scan_dma_multi_kernel from twelve
  // extra AOVs on, from nine beside the table interpreter): whichever the dispatcher places first keeps the other out, and where
  // that is the solve blocks they wait for a scan that cannot start until a publisher gives up -- 250 ms, then the redo
  // (tests/test_gpu_scan_shapes.py: second passes with 14 and 15 extra AOVs)
  if (ctx->V.n_extra && !fits_cu_beside_solves(dma_multi_lds(ctx), 1u, solve_block_lds(ctx), 512u)) return false;
  // One streamed pass per device at a time: the resident kernels of two of them could keep each other's scan off the chip.
  // A context that finds another one's streamed pass in flight does not wait for it: its pass runs in the chunked form,
  // whose kernels never wait for anything (LENTIL_STREAM_WAIT=1: wait, as rounds 2 did).
  static const bool wait_for_turn = getenv("LENTIL_STREAM_WAIT") && getenv("LENTIL_STREAM_WAIT")[0] == '1';
  if (!turn.take(wait_for_turn)) return false;
  init_draw_args(ctx, da);
  // (counted BEFORE the last gate: LENTIL_INJECT_STALL=k names the k-th pass that got this far, and the tests count with it)
  ++ctx->n_streamed;
  g_stat_streamed.fetch_add(1, std::memory_order_relaxed);
  da.inject_stall = (ctx->inject_stall_at > 0 && ctx->n_streamed == (uint64_t)ctx->inject_stall_at) ? 1 : 0;
  items = 2 * ctx->est_items_total + 4096;
  if (items > ctx->V.n) items = ctx->V.n;
  units = chunk_units(P, (uint64_t)da.n_channels, 2 * ctx->est_sum_total + (1ull << 20), items);
  return units <= ctx->max_pool_units;       // (more: sub-batches, the chunked pass knows how)
}

// Buffers, the scan's plan, the chunk's range, the pass's epoch and the range queue: all that has to exist before the pass's
// form is decided and its first kernel launched.
static int stream_prepare(lentil_hip_ctx *ctx, DrawArgs &da, uint64_t items, uint64_t units, ScanPlan &plan) {
  lentil_hip_ctx::Chunk &ch = ctx->chunks[0];
  int rc;
  if ((rc = size_chunk_buffers(ctx, ch, items, units))) return rc;
  bind_chunk_buffers(ch, da);
  if ((rc = plan_scan(ctx, plan))) return rc;
  da.F = ctx->F;                // (plan_scan decides where the direct sums go and whether splats are flagged)
  // the wipe clear_frame left on the chunk stream (clear_pending) rides beside the scan only where the scan leaves the splat
  // accumulators alone: own sums to FrameDev::dir, splats flagged
  if (ctx->clear_pending && !(ctx->F.dir && ctx->F.touched) && (rc = join_clear(ctx))) return rc;
  ch.tile_begin = 0; ch.tile_end = plan.n_tiles;
  ch.v_begin = 0; ch.v_end = ctx->V.n;
  for (int ci = 1; ci < ctx->n_chunks; ++ci) {
    lentil_hip_ctx::Chunk &o = ctx->chunks[ci];
    o.tile_begin = o.tile_end = plan.n_tiles; o.v_begin = o.v_end = ctx->V.n; o.n_items = 0;
  }
  ctx->epoch = (ctx->epoch + 1u) & 0x3FFFFFu;
  if (ctx->epoch == 0u) {
    // the 22-bit tag has come round: wipe what older passes left in the queues
    ctx->epoch = 1u;
    HIP_TRY(ctx, hipMemsetAsync(ch.tasks[0], 0, ch.task_cap * sizeof(Task), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ch.tasks[1], 0, ch.task_cap * sizeof(Task), ctx->stream));
    if (ctx->d_ranges) HIP_TRY(ctx, hipMemsetAsync(ctx->d_ranges, 0, ctx->range_cap * sizeof(uint64_t), ctx->stream));
    if (ch.slow) HIP_TRY(ctx, hipMemsetAsync(ch.slow, 0, ch.slow_cap * sizeof(SlowRec), ctx->stream));
  }
  // range queue: one record per flush of a wave queue (at most one per 64 visits, plus one per wave and tile)
  const uint64_t need = ctx->V.n / 64 + 2 * plan.n_tiles + 65536;
  if (need > ctx->range_cap) {
    if ((rc = grow(ctx, &ctx->d_ranges, need))) return rc;
    ctx->range_cap = need;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ranges, 0, need * sizeof(uint64_t), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  plan.sa.ranges = ctx->d_ranges;
  plan.sa.range_cap = (uint32_t)(ctx->range_cap < 0xFFFFFFF0ull ? ctx->range_cap : 0xFFFFFFF0ull);
  plan.sa.epoch = ctx->epoch;
  plan.sa.end_ranges = (uint32_t)ctx->publish_waves;
  plan.sa.flush_each_tile = ctx->est_items_total < (1u << 16) ? 1u : 0u;
  return LENTIL_OK;
}

// ---- the form of the pass ------------------------------------------------------------------------------------------------
// Every decision of a streamed pass, made before its first launch (make_stream_form: no launch, no stream operation) and not
// written afterwards: which kernels the pass consists of, on which streams, with which grids.
struct StreamForm {
  bool crypto_overlap = true, overlap_accept = true;      // LENTIL_CRYPTO_OVERLAP, LENTIL_OVERLAP_ACCEPT
  uint64_t nch = 1;                   // wavelength channels per attempt
  uint32_t retries = 0;
  bool inject = false;                // LENTIL_INJECT_STALL: this is the pass that stalls
  bool calibrates_now = false;        // this pass's host time holds the first-batch model's calibration kernel's
  uint64_t stuck_ticks = 0;           // how long a resident wave waits for its queue slot before it declares the pass stuck
  bool few = false;                   // few draws: solves that take long are parked (DrawArgs::slow_below) ...
  SlowRec *slow_base = nullptr;       // ... in these records (null: nothing parks)
  uint32_t slow_cap_all = 0, slow_waves_all = 0;      // how many records there are / straggler waves of a live queue
  bool live = false;                  // live straggler queue: solve_slow_kernel beside the first round's solves
  bool dry_only = false;              // only waves running dry park, and only their last lanes
  int blind_rounds = 2;               // rounds enqueued without looking
  bool overlap_plain = false, overlap = false, decoupled = false;      // how the second round meets the first accept (make_stream_form)
  unsigned a_blocks = 0, b_blocks = 0;      // resident solve blocks beside the scan (A) and behind it (B)
  bool predict = false, predicted = false;  // first batches from the model wanted / published
  bool lean_pass = false, ready_accept = false;      // lean tail: no second round in flight / accept_kernel<3> first
  unsigned accept_blocks = 0, accept1_blocks = 0;      // grid of the accepts / of the first one
  bool resolves_early = false, resolve_after_scan = false;      // the frame's resolve begins inside the pass / behind the scan already
};

static StreamForm make_stream_form(lentil_hip_ctx *ctx, const DrawArgs &seed, const ScanPlan &plan, bool calibrates_now) {
  // the pass's switches: those of the process, then the two the tests switch from pass to pass
  static const double forced_ms = getenv("LENTIL_STUCK_MS") ? atof(getenv("LENTIL_STUCK_MS")) : 0.0;
  static const bool crypto_overlap = !(getenv("LENTIL_CRYPTO_OVERLAP") && getenv("LENTIL_CRYPTO_OVERLAP")[0] == '0');
  const char *overlap_env = getenv("LENTIL_OVERLAP_ACCEPT");      // (read per pass: the tests switch it)
  const int forced_rounds = forced_blind_rounds();
  const lentil_params &P = ctx->P;
  StreamForm f;
  f.crypto_overlap = crypto_overlap;
  f.overlap_accept = !(overlap_env && overlap_env[0] == '0');
  f.nch = (uint64_t)seed.n_channels;
  f.retries = (uint32_t)(P.vignetting_retries < 0 ? 0 : P.vignetting_retries);
  f.inject = seed.inject_stall != 0;
  f.calibrates_now = calibrates_now;
  // How long a resident wave waits for its queue slot before it declares the pass stuck (the host then redoes the pass the
  // chunked way).  A wave may rightly wait for a whole scan -- its slot gets its end marker when the scan ends --, so: 250 ms
  // while nothing is known, else sixteen times the longest pass this context has seen, at least 30 ms (round 5: a stall,
  // rare as it is, then costs tens of milliseconds and not a quarter of a second; LENTIL_STUCK_MS overrides).
  {
    // (the estimate comes from earlier passes: it holds for a pass no larger than the one that set it -- more visits, or a
    // quarter more draws expected, and nothing is known again: 250 ms -- and every time-out this context has hit doubles it,
    // so that a slow box, a shared GPU or a profiler does not turn into a run of false stalls, each a wipe and a chunked redo)
    double ms = 250.0;
    if (ctx->longest_pass_ms > 0.0 && ctx->V.n <= ctx->longest_pass_visits &&
        ctx->est_sum_total <= ctx->longest_pass_sum + ctx->longest_pass_sum / 4) {
      ms = 16.0 * ctx->longest_pass_ms * (double)(1u << (ctx->n_stuck < 4 ? ctx->n_stuck : 4));
      if (ms < 30.0) ms = 30.0;
      if (ms > 250.0) ms = 250.0;
    }
    if (forced_ms > 0.0) ms = forced_ms;
    f.stuck_ticks = (uint64_t)(ms * 1.0e5);
  }
  f.few = ctx->est_sum_total < ctx->slow_below;
  f.slow_base = f.few ? seed.slow : nullptr;              // parking is for passes with few draws (DrawArgs::slow_below)
  f.slow_cap_all = seed.slow_cap;
  // Live straggler queue: solve_slow_kernel is launched behind the publishers (who end with the scan) and takes the parked
  // solves as they come, one wave per CU.  (Round 3, from the timeline: its waves are placed as the first solve waves
  // leave -- the idle ones do at once when the publishers' end markers arrive --, not in the registers the scan gives
  // back: a wave's registers are one contiguous range.)
  f.live = f.slow_base != nullptr && P.cameraType == LENTIL_POLYNOMIAL_OPTICS;
  f.blind_rounds = forced_rounds ? forced_rounds : (ctx->est_rounds_total < 2 ? 2 : (ctx->est_rounds_total > 6 ? 6 : ctx->est_rounds_total));
  // Second round beside the first accept: the accept kernel hands out the next round's tasks as it goes (tagged slots,
  // end markers from its last block), a kStream solve kernel -- one block per CU, which fits beside four accept blocks
  // -- takes them as they come, the straggler kernel beside both.  Launched AFTER the accept, so that a profiler that
  // serialises kernels runs them in an order that completes.
  // (Round 4: also in passes that park nothing -- more draws than LENTIL_SLOW_BELOW, BASELINE config 5 on one GPU: 4 560 items
  // x 2 048 draws --, whose first accept takes 0.65 ms and whose second round used to wait for all of it: 11.7 -> see DESIGN
  // section 5.  No straggler kernels there, just the accept feeding the resident second-round solves.)
  f.overlap_plain = f.slow_base == nullptr && f.nch == 1 && P.cameraType == LENTIL_POLYNOMIAL_OPTICS;
  f.overlap = (f.live || f.overlap_plain) && f.blind_rounds >= 2;
  // ... and the first accept does not wait for the first round's stragglers either (accept_item<1> / <2>): one
  // straggler queue and one solve_slow_kernel launch for both rounds, closed by the second round's solve kernel.
  // (A queue and a solve_slow_kernel launch per round, as ever: ONE kernel for both rounds would wait for end markers from
  // kernels submitted after it -- the first accept, the second round's solves -- and where two of the pass's streams share
  // a hardware queue, the default with the runtime's 4, those sit behind it in that queue: 250 ms, then the chunked redo.
  // The second round parks into the upper half of the record buffer, its kernel follows the first round's on their stream.)
  f.decoupled = f.live && f.overlap && f.nch == 1;
  // A live queue takes every solve that reaches slow_at iterations -- outliers, by the measure of the previous pass.  With
  // a lens where such solves are not outliers (the petzval table: 3 % of all solves, 62 000 a frame, each a whole wave
  // of the straggler kernel: 12 ms a frame against 10 chunked) only waves running dry park, and only their last lanes.
  // (It stays that way for the lens: a pass that parks dry waves' lanes only says nothing about what a live queue would get.)
  if (ctx->parked_frac > 1.0 / 256.0) ctx->park_dry_seen = true;
  f.dry_only = ctx->park_dry_only >= 0 ? ctx->park_dry_only != 0 : ctx->park_dry_seen;
  // (one straggler wave per CU; LENTIL_SLOW_WAVES_PER_CU, up to 4 -- measured on config 4, whose rounds end in hundreds
  // of parked solves at once: 9.15 / 9.18 / 9.35 / 9.46 ms with 1 / 2 / 3 / 4, the waves take from the solve kernel)
  // (Round 6: four per CU where parked solves are the outliers they are meant to be -- beauty-only frames, the live queue.  The
  // straggler kernel had become what the pass ends on: 2 300 parked solves of a headline frame, 27 000 iterations at ~3 us each,
  // are 320 us of work for 256 waves and half of it was still to do when the solve kernel's last wave left; with 1 024 waves
  // it ends with the solve kernel but for the solves that run all 100 iterations.  2.011 -> 1.989 ms, eight interleaved runs of
  // 60 steps each, gpurun_out/r06s05.  Config 4 parks dry waves' lanes only and keeps one.)
  const int slow_per_cu = ctx->slow_waves_per_cu;
  const uint32_t slow_default = (f.nch == 1 && ctx->V.n_extra == 0 && !f.dry_only) ? 4u : 1u;
  uint32_t slow_cu = slow_per_cu >= 1 && slow_per_cu <= 4 ? (uint32_t)slow_per_cu : slow_default;
  const size_t solve_lds = solve_block_lds(ctx);
  if (f.live) {
    // ... and no more per CU than leave room for what they wait for.  A live queue's waves spin on end markers that a resident
    // solve wave writes -- a round later, a solve wave fed by an accept's blocks --, and those kernels are launched beside the
    // straggler kernel, not ahead of it: whichever the dispatcher places first keeps its LDS.  A straggler wave's block is
    // 9-21 KB with the shipped tables and 41 KB with a table of kMaxTerms terms (coop_lds_bytes).  Of the four asked for per CU
    // three of those fit a CU's 160 KB, and with three resident no CU had the 52 KB of an interpreter's solve block left: no
    // task was ever taken, no end marker written, every straggler wave waited out its 250 ms, and every streamed pass of such
    // a table was redone (tests/lens_tables.py, "full").  So: as many as leave a CU one solve block and one accept block
    // -- then not every CU can be full of them.  Four, as ever, with every shipped table on either solve kernel (the
    // largest, petzval_58mm's 707 terms under the interpreter: 4 x 20.0 + 52.5 + 21 = 153.4 KB; two at kMaxTerms).
    // (A queue that is not live has no wave that waits: its kernel runs behind the solves and is left as it was.)
    constexpr size_t kAcceptBlockLds = 21u * 1024u;       // accept_kernel's block: 20.7 KB (tools/kernel_resources.py)
    const size_t wave_lds = coop_lds_bytes(ctx->hlens.n_terms) + sizeof(CoopShared) + 512u;
    while (slow_cu > 1u && !fits_cu_beside_solves((size_t)slow_cu * wave_lds + kAcceptBlockLds, 1u, solve_lds, 0u)) --slow_cu;
  }
  f.slow_waves_all = (uint32_t)ctx->num_cu * slow_cu;
  // A: as many resident solve blocks per CU as leave a scan block its LDS.  (Round 6: the table interpreter's blocks hold 52 KB each --
  // two of them and an 80 KB scan_dma_kernel block do not fit a CU's 160 KB, and where the dispatcher placed the solve blocks
  // first no scan block ever found room: the resident waves waited for a scan that could not start until a publisher gave up,
  // 250 ms, then the redo.  That was the "odd stalled pass" of small frames run through the interpreter -- every test that runs
  // its second pass with lentil_hip_set_lens_mode(ctx, 1) --, found when the library began to count its stalls.  plan_scan only
  // budgeted for scan_dma2_kernel.)
  unsigned a_per_cu = (unsigned)ctx->stream_blocks;
  while (a_per_cu > 1u && !fits_cu_beside_solves(plan.lds, a_per_cu, solve_lds, 512u)) --a_per_cu;
  f.a_blocks = (unsigned)ctx->num_cu * a_per_cu;
  // CUs the scan leaves alone (scan_cus_pct) have registers for one more resident solve block
  if (a_per_cu == 2u) f.a_blocks += scan_grid(ctx, plan, ctx->chunks[0], true).skipped;
  // B: a second solve launch behind the scan, in passes without a live queue.  (Measured, round 3: with the straggler
  // kernel's wave on one of a CU's SIMDs the blocks of this launch are not placed before the first launch's blocks leave --
  // zero iterations in every pass looked at: a pass with a live queue has none.)
  if (!f.live) {
    int b_per_cu = ctx->solve_max_blocks - ctx->stream_blocks;
    if (b_per_cu < 1) b_per_cu = 1;
    const uint64_t want = (f.nch * (ctx->est_sum_total / 64 + ctx->est_items_total) + 3) / 4;
    uint64_t b = (uint64_t)ctx->num_cu * (uint64_t)b_per_cu;
    if (want < b) b = want < 1 ? 1 : want;
    f.b_blocks = (unsigned)b;
  }
  // First batches from the lens and the frame (lentil_batch_model.h): every item is published with the traces it is expected
  // to need, so that the first accept finds nothing to schedule and the pass can do without a second round (lean tail)
  // (Not for items with very many draws each -- BASELINE config 5's 2 048: their first accept is long, 0.3-0.65 ms, and the
  // second round that runs beside it is all but free, while its traces inside the first round are throughput; the bands of
  // that frame, each alone on one GPU, took 5-19 % longer with the lean tail: profiles/r05_emulated_bands.txt.)
  const bool few_draws_per_item = ctx->est_items_total == 0 || ctx->est_sum_total / ctx->est_items_total <= ctx->predict_max_draws;
  f.predict = ctx->predict && f.decoupled && few_draws_per_item;
  f.predicted = f.predict && ctx->bm_valid && ctx->d_bm_land != nullptr;        // (calibrated ahead of the scan, by the caller)
  // The lean tail: known before anything is launched -- the solve and straggler kernels count parked solves per item for
  // accept_kernel<3> (DrawArgs::item_ready) in such a pass.
  // (LENTIL_INJECT_STALL stalls the second round's resident solve waves: that pass keeps its second round in flight)
  f.lean_pass = f.decoupled && f.predicted && ctx->lean_ok && f.blind_rounds <= 2 && !f.inject;
  // Round 6: the first accept takes the items whose parked solves are through, whole, and leaves the others to the accept behind
  // the stragglers (accept_kernel<3>).  For frames the wide walk serves: <= 64 retries, records of <= 64 floats.
  uint32_t add_floats = 1;
  for (uint32_t k = 0; k < ctx->F.n_aovs; ++k) if (!(ctx->F.closest_mask & (1u << k))) add_floats += 4;
  f.ready_accept = f.lean_pass && f.retries <= kAcceptWinRetries && add_floats <= 64u;
  const uint64_t acc_max = (uint64_t)ctx->num_cu * (uint64_t)(ctx->accept_stream_blocks < 1 ? 1 : ctx->accept_stream_blocks);
  const uint64_t acc_want = ctx->est_items_total + ctx->est_items_total / 4 + 1;
  f.accept_blocks = (unsigned)(acc_want > acc_max ? acc_max : acc_want);
  // (lean tail: no next round's solve waves share the CUs with the first accept -- a block per item, as many as fit.)
  // accept_kernel<3> waits for nothing and is what stands between the solve kernel's end and the touched groups' resolve:
  // a block per item where that many fit (4 per CU: 4 x 20.7 KB of LDS beside a straggler wave's 10, 16 waves of <= 96 registers)
  const uint64_t ready_max = (uint64_t)ctx->num_cu * (uint64_t)ctx->ready_blocks;
  f.accept1_blocks = f.ready_accept ? (unsigned)(acc_want > ready_max ? ready_max : acc_want) : f.accept_blocks;
  f.resolves_early = ctx->F.dir && ctx->F.touched && ctx->n_chunks >= 2 && !ctx->comm && !ctx->closest_deferred;
  // With accept_kernel<3> the frame's resolve does not wait for the first accept.  The whole frame is resolved behind the scan
  // -- the pixels' own sums are complete then, the HBM is idle and the solve waves do not need it --, the groups of pixels
  // the first accept's draws land in are resolved again behind it (about half of a headline frame's groups: 86 us where
  // the whole frame takes 130), the few groups of the last accept once more at the end.  (The accept behind the stragglers
  // has a few items, so the whole-frame resolve behind the first accept would be what the pass ends on.)
  f.resolve_after_scan = f.resolves_early && f.ready_accept;
  return f;
}

// ---- kernel arguments ----------------------------------------------------------------------------------------------------
static PublishArgs stream_publish_args(lentil_hip_ctx *ctx, const DrawArgs &seed, const StreamForm &f, const ScanPlan &plan) {
  const lentil_hip_ctx::Chunk &ch = ctx->chunks[0];
  PublishArgs pa{};
  pa.P = ctx->P; pa.V = ctx->V;
  StreamPub &pub = pa.S;
  pub.epoch = ctx->epoch;
  pub.n_channels = (uint32_t)f.nch;
  pub.retries = (int32_t)f.retries;
  pub.extra_num = ctx->est_sum_total < ctx->extra_below ? ctx->extra_num : 0u;
  pub.extra_const = ctx->est_sum_total < ctx->extra_below ? ctx->extra_const : 0u;
  pub.item_cap = (uint32_t)(ch.item_cap < 0xFFFFFFF0ull ? ch.item_cap : 0xFFFFFFF0ull);
  pub.task_cap = seed.task_cap;
  pub.pool_cap = seed.pool_cap;
  pub.hdr = ch.hdr; pub.prog = ch.prog; pub.active0 = ch.active[0]; pub.tasks0 = ch.tasks[0];
  if (f.predict && ctx->bm_valid) pub.model = batch_model_dev(ctx);        // (calibrated ahead of the scan)
  pa.ctr = ctx->d_ctr;
  pa.stuck_ticks = f.stuck_ticks;
  pa.work = ctx->d_work; pa.work_cap = ctx->V.n;
  pa.ranges = ctx->d_ranges; pa.range_cap = plan.sa.range_cap;
  pa.end_tasks = (f.a_blocks + f.b_blocks) * 4u;       // every first-round solve wave may hold one ticket past the last task
  return pa;
}

// what the pass's first kernels run with (A, the live straggler kernel); every later launch's arguments are made from these
static DrawArgs stream_base_args(lentil_hip_ctx *ctx, DrawArgs da, const StreamForm &f, const PublishArgs &pa) {
  da.stuck_ticks = f.stuck_ticks;
  da.ctr = ctx->d_ctr;
  da.retries = (int32_t)f.retries;
  da.work = ctx->d_work; da.work_cap = ctx->V.n;
  da.blind = 0u;
  da.n_items = pa.S.item_cap;
  da.parity = 0; da.round = 0; da.instance = 0;
  da.epoch = ctx->epoch;
  da.slow = f.slow_base;
  da.unknown_credit = ctx->unknown_credit;
  if (f.decoupled) { da.slow_indirect = 1; da.slow_cap = f.slow_cap_all / 2u > f.slow_waves_all ? f.slow_cap_all / 2u - f.slow_waves_all : 0u; }      // (its end markers stay below the upper half)
  da.slow_live = f.live ? 1 : 0;
  da.slow_dry_only = f.dry_only ? 1 : 0;
  // (the first round parks only once the scan has ended: 1 070 parked solves per headline pass instead of 2 486)
  da.slow_after_producers = 1;
  da.slow_waves = f.live ? f.slow_waves_all : 0u;
  da.producers_done = &ctx->d_ctr->publishers_done; da.producers_total = (uint32_t)ctx->publish_waves;
  da.item_ready = f.ready_accept ? 1 : 0;
  return da;
}
// ... the accept of round `round` (the coupled form's B and straggler launch: round 0)
static DrawArgs stream_round_args(DrawArgs d, const StreamForm &f, int round) {
  d.parity = round & 1; d.round = round;
  if (f.decoupled) {
    if (round >= 2) d.slow_cap = f.slow_cap_all;        // (round 1's accept still has both rounds' queue: the lower half)
  } else {
    d.instance = 1;                                     // behind the scan
    if (f.live && round >= 2) { d.producers_done = nullptr; d.producers_total = 0; }       // (its queues are complete when its kernels start)
  }
  return d;
}
// ... the first accept
static DrawArgs stream_first_accept_args(lentil_hip_ctx *ctx, const DrawArgs &base, const StreamForm &f) {
  DrawArgs d0 = f.decoupled ? base : stream_round_args(base, f, 0);
  d0.emit_live = (f.decoupled ? !f.lean_pass : f.overlap) ? 1 : 0;       // (lean tail: nobody is waiting for tasks)
  d0.lean_defer = f.lean_pass ? 1 : 0;
  d0.end_tasks = (uint32_t)ctx->num_cu * 4u;
  return d0;
}
// ... the second round's resident solves and their straggler kernel, beside or behind the first accept and fed by it
static DrawArgs stream_second_round_args(lentil_hip_ctx *ctx, const DrawArgs &base, const StreamForm &f) {
  DrawArgs d1 = stream_round_args(base, f, 1);
  d1.slow_after_producers = 0; d1.slow_indirect = 0;      // (its straggler kernel runs beside it from the start)
  d1.no_reset = 1;
  d1.producers_done = &ctx->d_ctr->accept_final[0]; d1.producers_total = 1u;      // (set behind the queue's end markers)
  if (f.decoupled) {                // (its parked solves go to the upper half of the records)
    d1.slow = f.slow_base + f.slow_cap_all / 2u;
    d1.slow_cap = f.slow_cap_all - f.slow_cap_all / 2u - d1.slow_waves;
  }
  return d1;
}
// ... a decoupled pass's later rounds' solves and stragglers: ordinary queues, complete when the kernels start
static DrawArgs stream_later_round_args(const DrawArgs &base, const StreamForm &f, int round) {
  DrawArgs d1 = stream_round_args(base, f, round);
  d1.slow_after_producers = 0; d1.slow_indirect = 0;
  d1.producers_done = nullptr; d1.producers_total = 0;
  return d1;
}
// ... what streamed_finish goes on from (StreamTail::da): the last round enqueued, one plain straggler queue per round
static DrawArgs stream_end_args(const DrawArgs &base, const StreamForm &f) {
  DrawArgs d = stream_round_args(base, f, f.blind_rounds >= 2 ? f.blind_rounds - 1 : 0);
  d.slow_indirect = 0; d.slow_cap = f.slow_cap_all;
  d.slow_live = 0;       // (rounds the host adds one by one park and finish their stragglers the plain way)
  return d;
}
// ... the lean tail's accept of the items that met parked solves: does nothing should the first accept have scheduled tasks
static DrawArgs stream_gated_accept_args(const DrawArgs &base, const StreamForm &f) {
  DrawArgs d2 = stream_end_args(base, f);
  d2.lean_gate = 1;
  return d2;
}

// ---- enqueue ---------------------------------------------------------------------------------------------------------------
// The head: the scan, the cryptomatte own-pixel adds, the publishers, the live straggler kernel, launch A.
static int stream_enqueue_head(lentil_hip_ctx *ctx, const StreamForm &f, const ScanPlan &plan, const PublishArgs &pa, const DrawArgs &base) {
  lentil_hip_ctx::Chunk &ch = ctx->chunks[0];
  int rc;
  // (the scan's start for lentil_hip_last_timing: the host work since the pass began -- sizing, the plan -- is not the kernel's)
  HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
  if ((rc = launch_scan(ctx, plan, ch, ctx->d_ctr, true))) return rc;
  ctx->last_scan_launches = 1;
  HIP_TRY(ctx, hipEventRecord(ch.scanned, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->scans_done, ctx->stream));
  // cryptomatte AOVs: the adds of the visits that stay in their pixel need the scan's work lists and nothing else of the
  // pass -- beside the draws, on the spare stream, where the runtime has one (LENTIL_CRYPTO_OVERLAP=0: after the pass)
  if (ctx->crypto && ctx->aux_stream && f.crypto_overlap) {
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->scans_done, 0));
    if ((rc = crypto_enqueue_direct(ctx, ctx->aux_stream))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_crypto, ctx->aux_stream));
    ctx->crypto_direct_enqueued = true;
  }
  // The publishers and A, resident beside the scan (the counters they poll were cleared by the memset ahead of
  // ev[0]).  Submitted AFTER what they wait for -- the scan, then the publishers: should the streams share a
  // hardware queue, each finds its producer ahead of it there.
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->pub_stream, ctx->ev[0], 0));
  hipLaunchKernelGGL(publish_kernel, dim3((unsigned)ctx->publish_waves), dim3(64), 0, ctx->pub_stream, pa);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->pub_done, ctx->pub_stream));
  if (f.live) {
    // (behind the publishers on their stream: they end with the scan, whose registers this kernel's waves need)
    hipLaunchKernelGGL(solve_slow_kernel, dim3(base.slow_waves), dim3(64), coop_lds_bytes(ctx->hlens.n_terms), ctx->pub_stream, base);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_slow, ctx->pub_stream));
  }
  HIP_TRY(ctx, hipStreamWaitEvent(ch.stream, ctx->ev[0], 0));
  launch_solve_po<true>(ctx, base, ch.stream, f.a_blocks);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ch.done, ch.stream));
  return LENTIL_OK;
}

// the resolve's last part behind the last accept enqueued blind (should the host have to add rounds, or redo the draws,
// lentil_hip_redistribute runs it once more)
static int stream_enqueue_late_resolve(lentil_hip_ctx *ctx, hipStream_t st) {
  if (!ctx->early_resolve_pending) return LENTIL_OK;
  HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_res, 0));
  const int rc = launch_resolve_half(ctx, st, 2u);
  if (!rc) ctx->late_resolve_done = true;
  return rc;
}

// ---- the decoupled pass with its chain of kernels laid along streams: a dependency that crosses streams costs
// 40-90 us (event, barrier packet, a queue waking up) where a kernel behind its predecessor on ONE stream costs ~2:
//   chunk stream : A -> first accept                      (the accept starts as the last first-round solve ends)
//   main stream  : scan -> second round's solves          (released by what the first accept waited for)
//   straggler st.: publishers -> stragglers of round one -> of round two -> second accept -> later rounds' accepts
//                  -> the resolve's second half -> counter read-back       (each behind the kernel it ends last)
// The only cross-stream waits left on the critical path release kernels that then sit waiting for tasks anyway.
// (Round 4: everything from the second round's stragglers on sits on THEIR stream -- the second accept follows the kernel
// that ends last, solve_slow_kernel of round two, in-stream; what else it needs -- the second round's solves, the first
// accept, the first round's stragglers -- has ended before that kernel does, so those waits find their events fired.
// On the publishers' stream the accept came ~60 us after the stragglers' end: three cross-stream waits in a row.)
// Its first accept, with the frame's early resolve around it; then one of the two tails below.
static int stream_enqueue_decoupled_accept(lentil_hip_ctx *ctx, const StreamForm &f, const DrawArgs &base) {
  lentil_hip_ctx::Chunk &ch = ctx->chunks[0];
  hipStream_t rs = ctx->chunks[1].stream;
  int rc;
  HIP_TRY(ctx, hipStreamWaitEvent(ch.stream, ctx->pub_done, 0));       // (both long past when A ends)
  HIP_TRY(ctx, hipStreamWaitEvent(ch.stream, ctx->scans_done, 0));
  HIP_TRY(ctx, hipEventRecord(ctx->ev_round, ch.stream));
  if (f.resolve_after_scan) {
    if (ctx->clear_pending) HIP_TRY(ctx, hipStreamWaitEvent(rs, ctx->ev_clear, 0));      // (it reads the accumulators clear_frame is wiping on the chunk stream)
    HIP_TRY(ctx, hipStreamWaitEvent(rs, ctx->scans_done, 0));
    if ((rc = launch_resolve_half(ctx, rs, 0u))) return rc;
  }
  const DrawArgs d0 = stream_first_accept_args(ctx, base, f);
  if (f.ready_accept) hipLaunchKernelGGL(accept_kernel<3>, dim3(f.accept1_blocks), dim3(256), 0, ch.stream, d0);
  else hipLaunchKernelGGL(accept_kernel<1>, dim3(f.accept1_blocks), dim3(256), 0, ch.stream, d0);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev_acc1, ch.stream));
  if (f.resolves_early) {
    HIP_TRY(ctx, hipStreamWaitEvent(rs, ctx->ev_acc1, 0));
    if ((rc = launch_resolve_half(ctx, rs, f.resolve_after_scan ? 1u : 0u))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_res, rs));
    ctx->early_resolve_pending = true;
  }
  return LENTIL_OK;
}

// Lean tail (first batches from the model): the first accept is expected to schedule nothing -- no second round's solve and
// straggler kernels, no waiting for them: the accept of the items that met parked solves follows the first accept on its
// stream, behind the first round's stragglers.  Should the first accept have scheduled tasks after all, that accept does
// nothing (DrawArgs::lean_gate) and the round is run by streamed_finish.
static int stream_enqueue_lean_tail(lentil_hip_ctx *ctx, const StreamForm &f, const DrawArgs &base, hipStream_t *tail) {
  hipStream_t ls = ctx->chunks[0].stream;
  HIP_TRY(ctx, hipStreamWaitEvent(ls, ctx->ev_slow, 0));      // the first round's stragglers
  hipLaunchKernelGGL(reset_round_kernel, dim3(1), dim3(1), 0, ls, ctx->d_ctr, 0u, 1u);
  hipLaunchKernelGGL(accept_kernel<2>, dim3(f.accept_blocks), dim3(256), 0, ls, stream_gated_accept_args(base, f));
  HIP_TRY(ctx, hipGetLastError());
  *tail = ls;
  return stream_enqueue_late_resolve(ctx, ls);
}

// The decoupled pass's rounds in flight: the second, fed by the first accept, then ordinary ones.
static int stream_enqueue_decoupled_tail(lentil_hip_ctx *ctx, const StreamForm &f, const DrawArgs &base, hipStream_t *tail) {
  hipStream_t ps = ctx->slow1_stream;
  // Round 5: the second round's resident solve and straggler kernels start BEHIND the first accept, not beside it.  Beside
  // it they were waiting -- holding registers and LDS -- for end markers that the accept's LAST block writes, and about one
  // such pass in 25 found only an eighth (or seven eighths) of the accept's blocks ever begun: whole XCDs' shares of the
  // grid stayed undispatched until the waiting waves gave up (250 ms, then the redo; lentil_hip_last_redo_note: "accept
  // blocks done 64 begun 64" of 512).  The blocks that did run had served every item, so nothing was wrong but the wait.
  // A kernel of a pass may spin only on kernels that hold all the resources they will ever need.  What this costs is the
  // head start of the second round's solves (~0.1 ms of a pass that has a second round at all; the lean tail has none).
  // Round 6: beside it again, by default.  Since the end markers of an emitting accept are written by the block that finishes
  // the pass's LAST ITEM (DevCounters::accept_items_done), not by the grid's last block, a share of the grid that is never
  // dispatched keeps nobody waiting; soaked with the dispatch probe's build armed (tools/sessions_r06/r06_session26.sh: 1 600
  // passes with a second round in flight -- config 5's bands, the headline without the first-batch model --, no stall, no
  // probe event; profiles/r06_overlap_accept_soak.txt) and worth 13 % of a config-5 band's pass.  LENTIL_OVERLAP_ACCEPT=0:
  // behind it.
  hipEvent_t go = f.overlap_accept ? ctx->ev_round : ctx->ev_acc1;
  const DrawArgs d1 = stream_second_round_args(ctx, base, f);
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, go, 0));
  launch_solve_po<true>(ctx, d1, ctx->stream, (unsigned)ctx->num_cu);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev_solve, ctx->stream));
  // (on a stream of its own: the first round's straggler kernel, ahead of everything on `ps`, is at work for another
  // ~0.25 ms -- its last records come when A ends -- and this round's parked solves need not wait for it)
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->slow1_stream, go, 0));
  hipLaunchKernelGGL(solve_slow_kernel, dim3(d1.slow_waves), dim3(64), coop_lds_bytes(ctx->hlens.n_terms), ctx->slow1_stream, d1);
  HIP_TRY(ctx, hipEventRecord(ctx->ev_slow1, ctx->slow1_stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ps, ctx->ev_slow, 0));      // the first round's stragglers (publishers' stream)
  HIP_TRY(ctx, hipStreamWaitEvent(ps, ctx->ev_solve, 0));
  HIP_TRY(ctx, hipStreamWaitEvent(ps, ctx->ev_acc1, 0));
  // (the first round's queues can go back to empty for what the accept below schedules; its result pool is still read)
  hipLaunchKernelGGL(reset_round_kernel, dim3(1), dim3(1), 0, ps, ctx->d_ctr, 0u, 1u);
  hipLaunchKernelGGL(accept_kernel<2>, dim3(f.accept_blocks), dim3(256), 0, ps, stream_round_args(base, f, 1));
  HIP_TRY(ctx, hipGetLastError());
  for (int round = 2; round < f.blind_rounds; ++round) {
    const DrawArgs dr = stream_later_round_args(base, f, round);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_round, ps));                   // behind the accept that filled this round's queues
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_round, 0));
    launch_solve_po<false>(ctx, dr, ctx->stream, (unsigned)ctx->num_cu);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_solve, ctx->stream));
    hipLaunchKernelGGL(solve_slow_kernel, dim3(dr.slow_waves), dim3(64), coop_lds_bytes(ctx->hlens.n_terms), ps, dr);      // beside the round's solves
    HIP_TRY(ctx, hipStreamWaitEvent(ps, ctx->ev_solve, 0));
    hipLaunchKernelGGL(accept_kernel<0>, dim3(f.accept_blocks), dim3(256), 0, ps, stream_round_args(base, f, round));
    HIP_TRY(ctx, hipGetLastError());
  }
  *tail = ps;
  return stream_enqueue_late_resolve(ctx, ps);
}

// The coupled pass: B, the first round's stragglers, the accepts and the later rounds on the main stream.
static int stream_enqueue_coupled_tail(lentil_hip_ctx *ctx, const StreamForm &f, const DrawArgs &base, hipStream_t *tail) {
  lentil_hip_ctx::Chunk &ch = ctx->chunks[0];
  int rc;
  if ((rc = join_clear(ctx))) return rc;       // (this form's accepts are on the main stream)
  // B: the rest of the CUs' room, once the scan's waves have left
  const DrawArgs db = stream_round_args(base, f, 0);
  if (f.b_blocks) launch_solve_po<true>(ctx, db, ctx->stream, f.b_blocks);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ch.done, 0));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->pub_done, 0));
  if (f.live) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_slow, 0));
  else launch_slow(ctx, db, ctx->stream);
  if (f.overlap) HIP_TRY(ctx, hipEventRecord(ctx->ev_round, ctx->stream));      // everything the first accept waits for
  hipLaunchKernelGGL(accept_kernel<0>, dim3(f.accept_blocks), dim3(256), 0, ctx->stream, stream_first_accept_args(ctx, base, f));
  HIP_TRY(ctx, hipGetLastError());
  // The frame's resolve, first half: behind the first accept, beside the second round's solves (one block per CU, no
  // HBM traffic to speak of) on the otherwise idle second chunk stream.  What later accepts add lands in groups of
  // pixels whose `touched` flag is set by then: lentil_hip_redistribute resolves those once more at its end.
  if (f.resolves_early) {
    hipStream_t rs = ctx->chunks[1].stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_acc1, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(rs, ctx->ev_acc1, 0));
    if ((rc = launch_resolve_half(ctx, rs, 0u))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_res, rs));
    ctx->early_resolve_pending = true;
  }
  for (int round = 1; round < f.blind_rounds; ++round) {
    const DrawArgs da = stream_round_args(base, f, round);
    if (f.overlap && round == 1) {
      // The second round's resident solves beside the first accept, released by what that accept itself waited for, fed by
      // its tagged task slots and closed by its last block's end markers.  With a live queue the round's stragglers beside
      // them: the straggler kernel on the publishers' stream, released likewise; this round's accept waits for both.
      const DrawArgs d1 = stream_second_round_args(ctx, base, f);
      HIP_TRY(ctx, hipStreamWaitEvent(ch.stream, ctx->ev_round, 0));
      launch_solve_po<true>(ctx, d1, ch.stream, (unsigned)ctx->num_cu);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipEventRecord(ch.done, ch.stream));
      if (f.live) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->pub_stream, ctx->ev_round, 0));
        hipLaunchKernelGGL(solve_slow_kernel, dim3(d1.slow_waves), dim3(64), coop_lds_bytes(ctx->hlens.n_terms), ctx->pub_stream, d1);
        HIP_TRY(ctx, hipEventRecord(ctx->ev_slow, ctx->pub_stream));
      }
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ch.done, 0));
      if (f.live) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_slow, 0));
      // (the first accept and this round's solves are done: the first round's queues can go back to empty for what
      // the accept below schedules)
      hipLaunchKernelGGL(reset_round_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->d_ctr, 0u, 0u);
    } else if (f.live) {
      // the round's stragglers beside its solves: the straggler kernel on the other stream, released by the accept
      // before it; this round's accept waits for both
      HIP_TRY(ctx, hipEventRecord(ctx->ev_round, ctx->stream));
      launch_solve_po<false>(ctx, da, ctx->stream, (unsigned)ctx->num_cu);
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->pub_stream, ctx->ev_round, 0));
      hipLaunchKernelGGL(solve_slow_kernel, dim3(da.slow_waves), dim3(64), coop_lds_bytes(ctx->hlens.n_terms), ctx->pub_stream, da);
      HIP_TRY(ctx, hipEventRecord(ctx->ev_slow, ctx->pub_stream));
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_slow, 0));
    } else {
      launch_solve(ctx, da, ctx->stream, (unsigned)ctx->num_cu);
    }
    hipLaunchKernelGGL(accept_kernel<0>, dim3(f.accept_blocks), dim3(256), 0, ctx->stream, da);
    HIP_TRY(ctx, hipGetLastError());
  }
  *tail = ctx->stream;
  return stream_enqueue_late_resolve(ctx, ctx->stream);
}

// ---- the end: left to whoever observes the context next, or awaited here ---------------------------------------------------
static int stream_end(lentil_hip_ctx *ctx, DeviceTurn &turn, StreamTail &t, bool *streamed, bool *deferred) {
  hipStream_t tail = t.tail;
  ht_mark(ctx, "all_launched");
  ctx->clear_pending = false;       // (every stream of the pass is behind the wipe by now, and the main stream will be behind the pass)
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_ctr_pinned, ctx->d_ctr, sizeof(DevCounters) * ctx->n_chunks, hipMemcpyDeviceToHost, tail));
  // The asynchronous end (lentil_hip_ctx::async_end): the lean tail is the pass that expects to have nothing left to do, and the
  // frame takes nothing but gaussian splats (closest-filtered AOVs, lentil_debug and cryptomatte have host steps behind the pass).
  // Everything of the pass is behind `tail` by now (the lean tail's accepts wait for the scan, the publishers, the stragglers
  // and the early resolve); the context's own stream waits for it in turn, so whatever the caller enqueues next follows the pass.
  const bool defer = ctx->async_end && t.lean && !ctx->crypto && !ctx->F.zkey && !ctx->F.zkey_dbg &&
                     !ctx->comm && !ctx->closest_deferred && !t.inject && !host_trace_passes() && ctx->inflight.size() < 2;
  if (defer) {
    lentil_hip_ctx::Slot &sl = ctx->slots[ctx->slot];
    HIP_TRY(ctx, hipEventRecord(sl.ev_tail, tail));
    if (tail != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, sl.ev_tail, 0));
    t.deferred = true;
    lentil_hip_ctx::Inflight in;
    in.slot = ctx->slot; in.t = t; in.V = ctx->V; in.have_visits = ctx->have_visits;
    ctx->inflight.push_back(in);
    turn.keep();                  // (the device's turn stays this context's until the pass has been looked at)
    ctx->last_streamed = 1;
    ++ctx->last_blind;
    *deferred = true;
    *streamed = true;
    return LENTIL_OK;
  }
  HIP_TRY(ctx, hipStreamSynchronize(tail));
  ht_mark(ctx, "tail_synced");
  // everything the pass enqueued anywhere is behind the read-back that has just arrived; what the caller enqueues on
  // the context's stream next (resolve, downloads, the next pass) follows the main stream's own last kernel
  if (tail != ctx->stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ht_mark(ctx, "main_synced");
  // (host time from the pass's first launch to its counters: an upper bound of every wait inside it)
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t.pass_t0).count();
  if (!t.calibrates_now && ms > ctx->longest_pass_ms && ms < 200.0) {
    ctx->longest_pass_ms = ms; ctx->longest_pass_visits = ctx->V.n; ctx->longest_pass_sum = ctx->est_sum_total;
  }
  ++ctx->last_blind;
  return streamed_finish(ctx, t, ctx->h_ctr_pinned, true, streamed);
}

static int redistribute_streamed(lentil_hip_ctx *ctx, bool *streamed, bool *deferred) {
  *streamed = false;
  *deferred = false;
  DeviceTurn turn(ctx);
  DrawArgs seed{};
  uint64_t items = 0, units = 0;
  if (!stream_pass_applies(ctx, turn, seed, items, units)) return LENTIL_OK;
  ScanPlan plan;
  int rc;
  if ((rc = stream_prepare(ctx, seed, items, units, plan))) return rc;
  StreamTail t;
  t.pass_t0 = std::chrono::steady_clock::now();
  ht_mark(ctx, "first_launch");
  // the first-batch model's calibration, should the camera set-up have changed: on the main stream, ahead of the event the
  // publishers (who read the table) wait for -- and ahead of the form, which asks whether there is a model
  const bool calibrates_now = ctx->predict && !ctx->bm_valid;
  if (ctx->predict && seed.n_channels == 1 && (rc = ensure_batch_model(ctx))) return rc;
  const StreamForm f = make_stream_form(ctx, seed, plan, calibrates_now);
  const PublishArgs pa = stream_publish_args(ctx, seed, f, plan);
  const DrawArgs base = stream_base_args(ctx, seed, f, pa);
  if ((rc = stream_enqueue_head(ctx, f, plan, pa, base))) return rc;
  if (f.decoupled) {
    if ((rc = stream_enqueue_decoupled_accept(ctx, f, base))) return rc;
    rc = f.lean_pass ? stream_enqueue_lean_tail(ctx, f, base, &t.tail) : stream_enqueue_decoupled_tail(ctx, f, base, &t.tail);
  } else {
    rc = stream_enqueue_coupled_tail(ctx, f, base, &t.tail);
  }
  if (rc) return rc;
  t.calibrates_now = f.calibrates_now; t.predicted = f.predicted; t.lean = f.lean_pass; t.live = f.live; t.inject = f.inject;
  t.blind_rounds = f.blind_rounds; t.da = stream_end_args(base, f); t.slow_base = f.slow_base; t.slow_cap_all = f.slow_cap_all;
  t.accept_blocks = f.accept_blocks; t.item_cap = pa.S.item_cap; t.task_cap = pa.S.task_cap; t.range_cap = plan.sa.range_cap;
  t.pool_cap = pa.S.pool_cap; t.stuck_ticks = f.stuck_ticks;
  return stream_end(ctx, turn, t, streamed, deferred);
}
