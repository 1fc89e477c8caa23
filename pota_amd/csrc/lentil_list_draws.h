// lentil_list_draws.h -- two queries over the context's bound visit stream, for a renderer that keeps its own film
// (lentil_hip_plan_visits, lentil_hip_list_draws): what the visit prologue decides per visit (src/lentil_filter.cpp:105-240),
// and the accepted draws of a visit range -- the first `samples` attempts among 0 ... 5 * samples - 1 that get through the lens
// and land in the frame (the loops of src/lentil_filter.cpp:249-300 and :311-447) -- with their continuous pixel coordinates.
// No frame, no accumulators, no counter block, no xor128 state, no probes; no existing kernel changes.
//
// plan_visits_kernel.  One lane per visit, 64 consecutive visits per wave and step (the five 16-byte columns are read
// coalesced), grid-stride over such groups; visit_prologue and visit_pixel are the pass's own (load_work_visit), the weight
// is formed as load_work_visit and the scan form it.  A 32-byte record per lane.  The totals are counted by ballot and
// __popcll (the samples by a shuffle reduction) into wave-uniform sums: one atomic per wave and total, at the end.
//
// list_draws_kernel.  A wave takes 64 consecutive visits on a dynamic ticket (one atomic per 64 visits), runs the prologue
// with lane = visit, ballots the redistribute decisions and then serves the set lanes one after another: the visit's position,
// pixel and draw count are handed to the whole wave through readlane (scalar registers), and the wave walks the visit's
// attempts 64 at a time with lane = attempt.  A slab is traced with trace_points_kernel's loops, operation for operation (the
// wave-uniform vignetting-retry loop, the per-lane Newton loop; the same device functions), its successes are balloted, and a
// success is taken while accepted_so_far + popcount(ballot & lower lanes) < samples -- the attempts the reference's loop
// would have accepted before it stopped.  The slab's records take consecutive slots of the list through one atomic
// (probe_wave_slot's pattern on a 64-bit counter) and are written where the slot lies below the capacity; the counter runs on,
// so the caller learns how many there are.  The attempts a visit made -- up to its last accepted draw if that was the
// `samples`-th, else all 5 * samples -- are summed per wave: one atomic per 64 visits.
// Every loop is bounded: ceil(n_visits / 64) tickets, at most 64 visits per ticket, at most ceil(5 * samples / 64) slabs per
// visit, at most vignetting_retries + 1 tries, at most 100 Newton iterations (newton_continue).
// What a record holds depends on its (visit, attempt) alone, so the list as a set does not depend on the grid, on the
// capacity or on how the stream is split into ranges; the order of the records does.
#pragma once
#include "lentil_kernels.h"

constexpr int kLdBlock = 256;
constexpr uint32_t kLdSlab = 64;    // attempts per slab = visits per ticket = lanes per wave

struct PlanArgs {
  lentil_params P;
  VisitsDev V;
  double lens_length;
  uint64_t v_begin, v_end;
  lentil_visit_plan *out;
  unsigned long long *totals;       // optional [3]: visits, redistributed visits, the sum of their samples
};

LD_DEV float plan_weight(float invd, bool redistribute, int samples) {
  if (!redistribute) return 1.0f * invd;                                  // filter_weight * inv_density, lentil.h:949-953
  const float inv_samples = (float)(1.0 / (double)(float)samples);
  return 1.0f * invd * inv_samples;                                       // src/lentil_filter.cpp:297
}

__global__ __launch_bounds__(kLdBlock) void plan_visits_kernel(PlanArgs a) {
  const VisitsDev &V = a.V;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kLdBlock / 64) + (threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kLdBlock / 64);
  const uint64_t n_groups = (a.v_end - a.v_begin + 63u) / 64u;
  unsigned long long n_visits = 0, n_red = 0, sum_samples = 0;             // the first two wave-uniform, the third per lane
  for (uint64_t g = wave; g < n_groups; g += waves) {
    const uint64_t v = a.v_begin + g * 64u + lane;
    const bool valid = v < a.v_end;
    bool red = false;
    if (valid) {
      const float invd = V.inv_density ? V.inv_density[v] : a.P.inverse_sample_density;
      const VisitInfo I = visit_prologue(a.P, a.lens_length, V.rgba[v], V.pos_z[v], V.raydir_time[v], V.volume_ignore[v],
                                         V.transmission[v], invd, V.cam);
      int px, py;
      visit_pixel(V, v, px, py);
      red = I.redistribute;
      lentil_visit_plan r;
      r.cs[0] = I.cs[0]; r.cs[1] = I.cs[1]; r.cs[2] = I.cs[2];
      r.add_energy = red ? I.add_energy : 0.0f;
      r.weight = plan_weight(invd, red, I.samples);
      r.samples = (uint32_t)I.samples;
      r.pixel = (uint32_t)((px & 0xFFFF) | (py << 16));
      r.flags = red ? LENTIL_PLAN_REDISTRIBUTE : 0u;
      a.out[v - a.v_begin] = r;
      if (red) sum_samples += (unsigned long long)(uint32_t)I.samples;
    }
    n_visits += (unsigned long long)__popcll(__ballot(valid));
    n_red += (unsigned long long)__popcll(__ballot(red));
  }
  if (a.totals) {
    for (int off = 32; off > 0; off >>= 1) sum_samples += __shfl_down(sum_samples, off);
    if (lane == 0u) {
      if (n_visits) atomicAdd(&a.totals[0], n_visits);
      if (n_red) atomicAdd(&a.totals[1], n_red);
      if (sum_samples) atomicAdd(&a.totals[2], sum_samples);
    }
  }
}

struct ListDrawArgs {
  lentil_params P;
  VisitsDev V;
  double lens_length;
  const DevLens *lens;              // polynomial optics only
  const DevTerm *terms;
  DevBokeh bokeh;
  uint64_t v_begin, v_end;
  uint64_t capacity;
  lentil_draw *out;
  double lambda;
  unsigned long long *ctr;          // [0] the ticket, [1] accepted draws (the list's counter), [2] attempts made
};

LD_DEV uint32_t ld_readlane(uint32_t x, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)x, src); }
LD_DEV float ld_readlane(float x, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src)); }
LD_DEV unsigned long long ld_readlane(unsigned long long x, int src) {
  return (unsigned long long)ld_readlane((uint32_t)x, src) | ((unsigned long long)ld_readlane((uint32_t)(x >> 32), src) << 32);
}

// One wave's wanted lanes take consecutive slots of the list: one atomic per wave (probe_wave_slot, on a 64-bit counter).
// Called by the whole wave, wmask != 0.
LD_DEV unsigned long long list_wave_slot(unsigned long long *count, unsigned long long wmask, uint32_t lane) {
  const int first = __builtin_ctzll(wmask);
  unsigned long long base = 0;
  if ((int)lane == first) base = atomicAdd(count, (unsigned long long)__builtin_popcountll(wmask));
  base = ld_readlane(base, first);
  return base + (unsigned long long)__builtin_popcountll(wmask & ((1ull << lane) - 1ull));
}

// LensT / kTables / PO: as trace_points_kernel (LdsLens with the term table staged into LDS, the interpreter -- also the thin
// lens's, which has no lens: PO false -- or GenLens<Gen> of a compiled-in lens).
template <class LensT, bool kTables, bool PO>
__global__ __launch_bounds__(kLdBlock) void list_draws_kernel(ListDrawArgs a) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  if (PO) {
    if (kTables) {
      const uint32_t nt = a.lens->n_terms;
      for (uint32_t i = threadIdx.x; i < nt; i += kLdBlock) s_terms[i] = a.terms[i];
    }
    if (threadIdx.x == 0) {
      s_k = *a.lens;
      s_k.lambda_pow[0] = 1.0; s_k.lambda_pow[1] = a.lambda;
      for (uint32_t e = 2; e <= kMaxExp; ++e) s_k.lambda_pow[e] = ipow_u(a.lambda, e);     // lens_ipow, like the host
    }
    __syncthreads();
  }
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = &s_k;
  const lentil_params &P = a.P;
  const VisitsDev &V = a.V;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long n_groups = (a.v_end - a.v_begin + 63u) / 64u;
  const double qnan = __builtin_nan("");
  for (;;) {
    unsigned long long g = 0;
    if (lane == 0u) g = atomicAdd(&a.ctr[0], 1ull);
    g = ld_readlane(g, 0);
    if (g >= n_groups) break;
    // ---- the prologue, lane = visit
    const uint64_t v = a.v_begin + g * 64u + lane;
    VisitInfo I{};
    int vpx = 0, vpy = 0;
    if (v < a.v_end) {
      const float invd = V.inv_density ? V.inv_density[v] : P.inverse_sample_density;
      I = visit_prologue(P, a.lens_length, V.rgba[v], V.pos_z[v], V.raydir_time[v], V.volume_ignore[v], V.transmission[v], invd, V.cam);
      visit_pixel(V, v, vpx, vpy);
    } else {
      I.redistribute = false;
    }
    unsigned long long todo = __ballot(I.redistribute);
    unsigned long long wave_attempts = 0;
    // ---- the set lanes one after another, lane = attempt
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const float cs[3] = {ld_readlane(I.cs[0], src), ld_readlane(I.cs[1], src), ld_readlane(I.cs[2], src)};
      const int px = (int)ld_readlane((uint32_t)vpx, src), py = (int)ld_readlane((uint32_t)vpy, src);
      const uint32_t samples = ld_readlane((uint32_t)I.samples, src);
      const uint32_t visit = (uint32_t)(a.v_begin + g * 64u) + (uint32_t)src;
      const uint32_t max_total = samples * 5u;                           // unsigned, as the reference's max_total_samples
      uint32_t accepted = 0, made = 0;
      for (uint32_t k0 = 0; k0 < max_total && accepted < samples; k0 = (max_total - k0 > kLdSlab) ? k0 + kLdSlab : max_total) {
        const uint32_t attempt = k0 + lane;
        const bool commit = max_total - k0 > lane;                      // attempt < max_total, without the sum's wrap

        uint32_t code = LENTIL_POINT_VIGNETTED;
        double xy0 = qnan, xy1 = qnan;
        int tries = 0;
        if (PO) {
          const DevLens &k = L.consts();
          const double target[3] = {-(double)cs[0] * 10.0, -(double)cs[1] * 10.0, -(double)cs[2] * 10.0};   // src/lentil_filter.cpp:271
          bool ok = false;
          bool trying = commit && tries <= P.vignetting_retries;
          double sensor[4] = {0.0, 0.0, 0.0, 0.0};
          while (__any(trying)) {
            double ax, ay;
            po_aperture_sample(P, a.bokeh, a.bokeh.cdfRow, (uint32_t)(px * py + px), attempt + (uint32_t)tries, ax, ay);
            NewtonState s;
            newton_init(s);
            while (trying && newton_continue(s)) newton_iter(L, target, ax, ay, s);
            double out4;
            const float transmittance = (float)newton_finish(L, s, out4);
            bool pass = !(transmittance <= 0);
            const double ipx = s.x + s.dx * k.back_focal_length;
            const double ipy = s.y + s.dy * k.back_focal_length;
            if (ipx * ipx + ipy * ipy > k.inner_pupil_radius * k.inner_pupil_radius) pass = false;
            if (trying) {
              if (pass) {
                sensor[0] = s.x; sensor[1] = s.y; sensor[2] = s.dx; sensor[3] = s.dy;
                ok = true; trying = false;
              } else {
                ++tries; trying = tries <= P.vignetting_retries;
              }
            }
          }
          if (ok) {
            const double sen0 = sensor[0] + sensor[2] * -P.sensor_shift;
            const double sen1 = sensor[1] + sensor[3] * -P.sensor_shift;
            uint32_t pn = 0;
            code = po_sensor_to_pixel_xy(P, sen0, sen1, pn, xy0, xy1) ? pn : LENTIL_POINT_OUTSIDE;
          }
        } else if (commit) {
          TlRay ray;
          if (thinlens_ray(P, a.bokeh, a.bokeh.cdfRow, cs, px, py, attempt, ray)) {
            const float image_dist_focusdist =
                (float)(((double)-P.focal_length * -P.focus_distance) / ((double)-P.focal_length + -P.focus_distance));
            uint32_t pn = 0;
            float fx, fy;
            code = thinlens_project_xy(P, ray, image_dist_focusdist, pn, fx, fy) ? pn : LENTIL_POINT_OUTSIDE;
            xy0 = (double)fx; xy1 = (double)fy;
          }
        }

        // ---- the reference's selection: the successes in attempt order, until `samples` of them are in
        const bool success = commit && code < LENTIL_POINT_OUTSIDE;
        const unsigned long long okm = __ballot(success);
        const bool take = success && accepted + (uint32_t)__builtin_popcountll(okm & below) < samples;
        const unsigned long long tm = __ballot(take);
        const uint32_t nt = (uint32_t)__builtin_popcountll(tm);
        if (tm) {
          const unsigned long long slot = list_wave_slot(&a.ctr[1], tm, lane);
          if (take && slot < a.capacity) {
            lentil_draw r;
            r.visit = visit; r.attempt = attempt; r.pixel = code; r.tries = tries;
            r.xy[0] = xy0; r.xy[1] = xy1;
            a.out[slot] = r;
          }
        }
        accepted += nt;
        // (the loop ends behind its `samples`-th accepted draw; a slab without it was attempted to its end)
        if (accepted >= samples) made = k0 + (uint32_t)(63 - __builtin_clzll(tm)) + 1u;
        else made = (max_total - k0 > kLdSlab) ? k0 + kLdSlab : max_total;
      }
      wave_attempts += made;
    }
    if (lane == 0u && wave_attempts) atomicAdd(&a.ctr[2], wave_attempts);
  }
}
