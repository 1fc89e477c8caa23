// lentil_trace_points.h -- scene points traced backward through the lens in batches (lentil_hip_trace_points): for a
// camera-space point and an attempt number, where on the sensor a draw of the redistribution pass would put it --
// Camera::trace_ray_bw_po (src/lentil.h:573-661) and the sensor -> pixel mapping of src/lentil_filter.cpp:271-290 for
// polynomial optics, the thin-lens draw of src/lentil_filter.cpp:311-434 (abb_chromatic == 0) for the thin lens.  The
// backward counterpart of lentil_camera_rays.h: no frame, no visits, no accumulators, no probes.
//
// Mapping.  A query is (point, attempt); a point's K attempts are consecutive.  A wave takes one slab -- one point and 64
// consecutive attempts of it -- so the point's position, source pixel and first attempt are wave-uniform (read once, through
// scalar registers) and lane = attempt: every output array is written lane-contiguous.  The lanes of a point's last slab
// that lie beyond K do not try and commit nothing.  Slabs are walked in a grid-stride loop; the host bounds the grid by the
// CU count.
//
// Convergence.  The table interpreter reads a term's exponents through readfirstlane, so the vignetting-retry loop is
// wave-uniform: it runs while ANY lane of the wave still tries, and a lane that is done keeps the values it has.  The Newton
// loop inside a try ends per lane, as in focus_miss_kernel and camera_rays_kernel (every lane reads the same term, so what
// readfirstlane returns is right for whichever lanes still iterate); a lane that no longer tries does not enter it.  Both
// loops are bounded: at most vignetting_retries + 1 tries, at most 100 Newton iterations (newton_continue).  A compiled-in
// lens (GenLens<Gen>) runs the same loops over straight-line polynomials.
//
// trace_attempt is that trace of one attempt, and the only one: trace_points_kernel calls it once per slab, and so do the
// list kernels of lentil_list_draws.h (list_draws_kernel, list_draws_probed_kernel; list_draws_chroma_kernel once per colour
// channel).  What the probed list adds -- answers about the seeds -- comes in as a policy, NoSeedAnswers for everybody else.
#pragma once
#include "lentil_kernels.h"

constexpr int kTpBlock = 256;
constexpr uint32_t kTpSlab = 64;    // attempts per slab = lanes per wave

struct TracePointArgs {
  lentil_params P;
  const DevLens *lens;            // polynomial optics only
  const DevTerm *terms;
  DevBokeh bokeh;
  uint32_t n_slabs;               // n_points * slabs_per_point (< 2^32: n_points * attempts is)
  uint32_t slabs_per_point;       // ceil(attempts / 64)
  uint32_t attempts;
  const float *cs;                // [n_points][3]
  const uint32_t *pixel;          // [n_points] px | py << 16
  const uint32_t *first_attempt;  // optional [n_points]
  double lambda;
  uint32_t *out_pixel;            // [n_points * attempts]
  double *out_xy;                 // optional [n_points * attempts][2]
  double *out_sensor;             // optional [n_points * attempts][2], polynomial optics
  int32_t *out_tries;             // optional [n_points * attempts]
};

// The seed answers of a trace that no occlusion probe watches: no seed is occluded, every answer is known.  (The probed
// list's policy is SeedAnswers, lentil_list_draws.h.)
struct NoSeedAnswers {
  LD_DEV void look(uint32_t, bool &occluded, bool &known) const { occluded = false; known = true; }
};

struct AttemptTrace {
  uint32_t code;          // the pixel, LENTIL_POINT_OUTSIDE or LENTIL_POINT_VIGNETTED
  double xy0, xy1;        // the continuous pixel position (NaN where there is none)
  double sen0, sen1;      // polynomial optics: the sensor position
  int tries;              // the failed tries; the passing try's seed is attempt + tries
  // for a caller whose seeds have answers: the passing seed's answer is not known yet, and that try's aperture point
  bool open;
  float lx, ly;
};

// One attempt of a draw traced backward, by a whole wave (lane = attempt; a lane that does not `commit` neither tries nor
// looks anything up and comes back LENTIL_POINT_VIGNETTED).  Polynomial optics: the wave-uniform vignetting-retry loop, the
// per-lane Newton loop, the inner-pupil test, then sensor -> pixel (see Convergence above).  Thin lens: thinlens_ray and
// thinlens_project_xy.  `seeds` answers for seed m = attempt + try: a try at an occluded seed fails without a solve (thin
// lens: the attempt is lost), a pass at a seed whose answer is not known comes back `open`.  With NoSeedAnswers `solve` is
// `trying`, and `if (!solve) pass = false` touches only lanes whose `pass` nobody reads.
template <bool PO, class LensT, class Seeds>
LD_DEV AttemptTrace trace_attempt(const lentil_params &P, const LensT &L, const DevBokeh &bokeh, const float cs[3], int px, int py,
                                  uint32_t attempt, bool commit, const Seeds &seeds) {
  const double qnan = __builtin_nan("");
  AttemptTrace r;
  r.code = LENTIL_POINT_VIGNETTED;
  r.xy0 = qnan; r.xy1 = qnan; r.sen0 = qnan; r.sen1 = qnan;
  r.tries = 0;
  r.open = false; r.lx = 0.f; r.ly = 0.f;
  if (PO) {
    const DevLens &k = L.consts();
    const double target[3] = {-(double)cs[0] * 10.0, -(double)cs[1] * 10.0, -(double)cs[2] * 10.0};   // src/lentil_filter.cpp:271
    bool ok = false;
    bool trying = commit && r.tries <= P.vignetting_retries;
    double sensor[4] = {0.0, 0.0, 0.0, 0.0};
    while (__any(trying)) {
      const uint32_t m = attempt + (uint32_t)r.tries;
      bool occluded = false, known = true;
      if (trying) seeds.look(m, occluded, known);
      const bool solve = trying && !occluded;
      double ax, ay;
      po_aperture_sample(P, bokeh, bokeh.cdfRow, (uint32_t)(px * py + px), m, ax, ay);
      NewtonState s;
      newton_init(s);
      while (solve && newton_continue(s)) newton_iter(L, target, ax, ay, s);
      double out4;
      const float transmittance = (float)newton_finish(L, s, out4);
      bool pass = !(transmittance <= 0);
      const double ipx = s.x + s.dx * k.back_focal_length;
      const double ipy = s.y + s.dy * k.back_focal_length;
      if (ipx * ipx + ipy * ipy > k.inner_pupil_radius * k.inner_pupil_radius) pass = false;
      if (!solve) pass = false;
      if (trying) {
        if (pass) {
          sensor[0] = s.x; sensor[1] = s.y; sensor[2] = s.dx; sensor[3] = s.dy;
          ok = true; trying = false;
          if (!known) { r.open = true; r.lx = (float)(-ax * 0.1); r.ly = (float)(-ay * 0.1); }   // src/lentil.h:614
        } else {
          ++r.tries; trying = r.tries <= P.vignetting_retries;
        }
      }
    }
    if (ok) {
      r.sen0 = sensor[0] + sensor[2] * -P.sensor_shift;
      r.sen1 = sensor[1] + sensor[3] * -P.sensor_shift;
      uint32_t pn = 0;
      r.code = po_sensor_to_pixel_xy(P, r.sen0, r.sen1, pn, r.xy0, r.xy1) ? pn : LENTIL_POINT_OUTSIDE;
    }
  } else if (commit) {
    TlRay ray;
    if (thinlens_ray(P, bokeh, bokeh.cdfRow, cs, px, py, attempt, ray)) {
      bool occluded = false, known = true;
      seeds.look(attempt, occluded, known);
      if (!occluded) {                                              // (an occluded attempt is lost)
        const float image_dist_focusdist =
            (float)(((double)-P.focal_length * -P.focus_distance) / ((double)-P.focal_length + -P.focus_distance));
        uint32_t pn = 0;
        float fx, fy;
        r.code = thinlens_project_xy(P, ray, image_dist_focusdist, pn, fx, fy) ? pn : LENTIL_POINT_OUTSIDE;
        r.xy0 = (double)fx; r.xy1 = (double)fy;
        if (!known) { r.open = true; r.lx = ray.lx; r.ly = ray.ly; }
      }
    }
  }
  return r;
}

// LensT / kTables: LdsLens with the term table staged into LDS (the interpreter; also the thin lens's, which has no lens: PO
// false), or GenLens<Gen> of a compiled-in lens -- only the header and the lambda powers in LDS.
template <class LensT, bool kTables, bool PO>
__global__ __launch_bounds__(kTpBlock) void trace_points_kernel(TracePointArgs a) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  if (PO) {
    stage_lens<kTables>(a.lens, a.terms, a.lambda, kTpBlock, s_terms, &s_k, threadIdx.x == 0);
    __syncthreads();
  }
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = &s_k;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * (kTpBlock / 64);
  // (slab < n_slabs - waves before the step: the sum cannot wrap)
  for (uint32_t slab = blockIdx.x * (kTpBlock / 64) + wave; slab < a.n_slabs; slab = (a.n_slabs - slab > waves) ? slab + waves : a.n_slabs) {
    const uint32_t point = slab / a.slabs_per_point;
    const uint32_t k0 = (slab - point * a.slabs_per_point) * kTpSlab;
    const float cs[3] = {a.cs[(size_t)point * 3], a.cs[(size_t)point * 3 + 1], a.cs[(size_t)point * 3 + 2]};
    const uint32_t pix = a.pixel[point];
    const int px = (int)(pix & 0xFFFFu), py = (int)(pix >> 16);
    const uint32_t attempt = (a.first_attempt ? a.first_attempt[point] : 0u) + k0 + lane;
    const bool commit = k0 + lane < a.attempts;
    const uint64_t q = (uint64_t)point * a.attempts + k0 + lane;
    const AttemptTrace t = trace_attempt<PO>(a.P, L, a.bokeh, cs, px, py, attempt, commit, NoSeedAnswers{});
    if (commit) {
      a.out_pixel[q] = t.code;
      if (a.out_xy) { a.out_xy[q * 2] = t.xy0; a.out_xy[q * 2 + 1] = t.xy1; }            // (the caller's arrays are 8-byte aligned, no more)
      if (a.out_sensor) { a.out_sensor[q * 2] = t.sen0; a.out_sensor[q * 2 + 1] = t.sen1; }
      if (a.out_tries) a.out_tries[q] = t.tries;
    }
  }
}

// lentil_hip_trace_points_spectral: point j at lambdas[j] (0: a.lambda, which the host sets to params.lambda_bw), polynomial
// optics.  trace_points_kernel's slab loop line for line (a kernel of its own, not a parameter of that one: the scalar call's
// code stays what it is) with the staging of the wavelength in front.  A wave traces one point at a time, so the wavelength is
// wave-uniform: every wave keeps the lambda powers of its point in a row of LDS of its own (LensT = LdsLensAt<LambdaTable> or
// GenLensAt<Gen>; the block shares the header's constants alone) and rewrites the row when its next slab belongs to another
// point.  The waves of a block make different numbers of trips through the loop, so nothing in it may wait for the block.
// Nothing has to: the row is the wave's own, written by its lanes 0 ... kMaxExp and read by all of them, and LDS serves a
// wave's accesses in the order it issues them.  What is needed is that the compiler keeps the reads of the last slab, the
// writes, and the reads of this slab in that order; the two wave-scope fences say so (DESIGN.md 4.7 has what the loop compiles
// to).
template <class LensT, bool kTables>
__global__ __launch_bounds__(kTpBlock) void trace_points_spectral_kernel(TracePointArgs a, const double *lambdas) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  __shared__ double s_lp[kTpBlock / 64][kMaxExp + 1];
  stage_lens<kTables>(a.lens, a.terms, a.lambda, kTpBlock, s_terms, &s_k, threadIdx.x == 0);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * (kTpBlock / 64);
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = &s_k;
  L.lam.lp = s_lp[wave];
  uint32_t staged = 0xFFFFFFFFu;      // (no point: n_points < 2^32)
  // (slab < n_slabs - waves before the step: the sum cannot wrap)
  for (uint32_t slab = blockIdx.x * (kTpBlock / 64) + wave; slab < a.n_slabs; slab = (a.n_slabs - slab > waves) ? slab + waves : a.n_slabs) {
    const uint32_t point = slab / a.slabs_per_point;
    if (point != staged) {            // wave-uniform
      double lambda = lambdas[point];
      if (lambda == 0.0) lambda = a.lambda;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (lane <= (uint32_t)kMaxExp) s_lp[wave][lane] = lane == 0u ? 1.0 : ipow_u(lambda, lane);      // (ipow_u(x, 1) is x)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      staged = point;
    }
    const uint32_t k0 = (slab - point * a.slabs_per_point) * kTpSlab;
    const float cs[3] = {a.cs[(size_t)point * 3], a.cs[(size_t)point * 3 + 1], a.cs[(size_t)point * 3 + 2]};
    const uint32_t pix = a.pixel[point];
    const int px = (int)(pix & 0xFFFFu), py = (int)(pix >> 16);
    const uint32_t attempt = (a.first_attempt ? a.first_attempt[point] : 0u) + k0 + lane;
    const bool commit = k0 + lane < a.attempts;
    const uint64_t q = (uint64_t)point * a.attempts + k0 + lane;
    const AttemptTrace t = trace_attempt<true>(a.P, L, a.bokeh, cs, px, py, attempt, commit, NoSeedAnswers{});
    if (commit) {
      a.out_pixel[q] = t.code;
      if (a.out_xy) { a.out_xy[q * 2] = t.xy0; a.out_xy[q * 2 + 1] = t.xy1; }            // (the caller's arrays are 8-byte aligned, no more)
      if (a.out_sensor) { a.out_sensor[q * 2] = t.sen0; a.out_sensor[q * 2 + 1] = t.sen1; }
      if (a.out_tries) a.out_tries[q] = t.tries;
    }
  }
}
