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

// LensT / kTables: LdsLens with the term table staged into LDS (the interpreter; also the thin lens's, which has no lens: PO
// false), or GenLens<Gen> of a compiled-in lens -- only the header and the lambda powers in LDS.
template <class LensT, bool kTables, bool PO>
__global__ __launch_bounds__(kTpBlock) void trace_points_kernel(TracePointArgs a) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  if (PO) {
    if (kTables) {
      const uint32_t nt = a.lens->n_terms;
      for (uint32_t i = threadIdx.x; i < nt; i += kTpBlock) s_terms[i] = a.terms[i];
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
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * (kTpBlock / 64);
  const double qnan = __builtin_nan("");
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

    uint32_t code = LENTIL_POINT_VIGNETTED;
    double xy0 = qnan, xy1 = qnan, sen0 = qnan, sen1 = qnan;
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
        sen0 = sensor[0] + sensor[2] * -P.sensor_shift;
        sen1 = sensor[1] + sensor[3] * -P.sensor_shift;
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
    if (commit) {
      a.out_pixel[q] = code;
      if (a.out_xy) { a.out_xy[q * 2] = xy0; a.out_xy[q * 2 + 1] = xy1; }            // (the caller's arrays are 8-byte aligned, no more)
      if (a.out_sensor) { a.out_sensor[q * 2] = sen0; a.out_sensor[q * 2 + 1] = sen1; }
      if (a.out_tries) a.out_tries[q] = tries;
    }
  }
}
