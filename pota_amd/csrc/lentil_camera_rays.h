// lentil_camera_rays.h -- forward camera rays in batches: camera_create_ray (src/lentil_camera.cpp:78-125) over
// Camera::trace_ray_fw_po / trace_ray_fw_thinlens (src/lentil.h:283-569), one lane per camera sample.
//
// A ray is three traces in sequence: the ray itself and, at sx + dsx * 0.001f and sy + dsy * 0.001f, the two rays
// its differentials are the finite differences to.  The arithmetic is the reference's operation for operation
// (fp64 where it is double, fp32 where it is float, no contraction), so a ray comes out with the bits the CPU
// computes -- up to what the device's sin / cos / log / exp / powf round differently from the host's libm, which
// only the thin lens's coma and optical-vignetting terms go through.
//
// Convergence.  The table interpreter reads a term's exponents through readfirstlane and branches on them with
// scalar branches, so the vignetting-retry loop is wave-uniform: it runs while ANY lane of the wave still tries, and
// a lane that is done (or past the batch's end) computes along on the values it has and commits nothing.  The three
// traces are one wave-uniform loop for the same reason.  (The Newton loop inside lens_pt_sample_aperture still ends
// per lane, as in focus_miss_kernel: every lane reads the same term, so the value readfirstlane returns is right for
// whichever lanes are still iterating.)  A compiled lens (GenLens<Gen>: the polynomials as straight-line code, no
// readfirstlane) runs the same uniform loops: a wave lasts as long as its slowest lane whether the others leave or
// compute along, and one body of trace_ray_fw_po serves every lens type.
//
// xor128.  The reference redraws the lens sample of a vignetted try from xor128 (src/global.h:22-27), whose state
// it keeps in function statics -- one per process, advanced by whichever thread gets there first.  Here every ray
// owns a state derived from its id (w0 = tea8(id, seed), w_k = tea8(id, w_{k-1})), so what a ray draws depends on
// neither the other rays nor how a batch is split into calls.
#pragma once
#include "lentil_kernels.h"

constexpr int kRayInFloats = 6;     // sx, sy, dsx, dsy, lensx, lensy
constexpr int kRayOutFloats = 21;   // lentil_host_camera_ray: origin, dir, weight, dOdx, dOdy, dDdx, dDdy
constexpr int kRayBlock = 256;

struct CameraRayArgs {
  lentil_params P;
  const DevLens *lens;      // polynomial optics only
  const DevTerm *terms;
  DevBokeh bokeh;
  uint64_t n;
  uint32_t first_ray;
  uint32_t differentials;
  const float *in;          // [n][6]
  float *out;               // [n][21]
  int32_t *tries;           // optional [n]
  double lambda;
  float exposure;
  uint32_t rng_seed;
};

struct FwRay {
  float o[3], d[3];
  float w;        // 1, or 0 when every try was vignetted (polynomial optics: or a NaN came out)
  int tries;
};

struct RayRng { uint32_t x, y, z, w; };

LD_DEV RayRng ray_rng_init(uint32_t id, uint32_t seed) {
  RayRng s;
  s.x = tea8(id, seed); s.y = tea8(id, s.x); s.z = tea8(id, s.y); s.w = tea8(id, s.z);
  if ((s.x | s.y | s.z | s.w) == 0u) { s.x = 123456789u; s.y = 362436069u; s.z = 521288629u; s.w = 88675123u; }   // the all-zero state is xor128's fixed point
  return s;
}
LD_DEV double ray_rng_draw(RayRng &s) { return (double)xor128_next(s.x, s.y, s.z, s.w) / 4294967296.0; }

// The aperture point of a try (src/lentil.h:300-330, 452-470), on the unit disk.  `trying` lanes draw; the others keep
// their lens sample and their generator.
template <bool PO>
LD_DEV void fw_lens_sample(const lentil_params &P, const DevBokeh &B, RayRng &rng, double &r1, double &r2, bool redraw,
                           bool trying, double &ux, double &uy) {
  ux = 0.0; uy = 0.0;
  if (!P.enable_dof) return;
  if (redraw) { r1 = ray_rng_draw(rng); r2 = ray_rng_draw(rng); }
  if (P.bokeh_enable_image) {
    if (trying) { ray_rng_draw(rng); ray_rng_draw(rng); }      // the two stratification draws the reference makes and drops
    bokeh_sample(B, B.cdfRow, (float)r1, (float)r2, ux, uy);
  } else if (P.bokeh_aperture_blades < 2) {
    if (PO) concentric_disk_sample(r1, r2, ux, uy);
    else concentricDiskSample_tl((float)r1, (float)r2, ux, uy, P.abb_spherical, P.circle_to_square);
  } else {
    triangular_aperture(ux, uy, r1, r2, 1.0, P.bokeh_aperture_blades, B.blade_sc, B.blade_count);
  }
}

// Camera::trace_ray_fw_po, src/lentil.h:283-427.  A differential trace (deriv_ray) keeps r1, r2, so every one of its
// tries computes what its first did: it makes that one try only (its try count is not part of the result).
template <class Lens>
LD_DEV void trace_ray_fw_po(const lentil_params &P, const Lens &L, const DevBokeh &B, RayRng &rng, double sx, double sy,
                            double &r1, double &r2, bool deriv_ray, bool active, FwRay &ray) {
  const DevLens &k = L.consts();
  const int last_try = (deriv_ray && P.vignetting_retries > 0) ? 0 : P.vignetting_retries;
  int tries = 0;
  bool ok = false;
  bool trying = active && tries <= last_try;
  double out[4] = {0.0, 0.0, 0.0, 0.0};
  while (__any(trying)) {
    double sensor[4] = {sx * (P.sensor_width * 0.5), sy * (P.sensor_width * 0.5), 0.0, 0.0};
    double ux, uy;
    fw_lens_sample<true>(P, B, rng, r1, r2, trying && !deriv_ray && tries > 0, trying, ux, uy);
    const double ax = ux * P.aperture_radius, ay = uy * P.aperture_radius;
    if (P.enable_dof) {
      double adx, ady;
      lens_pt_sample_aperture(L, sensor, ax, ay, P.sensor_shift, adx, ady);
    }
    sensor[0] += sensor[2] * P.sensor_shift;
    sensor[1] += sensor[3] * P.sensor_shift;
    double o4[4];
    const double transmittance = lens_evaluate(L, sensor, o4);
    bool pass = !(transmittance <= 0.0);
    if (o4[0] * o4[0] + o4[1] * o4[1] > k.outer_pupil_radius * k.outer_pupil_radius) pass = false;
    const double px = sensor[0] + sensor[2] * k.back_focal_length, py = sensor[1] + sensor[3] * k.back_focal_length;
    if (px * px + py * py > k.inner_pupil_radius * k.inner_pupil_radius) pass = false;
    if (trying) {
      out[0] = o4[0]; out[1] = o4[1]; out[2] = o4[2]; out[3] = o4[3];
      if (pass) { ok = true; trying = false; }
      else { ++tries; trying = tries <= last_try; }
    }
  }
  const double R = k.outer_pupil_curvature_radius;
  double pos[3], dir[3];
  if (k.outer_pupil_geometry == LENTIL_GEOM_SPHERICAL) sphereToCs(out[0], out[1], out[2], out[3], pos, dir, -R, R);
  else cylinderToCs(out[0], out[1], out[2], out[3], pos, dir, -R, R, k.outer_pupil_geometry == LENTIL_GEOM_CYL_Y);
  float sc = -1.0f;                                           // src/lentil.h:395-416
  if (P.unitModel == LENTIL_UNIT_CM) sc = -0.1f;
  else if (P.unitModel == LENTIL_UNIT_DM) sc = -0.01f;
  else if (P.unitModel == LENTIL_UNIT_M) sc = -0.001f;
  bool nan = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) { ray.o[c] = (float)pos[c] * sc; ray.d[c] = (float)dir[c] * sc; }
  v3norm(ray.d[0], ray.d[1], ray.d[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) nan = nan || ray.o[c] != ray.o[c] || ray.d[c] != ray.d[c];
  ray.w = (ok && !nan) ? 1.0f : 0.0f;
  ray.tries = tries;
}

// Camera::trace_ray_fw_thinlens, src/lentil.h:431-569
LD_DEV void trace_ray_fw_thinlens(const lentil_params &P, const DevBokeh &B, RayRng &rng, double sx, double sy, double &r1,
                                  double &r2, bool deriv_ray, bool active, FwRay &ray) {
  const int last_try = (deriv_ray && P.vignetting_retries > 0) ? 0 : P.vignetting_retries;      // (the vignetting test is the main trace's alone)
  int tries = 0;
  bool ok = false;
  bool trying = active && tries <= last_try;
  float og[3] = {0.0f, 0.0f, 0.0f}, dg[3] = {0.0f, 0.0f, 0.0f};
  while (__any(trying)) {
    float ssx = (float)sx, ssy = (float)sy;
    if (P.abb_distortion > 0.0f) {                            // barrelDistortion, src/lens.h:545-548
      const float f = (float)(1. + (double)((ssx * ssx + ssy * ssy) * P.abb_distortion));
      ssx *= f; ssy *= f;
    }
    float dcx = (float)((double)ssx * (P.sensor_width * 0.5)), dcy = (float)((double)ssy * (P.sensor_width * 0.5)), dcz = -P.focal_length;
    v3norm(dcx, dcy, dcz);
    double ux, uy;
    fw_lens_sample<false>(P, B, rng, r1, r2, trying && !deriv_ray && tries > 0, trying, ux, uy);
    ux *= (double)P.bokeh_anamorphic;
    const float lx = (float)(ux * P.aperture_radius), ly = (float)(uy * P.aperture_radius), lz = 0.0f;
    const float hit = (float)fabs(P.focus_distance / (double)lerpf(0.0f, dcz, 1.0f));
    float dlx = dcx * hit - lx, dly = dcy * hit - ly, dlz = dcz * hit - lz;
    v3norm(dlx, dly, dlz);
    {                                                         // coma, src/lentil.h:490-491
      const float mult = P.abb_coma * abb_coma_multipliers((float)P.sensor_width, P.focal_length, dcx, dcy, dcz, ux, uy);
      float rx, ry, rz;
      abb_coma_perturb(dlx, dly, dlz, dlx, dly, dlz, mult, false, rx, ry, rz);
      dlx = rx; dly = ry; dlz = rz;
    }
    bool pass = true;
    if (P.optical_vignetting_distance > 0.0f && !deriv_ray) { // src/lens.h:529-543
      const float squarebias = (float)(1.0 + log(1.0 + (double)P.circle_to_square) * exp((double)P.circle_to_square * 3.0));
      const float inter = fabsf(P.optical_vignetting_distance / dlz);
      const float ovx = dlx * inter - lx, ovy = dly * inter - ly;
      const float power = (float)(1.0 + (double)squarebias);
      const float radius = (float)P.aperture_radius * P.optical_vignetting_radius;
      const float dist = powf(fabsf(ovx), power) + powf(fabsf(ovy), power);
      if (dist > powf(radius, power)) pass = false;
    }
    if (trying) {
      if (pass) {
        float sc = 1.0f;                                      // src/lentil.h:540-561
        if (P.unitModel == LENTIL_UNIT_MM) sc = 10.0f;
        else if (P.unitModel == LENTIL_UNIT_DM) sc = 0.1f;
        else if (P.unitModel == LENTIL_UNIT_M) sc = 0.01f;
        og[0] = lx * sc; og[1] = ly * sc; og[2] = lz * sc;
        dg[0] = dlx * sc; dg[1] = dly * sc; dg[2] = dlz * sc;
        ok = true; trying = false;
      } else {
        ++tries; trying = tries <= last_try;
      }
    }
  }
  v3norm(dg[0], dg[1], dg[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) { ray.o[c] = og[c]; ray.d[c] = dg[c]; }
  ray.w = ok ? 1.0f : 0.0f;
  ray.tries = tries;
}

// One lane per ray, 256 rays per block.  A block's input (24 B per ray) and output (84 B per ray) are contiguous in
// memory: both go through LDS, lanes moving consecutive dwords, so that no lane strides through 21 dwords of its own.
// LensT / kTables: LdsLens with the term table staged into LDS (the interpreter; also the thin lens's, which has no lens:
// PO false), or GenLens<Gen> of a compiled-in or run-time lens -- straight-line polynomials, only the header, the lambda
// powers and the I/O buffer in LDS.
template <class LensT, bool kTables, bool PO>
__global__ __launch_bounds__(kRayBlock) void camera_rays_kernel(CameraRayArgs a) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  __shared__ float s_io[kRayBlock * kRayOutFloats];
  if (PO) stage_lens<kTables>(a.lens, a.terms, a.lambda, kRayBlock, s_terms, &s_k, threadIdx.x == 0);      // (the barrier is the input's, below)
  const uint64_t ray0 = (uint64_t)blockIdx.x * kRayBlock;
  const uint32_t nb = (uint32_t)((a.n - ray0) < (uint64_t)kRayBlock ? (a.n - ray0) : (uint64_t)kRayBlock);   // >= 1: the grid is ceil(n / 256)
  for (uint32_t j = threadIdx.x; j < nb * kRayInFloats; j += kRayBlock) s_io[j] = a.in[ray0 * kRayInFloats + j];
  __syncthreads();
  const bool active = threadIdx.x < nb;
  const uint32_t li = active ? threadIdx.x : nb - 1u;          // lanes past the end walk along on the last ray
  float in[kRayInFloats];
#pragma unroll
  for (int c = 0; c < kRayInFloats; ++c) in[c] = s_io[li * kRayInFloats + c];
  __syncthreads();                                             // (s_io takes the output next)

  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = &s_k;
  RayRng rng = ray_rng_init(a.first_ray + (uint32_t)ray0 + li, a.rng_seed);
  double r1 = (double)in[4], r2 = (double)in[5];
  const float step = 0.001f;
  const float sxd = in[0] + (in[2] * step), syd = in[1] + (in[3] * step);
  const float inv = 1.0f / step;                               // AtVector / float multiplies by 1 / f
  float res[kRayOutFloats];
#pragma unroll
  for (int c = 9; c < kRayOutFloats; ++c) res[c] = 0.0f;
  int tries_main = 0;
  const int n_traces = a.differentials ? 3 : 1;
  for (int t = 0; t < n_traces; ++t) {
    const double sx = (double)(t == 1 ? sxd : in[0]), sy = (double)(t == 2 ? syd : in[1]);
    FwRay ray;
    if (PO) trace_ray_fw_po(a.P, L, a.bokeh, rng, sx, sy, r1, r2, t != 0, active, ray);
    else trace_ray_fw_thinlens(a.P, a.bokeh, rng, sx, sy, r1, r2, t != 0, active, ray);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (t == 0) { res[c] = ray.o[c]; res[3 + c] = ray.d[c]; res[6 + c] = ray.w * a.exposure; }
      else if (t == 1) { res[9 + c] = (ray.o[c] - res[c]) * inv; res[15 + c] = (ray.d[c] - res[3 + c]) * inv; }
      else { res[12 + c] = (ray.o[c] - res[c]) * inv; res[18 + c] = (ray.d[c] - res[3 + c]) * inv; }
    }
    if (t == 0) tries_main = ray.tries;
  }
#pragma unroll
  for (int c = 0; c < kRayOutFloats; ++c) s_io[threadIdx.x * kRayOutFloats + c] = res[c];
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < nb * kRayOutFloats; j += kRayBlock) a.out[ray0 * kRayOutFloats + j] = s_io[j];
  if (a.tries && active) a.tries[ray0 + threadIdx.x] = tries_main;
}

// lentil_hip_camera_rays_spectral: ray i at lambdas[i] (a.lambda is not read), polynomial optics.  camera_rays_kernel line
// for line but for the lens it hands trace_ray_fw_po (a kernel of its own, not a parameter of that one: the scalar call's
// code stays what it is).  The wavelength differs from lane to lane, so the lambda powers are the lane's own and the block
// shares the header's constants alone: a compiled-in lens (LensT = GenLensAt<Gen>) gets the powers as a local array that its
// straight-line code indexes with constants -- registers -- and the interpreter (LdsLensAt<LambdaLane>) raises the lane's
// wavelength at the term, the exponent being wave-uniform like the others (DESIGN.md 4.6 has the LDS table it was weighed
// against).
template <class LensT, bool kTables>
__global__ __launch_bounds__(kRayBlock) void camera_rays_spectral_kernel(CameraRayArgs a, const double *lambdas) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  __shared__ float s_io[kRayBlock * kRayOutFloats];
  stage_lens<kTables>(a.lens, a.terms, 0.0, kRayBlock, s_terms, &s_k, threadIdx.x == 0);      // (the barrier is the input's, below)
  const uint64_t ray0 = (uint64_t)blockIdx.x * kRayBlock;
  const uint32_t nb = (uint32_t)((a.n - ray0) < (uint64_t)kRayBlock ? (a.n - ray0) : (uint64_t)kRayBlock);   // >= 1: the grid is ceil(n / 256)
  for (uint32_t j = threadIdx.x; j < nb * kRayInFloats; j += kRayBlock) s_io[j] = a.in[ray0 * kRayInFloats + j];
  __syncthreads();
  const bool active = threadIdx.x < nb;
  const uint32_t li = active ? threadIdx.x : nb - 1u;          // lanes past the end walk along on the last ray
  float in[kRayInFloats];
#pragma unroll
  for (int c = 0; c < kRayInFloats; ++c) in[c] = s_io[li * kRayInFloats + c];
  __syncthreads();                                             // (s_io takes the output next)

  const double lambda = lambdas[ray0 + li];
  double lp[kMaxExp + 1];
  LensT L{};
  L.k = &s_k;
  if constexpr (kTables) {
    L.terms = s_terms;
    L.lam.lambda = lambda;
  } else {
    lambda_powers(lambda, lp);
    L.lam.lp = lp;
  }
  RayRng rng = ray_rng_init(a.first_ray + (uint32_t)ray0 + li, a.rng_seed);
  double r1 = (double)in[4], r2 = (double)in[5];
  const float step = 0.001f;
  const float sxd = in[0] + (in[2] * step), syd = in[1] + (in[3] * step);
  const float inv = 1.0f / step;                               // AtVector / float multiplies by 1 / f
  float res[kRayOutFloats];
#pragma unroll
  for (int c = 9; c < kRayOutFloats; ++c) res[c] = 0.0f;
  int tries_main = 0;
  const int n_traces = a.differentials ? 3 : 1;
  for (int t = 0; t < n_traces; ++t) {
    const double sx = (double)(t == 1 ? sxd : in[0]), sy = (double)(t == 2 ? syd : in[1]);
    FwRay ray;
    trace_ray_fw_po(a.P, L, a.bokeh, rng, sx, sy, r1, r2, t != 0, active, ray);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (t == 0) { res[c] = ray.o[c]; res[3 + c] = ray.d[c]; res[6 + c] = ray.w * a.exposure; }
      else if (t == 1) { res[9 + c] = (ray.o[c] - res[c]) * inv; res[15 + c] = (ray.d[c] - res[3 + c]) * inv; }
      else { res[12 + c] = (ray.o[c] - res[c]) * inv; res[18 + c] = (ray.d[c] - res[3 + c]) * inv; }
    }
    if (t == 0) tries_main = ray.tries;
  }
#pragma unroll
  for (int c = 0; c < kRayOutFloats; ++c) s_io[threadIdx.x * kRayOutFloats + c] = res[c];
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < nb * kRayOutFloats; j += kRayBlock) a.out[ray0 * kRayOutFloats + j] = s_io[j];
  if (a.tries && active) a.tries[ray0 + threadIdx.x] = tries_main;
}
