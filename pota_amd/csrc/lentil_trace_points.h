// lentil_trace_points.h -- scene points traced backward through the lens in batches (lentil_hip_trace_points): for a
// camera-space point and an attempt number, where on the sensor a draw of the redistribution pass would put it --
// Camera::trace_ray_bw_po (src/lentil.h:573-661) and the sensor -> pixel mapping of src/lentil_filter.cpp:271-290 for
// polynomial optics, the thin-lens draw of src/lentil_filter.cpp:311-434 (abb_chromatic == 0) for the thin lens.  The
// backward counterpart of lentil_camera_rays.h: no frame, no visits, no accumulators; an occlusion probe only in the probed
// call (lentil_hip_trace_points_probed, at the end of this file).
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
// trace_attempt is that trace of one attempt, and the only one: the slab loop below (tp_slab_loop) calls it once per slab, and
// so do the walks of lentil_list_draws.h (ld_walk, ld_probed_walk; list_draws_chroma_kernel once per colour channel).  What a
// probed caller adds -- answers about the seeds -- comes in as a policy, NoSeedAnswers for everybody else.
//
// The slab loop is written once, tp_slab_loop, with two compile-time policies: the wavelength (FixedLambda, or WaveLambda's
// row of LDS per wave) and the answers (TpUnprobed, or TpProbed: a turn of lentil_hip_trace_points_probed).  The kernels at the
// end of this file declare their LDS, stage the lens and call it; trace_points_spectral_kernel has it written out (see there).
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

// ---- the wavelength policy of the trace and list kernels --------------------------------------------------------------------
// FixedLambda: every point (visit) at a.lambda, whose powers stage_lens put into the block's header; nothing is staged.
// WaveLambda: point j (visit v_begin + j) at lambdas[j], 0: a.lambda, which the host sets to params.lambda_bw -- polynomial
// optics.  A wave traces one point (serves one visit) at a time, so the wavelength is wave-uniform: every wave keeps the lambda
// powers of the one it is at in a row of LDS of its own (LensT = LdsLensAt<LambdaTable> or GenLensAt<Gen>; the block shares the
// header's constants alone) and rewrites the row when it comes to another.  The waves of a block make different numbers of
// trips through every loop of these kernels, so nothing in them may wait for the block.  Nothing has to: the row is the wave's
// own, written by its lanes 0 ... kMaxExp and read by all of them, and LDS serves a wave's accesses in the order it issues
// them.  What is needed is that the compiler keeps the reads of the last point, the writes, and the reads of this point in that
// order; the two wave-scope fences say so (DESIGN.md 4.7 has what the loop compiles to).
LD_DEV void ld_stage_lambda(double *row, double lambda, uint32_t lane) {      // called by the whole wave, `lambda` wave-uniform
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  if (lane <= (uint32_t)kMaxExp) row[lane] = lane == 0u ? 1.0 : ipow_u(lambda, lane);      // (ipow_u(x, 1) is x)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct FixedLambda {
  static constexpr bool kStaged = false;
  template <class LensT> LD_DEV void bind(LensT &) const {}
  LD_DEV double read(uint64_t) const { return 0.0; }
  LD_DEV void stage(double, double, uint32_t) const {}
};

struct WaveLambda {
  static constexpr bool kStaged = true;
  const double *lambdas;
  double *row;                      // the wave's own: kMaxExp + 1 powers
  template <class LensT> LD_DEV void bind(LensT &L) const { L.lam.lp = row; }
  LD_DEV double read(uint64_t j) const { return lambdas[j]; }
  LD_DEV void stage(double lambda, double fallback, uint32_t lane) const { ld_stage_lambda(row, lambda == 0.0 ? fallback : lambda, lane); }
};

// ---------------------------------------------------------------------------------------
// lentil_hip_trace_points_probed: the batch under the context's occlusion probe.  Query (point, m) makes its tries at seeds
// m + tries, and a try whose segment -- from the point's world position to the try's aperture point -- is occluded fails like
// one the lens vignettes (thin lens: the attempt is lost).  Which seeds a query reaches depends on the answers, so the batch is
// traced in turns (lentil_hip.hip: probe_turns).
//
// The answer store.  Two bits per seed offset 0 ... attempts + max(vignetting_retries, 0) - 1 of every point, in the probed
// list's encoding (lentil_list_draws.h: (A, B) = (0, 0) never asked about, (1, 0) asked in this turn, (1, 1) clear, (0, 1)
// occluded), so that ld_probe_apply_kernel serves unchanged.  Every point has the same number of words; point j's begin at
// j * words_per_point.  A seed's offset is m - first_attempt[point], subtracted on the seed itself.
//
// One turn.  The slab loop over the slabs that are not settled, trace_attempt with the store's answers.  A lane whose trace
// comes back `open` -- it got through the lens at a seed whose answer is not known -- asks about that seed (probe_ask_seed).
// A lane that is not open has its final outputs -- a known answer never changes -- and writes them (every turn until its slab
// settles: the same values).  A slab none of whose lanes is open is settled, a byte per slab; the others are counted for the
// host.  Every open query asks about, or finds asked, its next seed in every turn, so a query is open for at most
// max(vignetting_retries, 0) + 1 turns whose lists fit.  A try at a seed known to be occluded fails without a solve
// (trace_attempt).  Every loop is bounded as in the unprobed call.
// ---------------------------------------------------------------------------------------
struct TracePointProbeArgs {
  const float *origin;            // [n_points][3] world space: the segment's origin
  const float *time;              // optional [n_points]: the sample's time (the motion keys' blend)
  const uint8_t *exempt;          // optional [n_points]: non-zero = the skydome supplied the sample
  uint32_t *A, *B;                // the answer store
  uint32_t words_per_point;
  uint8_t *settled;               // [n_slabs]
  unsigned long long *unsettled;  // the slabs this turn left open (reset every turn)
  CamMotion cam;                  // the context's motion keys and shutter, as a visit stream carries them
};

// trace_attempt's policy over a point's words of the store
struct PointSeedAnswers {
  const uint32_t *A, *B;
  uint32_t first;                 // first_attempt[point]
  bool exempt;
  LD_DEV void look(uint32_t m, bool &occluded, bool &known) const {
    occluded = false; known = true;
    if (!exempt) {
      const uint32_t o = m - first;
      const uint32_t bit = 1u << (o & 31u);
      const bool sa = (__hip_atomic_load(&A[o >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) != 0u;
      const bool sb = (B[o >> 5] & bit) != 0u;
      occluded = sb && !sa;
      known = sb;
    }
  }
};

// The lanes with `ask` ask about a seed each: `wa` the seed's word of A, `bit` its bit there, `bit_at` its bit index in the
// whole store.  Neighbouring attempts (the lanes of a slab, the waves that hold neighbouring slabs, the blocks) share seeds: an
// atomicOr on the A bit elects one lister per seed, the elected lanes take slots by probe_wave_slot, and one whose slot lies
// beyond the turn's buffers takes its bit back (the seed is asked about in a later turn; the host grows the buffers from the
// count).  The segment runs from `origin` (world space) to the aperture point (lx, ly) at `time`.  Called by the whole wave.
LD_DEV void probe_ask_seed(const lentil_params &P, const ProbeArgs &pr, bool ask, uint32_t *wa, uint32_t bit, uint32_t bit_at,
                           const CamMotion &cam, float time, const float *origin, float lx, float ly, uint32_t lane) {
  bool win = false;
  if (ask) win = (atomicOr(wa, bit) & bit) == 0u;
  const unsigned long long wm = __ballot(win);
  if (wm) {
    const uint32_t slot = probe_wave_slot(pr.count, wm, lane);
    if (win) {
      if (slot < pr.cap) {
        float c2w[4][4];
        probe_cam_to_world(cam, pr, time, c2w);
        float tgt[3];
        probe_target(P, c2w, lx, ly, 0.0f, tgt);
        lentil_probe_segment sg;
        sg.origin[0] = origin[0]; sg.origin[1] = origin[1]; sg.origin[2] = origin[2];
        sg.target[0] = tgt[0]; sg.target[1] = tgt[1]; sg.target[2] = tgt[2];
        pr.seg[slot] = sg;
        pr.idx[slot] = bit_at;
      } else {
        atomicAnd(wa, ~bit);
      }
    }
  }
}

// What a slab does with its trace: the lanes that are not open commit, the open ones ask.  Called by the whole wave; returns
// whether some lane is open.
LD_DEV bool tp_probed_slab(const TracePointArgs &a, const ProbeArgs &pr, const TracePointProbeArgs &b, const AttemptTrace &t, uint32_t point,
                           uint32_t first, uint32_t attempt, bool commit, uint64_t q, uint32_t lane) {
  if (commit && !t.open) {
    a.out_pixel[q] = t.code;
    if (a.out_xy) { a.out_xy[q * 2] = t.xy0; a.out_xy[q * 2 + 1] = t.xy1; }
    if (a.out_sensor) { a.out_sensor[q * 2] = t.sen0; a.out_sensor[q * 2 + 1] = t.sen1; }
    if (a.out_tries) a.out_tries[q] = t.tries;
  }
  if (!__ballot(t.open)) return false;
  const uint32_t off = point * b.words_per_point;                      // (the host refuses a store of 2^27 words or more per array)
  const uint32_t o = attempt + (uint32_t)t.tries - first;              // < attempts + max(vignetting_retries, 0)
  probe_ask_seed(a.P, pr, t.open, b.A + off + (o >> 5), 1u << (o & 31u), off * 32u + o, b.cam, b.time ? b.time[point] : 0.0f,
                 b.origin + (size_t)point * 3, t.lx, t.ly, lane);
  return true;
}

// the answers policy of the slab loop: nobody probes (NoSeedAnswers, a plain commit), or a turn of the probed call
struct TpUnprobed {
  static constexpr bool kProbed = false;
};
struct TpProbed {
  static constexpr bool kProbed = true;
  const ProbeArgs &pr;
  const TracePointProbeArgs &b;
};

// The slab loop of the four kernels below; s_terms / s_k: the block's staged lens.  Lam: the wavelength policy, its row
// rewritten when the wave's next slab (that is not settled) belongs to another point.
template <class LensT, bool kTables, bool PO, class Lam, class Probe>
LD_DEV void tp_slab_loop(const TracePointArgs &a, const DevTerm *s_terms, const DevLens *s_k, const Lam &lam, const Probe &probe) {
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = s_k;
  lam.bind(L);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * (kTpBlock / 64);
  uint32_t staged = 0xFFFFFFFFu;      // (no point: n_points < 2^32)
  unsigned long long wave_open = 0;
  // (slab < n_slabs - waves before the step: the sum cannot wrap)
  for (uint32_t slab = blockIdx.x * (kTpBlock / 64) + wave; slab < a.n_slabs; slab = (a.n_slabs - slab > waves) ? slab + waves : a.n_slabs) {
    if constexpr (Probe::kProbed) {
      if (probe.b.settled[slab]) continue;      // wave-uniform
    }
    const uint32_t point = slab / a.slabs_per_point;
    if constexpr (Lam::kStaged) {
      if (point != staged) {                    // wave-uniform
        lam.stage(lam.read(point), a.lambda, lane);
        staged = point;
      }
    }
    const uint32_t k0 = (slab - point * a.slabs_per_point) * kTpSlab;
    const float cs[3] = {a.cs[(size_t)point * 3], a.cs[(size_t)point * 3 + 1], a.cs[(size_t)point * 3 + 2]};
    const uint32_t pix = a.pixel[point];
    const int px = (int)(pix & 0xFFFFu), py = (int)(pix >> 16);
    const uint32_t first = a.first_attempt ? a.first_attempt[point] : 0u;
    const uint32_t attempt = first + k0 + lane;
    const bool commit = k0 + lane < a.attempts;
    const uint64_t q = (uint64_t)point * a.attempts + k0 + lane;
    if constexpr (Probe::kProbed) {
      const TracePointProbeArgs &b = probe.b;
      const size_t off = (size_t)point * b.words_per_point;
      const PointSeedAnswers seeds{b.A + off, b.B + off, first, b.exempt && b.exempt[point] != 0};
      const AttemptTrace t = trace_attempt<PO>(a.P, L, a.bokeh, cs, px, py, attempt, commit, seeds);
      if (tp_probed_slab(a, probe.pr, b, t, point, first, attempt, commit, q, lane)) ++wave_open;
      else if (lane == 0u) b.settled[slab] = 1;
    } else {
      const AttemptTrace t = trace_attempt<PO>(a.P, L, a.bokeh, cs, px, py, attempt, commit, NoSeedAnswers{});
      if (commit) {
        a.out_pixel[q] = t.code;
        if (a.out_xy) { a.out_xy[q * 2] = t.xy0; a.out_xy[q * 2 + 1] = t.xy1; }            // (the caller's arrays are 8-byte aligned, no more)
        if (a.out_sensor) { a.out_sensor[q * 2] = t.sen0; a.out_sensor[q * 2 + 1] = t.sen1; }
        if (a.out_tries) a.out_tries[q] = t.tries;
      }
    }
  }
  if constexpr (Probe::kProbed) {
    if (lane == 0u && wave_open) atomicAdd(probe.b.unsettled, wave_open);
  }
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
  tp_slab_loop<LensT, kTables, PO>(a, s_terms, &s_k, FixedLambda{}, TpUnprobed{});
}

// lentil_hip_trace_points_spectral: a wavelength per point, polynomial optics (LensT: SpectralLens<...>::Wave of the scalar
// call's).  What tp_slab_loop is under WaveLambda and TpUnprobed, written out: as a call of tp_slab_loop the compiled-in
// double gauss measured 1.3 % slower than this loop (174.4 against 172.1 ms where two runs of this loop differ by 0.02;
// profiles/one_loop_kernels.txt), and this is the one of the eight kernels with a rate on record to lose.  A
// change to the loop above is made here too.
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
  for (uint32_t slab = blockIdx.x * (kTpBlock / 64) + wave; slab < a.n_slabs; slab = (a.n_slabs - slab > waves) ? slab + waves : a.n_slabs) {
    const uint32_t point = slab / a.slabs_per_point;
    if (point != staged) {            // wave-uniform
      double lambda = lambdas[point];
      if (lambda == 0.0) lambda = a.lambda;
      ld_stage_lambda(s_lp[wave], lambda, lane);
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

// LensT / kTables / PO: as trace_points_kernel.  One launch per turn.
template <class LensT, bool kTables, bool PO>
__global__ __launch_bounds__(kTpBlock) void trace_points_probed_kernel(TracePointArgs a, ProbeArgs pr, TracePointProbeArgs b) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  if (PO) {
    stage_lens<kTables>(a.lens, a.terms, a.lambda, kTpBlock, s_terms, &s_k, threadIdx.x == 0);
    __syncthreads();
  }
  tp_slab_loop<LensT, kTables, PO>(a, s_terms, &s_k, FixedLambda{}, TpProbed{pr, b});
}

// the probed call with a wavelength per point (lentil_point_probe::lambdas), polynomial optics
template <class LensT, bool kTables>
__global__ __launch_bounds__(kTpBlock) void trace_points_probed_spectral_kernel(TracePointArgs a, ProbeArgs pr, TracePointProbeArgs b, const double *lambdas) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  __shared__ double s_lp[kTpBlock / 64][kMaxExp + 1];
  stage_lens<kTables>(a.lens, a.terms, a.lambda, kTpBlock, s_terms, &s_k, threadIdx.x == 0);
  __syncthreads();
  tp_slab_loop<LensT, kTables, true>(a, s_terms, &s_k, WaveLambda{lambdas, s_lp[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]}, TpProbed{pr, b});
}
