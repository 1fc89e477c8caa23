// lentil_list_draws.h -- two queries over the context's bound visit stream, for a renderer that keeps its own film
// (lentil_hip_plan_visits, lentil_hip_list_draws): what the visit prologue decides per visit (src/lentil_filter.cpp:105-240),
// and the accepted draws of a visit range -- the first `samples` attempts among 0 ... 5 * samples - 1 that get through the lens
// and land in the frame (the loops of src/lentil_filter.cpp:249-300 and :311-447) -- with their continuous pixel coordinates.
// No frame, no accumulators, no counter block, no xor128 state; occlusion probes only in the probed list further down.  Polynomial
// optics with abb_chromatic != 0 -- three colour channels per attempt, counted by another rule -- have a kernel of their own at
// the end of this file (list_draws_chroma_kernel, LENTIL_DRAWS_CHANNELS).  A wavelength per visit (lentil_hip_list_draws_spectral)
// is a policy of the two walks (WaveLambda, lentil_trace_points.h): list_draws_spectral_kernel is ld_walk, as
// list_draws_kernel is, and list_draws_probed_spectral_kernel is ld_probed_walk, which list_draws_probed_kernel has written out.
//
// plan_visits_kernel.  One lane per visit, 64 consecutive visits per wave and step (the five 16-byte columns are read
// coalesced), grid-stride over such groups; visit_prologue and visit_pixel are the pass's own (load_work_visit), the weight
// is formed as load_work_visit and the scan form it.  A 32-byte record per lane.  The totals are counted by ballot and
// __popcll (the samples by a shuffle reduction) into wave-uniform sums: one atomic per wave and total, at the end.
//
// list_draws_kernel.  A wave takes 64 consecutive visits on a dynamic ticket (one atomic per 64 visits), runs the prologue
// with lane = visit, ballots the redistribute decisions and then serves the set lanes one after another: the visit's position,
// pixel and draw count are handed to the whole wave through readlane (scalar registers), and the wave walks the visit's
// attempts 64 at a time with lane = attempt.  A slab is traced by trace_attempt (lentil_trace_points.h: the one backward trace
// of an attempt, which trace_points_kernel and the three list kernels of this file call), its successes are balloted, and a
// success is taken while accepted_so_far + popcount(ballot & lower lanes) < samples -- the attempts the reference's loop
// would have accepted before it stopped.  The slab's records take consecutive slots of the list through one atomic
// (probe_wave_slot's pattern on a 64-bit counter) and are written where the slot lies below the capacity; the counter runs on,
// so the caller learns how many there are.  The attempts a visit made -- up to its last accepted draw if that was the
// `samples`-th, else all 5 * samples -- are summed per wave and go out once, behind the ticket loop: one atomic per wave.
// Every loop is bounded: ceil(n_visits / 64) tickets, at most 64 visits per ticket, at most ceil(5 * samples / 64) slabs per
// visit, at most vignetting_retries + 1 tries, at most 100 Newton iterations (newton_continue).
// What a record holds depends on its (visit, attempt) alone, so the list as a set does not depend on the grid, on the
// capacity or on how the stream is split into ranges; the order of the records does.
//
// The walk over the visits -- ticket, prologue, broadcast, slab step, the attempts made, the record store -- is the ld_*
// helpers below, shared by the list kernels (the prologue also by plan_visits_kernel and ld_probe_alloc_kernel).
#pragma once
#include "lentil_trace_points.h"

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

// A lane's visit: its columns through the pass's prologue (load_work_visit's line) and its pixel.  All zero, `redistribute`
// false, on a lane without a visit.
struct LdVisitLane {
  VisitInfo I;
  int px, py;
  float invd;
  float4 pos_z, raydir_time;
};

LD_DEV LdVisitLane ld_visit_lane(const lentil_params &P, const VisitsDev &V, double lens_length, uint64_t v) {
  LdVisitLane x;
  x.invd = V.inv_density ? V.inv_density[v] : P.inverse_sample_density;
  x.pos_z = V.pos_z[v];
  x.raydir_time = V.raydir_time[v];
  x.I = visit_prologue(P, lens_length, V.rgba[v], x.pos_z, x.raydir_time, V.volume_ignore[v], V.transmission[v], x.invd, V.cam);
  visit_pixel(V, v, x.px, x.py);
  return x;
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
      const LdVisitLane x = ld_visit_lane(a.P, V, a.lens_length, v);
      const VisitInfo &I = x.I;
      red = I.redistribute;
      lentil_visit_plan r;
      r.cs[0] = I.cs[0]; r.cs[1] = I.cs[1]; r.cs[2] = I.cs[2];
      r.add_energy = red ? I.add_energy : 0.0f;
      r.weight = plan_weight(x.invd, red, I.samples);
      r.samples = (uint32_t)I.samples;
      r.pixel = (uint32_t)((x.px & 0xFFFF) | (x.py << 16));
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
LD_DEV double ld_readlane(double x, int src) { return __longlong_as_double((long long)ld_readlane((unsigned long long)__double_as_longlong(x), src)); }

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
// ---- the visit walk of the list kernels ------------------------------------------------------------------------------------
// A wave's next group of 64 visits, on a dynamic ticket: one atomic per group, handed to the wave through readlane; the
// ticket loop ends at the first ticket that is no group.  Its body must not end in a branch on the lane: with
// `if (lane == 0u)` twice in a row -- a wave sum's atomic at the body's end, then this one -- the compiler once sent lanes
// 1 ... 63 straight back to the readlane here, past lane 0 and its atomic (jump threading over the two equal conditions): they
// read ticket 0 again and never left.  So a wave's sums go out once, behind the ticket loop (ld_add_wave_sum).
LD_DEV unsigned long long ld_take_ticket(unsigned long long *ticket, uint32_t lane) {
  unsigned long long g = 0;
  if (lane == 0u) g = atomicAdd(ticket, 1ull);
  return ld_readlane(g, 0);
}

LD_DEV void ld_add_wave_sum(unsigned long long *total, unsigned long long sum, uint32_t lane) {
  if (lane == 0u && sum) atomicAdd(total, sum);
}

// The visit of lane `src`, handed to the whole wave through readlane: scalar registers.
struct LdWaveVisit {
  float cs[3];
  int px, py;
  uint32_t samples;
  uint32_t max_total;               // 5 * samples, unsigned, as the reference's max_total_samples
  uint32_t visit;                   // its number in the stream; visit0: that of the group's lane 0
};

LD_DEV LdWaveVisit ld_broadcast_visit(const LdVisitLane &x, int src, uint32_t visit0) {
  LdWaveVisit w;
  w.cs[0] = ld_readlane(x.I.cs[0], src); w.cs[1] = ld_readlane(x.I.cs[1], src); w.cs[2] = ld_readlane(x.I.cs[2], src);
  w.px = (int)ld_readlane((uint32_t)x.px, src); w.py = (int)ld_readlane((uint32_t)x.py, src);
  w.samples = ld_readlane((uint32_t)x.I.samples, src);
  w.max_total = w.samples * 5u;
  w.visit = visit0 + (uint32_t)src;
  return w;
}

// the slab behind the one at k0 < max_total, without the sum's wrap; lane = attempt commits while max_total - k0 > lane
LD_DEV uint32_t ld_next_slab(uint32_t k0, uint32_t max_total) { return (max_total - k0 > kLdSlab) ? k0 + kLdSlab : max_total; }

// The attempts a visit has made behind the slab at k0: its loop ends behind the attempt that brought its count to `samples`
// (`reached`, on lane last_lane); a slab without it was attempted to its end.
LD_DEV uint32_t ld_made(uint32_t k0, uint32_t max_total, bool reached, uint32_t last_lane) {
  return reached ? k0 + last_lane + 1u : ld_next_slab(k0, max_total);
}

// a record at its slot, where the slot lies below the capacity (the counter runs on)
LD_DEV void ld_store_draw(const ListDrawArgs &a, unsigned long long slot, uint32_t visit, uint32_t attempt, uint32_t code, int tries,
                          double xy0, double xy1) {
  if (slot < a.capacity) {
    lentil_draw r;
    r.visit = visit; r.attempt = attempt; r.pixel = code; r.tries = tries;
    r.xy[0] = xy0; r.xy[1] = xy1;
    a.out[slot] = r;
  }
}

// The walk of list_draws_kernel and list_draws_spectral_kernel; s_terms / s_k: the block's staged lens.  Lam: the wavelength
// policy of lentil_trace_points.h.  WaveLambda (lentil_hip_list_draws_spectral) takes visit v at lambdas[v - v_begin]: read in
// the prologue, lane = visit, one coalesced load per group of 64 visits; the served visit's goes to the whole wave through
// readlane, like everything else of the visit -- a scalar register, no load inside the walk -- and the wave's row is rewritten
// before every visit's walk, not between the slabs of one visit.  A wave's trips through every loop here differ from its
// block's other waves', so nothing waits for the block (see the policy).
template <class LensT, bool kTables, bool PO, class Lam>
LD_DEV void ld_walk(const ListDrawArgs &a, const DevTerm *s_terms, const DevLens *s_k, const Lam &lam) {
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = s_k;
  lam.bind(L);
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long n_groups = (a.v_end - a.v_begin + 63u) / 64u;
  unsigned long long wave_attempts = 0;
  for (;;) {
    const unsigned long long g = ld_take_ticket(&a.ctr[0], lane);
    if (g >= n_groups) break;
    // ---- the prologue, lane = visit: its columns and, where the policy stages one, its wavelength
    const uint64_t v = a.v_begin + g * 64u + lane;
    LdVisitLane x{};
    double lam_v = 0.0;
    if (v < a.v_end) {
      x = ld_visit_lane(a.P, a.V, a.lens_length, v);
      lam_v = lam.read(v - a.v_begin);                                   // (indexed by the range, not by the stream)
    }
    unsigned long long todo = __ballot(x.I.redistribute);
    // ---- the set lanes one after another, lane = attempt
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const LdWaveVisit w = ld_broadcast_visit(x, src, (uint32_t)(a.v_begin + g * 64u));
      if constexpr (Lam::kStaged) lam.stage(ld_readlane(lam_v, src), a.lambda, lane);
      uint32_t accepted = 0, made = 0;
      for (uint32_t k0 = 0; k0 < w.max_total && accepted < w.samples; k0 = ld_next_slab(k0, w.max_total)) {
        const uint32_t attempt = k0 + lane;
        const bool commit = w.max_total - k0 > lane;
        const AttemptTrace t = trace_attempt<PO>(a.P, L, a.bokeh, w.cs, w.px, w.py, attempt, commit, NoSeedAnswers{});

        // ---- the reference's selection: the successes in attempt order, until `samples` of them are in
        const bool success = commit && t.code < LENTIL_POINT_OUTSIDE;
        const unsigned long long okm = __ballot(success);
        const bool take = success && accepted + (uint32_t)__builtin_popcountll(okm & below) < w.samples;
        const unsigned long long tm = __ballot(take);
        if (tm) {
          const unsigned long long slot = list_wave_slot(&a.ctr[1], tm, lane);
          if (take) ld_store_draw(a, slot, w.visit, attempt, t.code, t.tries, t.xy0, t.xy1);
        }
        accepted += (uint32_t)__builtin_popcountll(tm);
        made = ld_made(k0, w.max_total, accepted >= w.samples, (uint32_t)(63 - __builtin_clzll(tm | 1ull)));   // (| 1: defined for an empty mask, whose lane nobody asks for)
      }
      wave_attempts += made;
    }
  }
  ld_add_wave_sum(&a.ctr[2], wave_attempts, lane);
}

template <class LensT, bool kTables, bool PO>
__global__ __launch_bounds__(kLdBlock) void list_draws_kernel(ListDrawArgs a) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  if (PO) {
    stage_lens<kTables>(a.lens, a.terms, a.lambda, kLdBlock, s_terms, &s_k, threadIdx.x == 0);
    __syncthreads();
  }
  ld_walk<LensT, kTables, PO>(a, s_terms, &s_k, FixedLambda{});
}

// lentil_hip_list_draws_spectral: WaveLambda, polynomial optics with abb_chromatic == 0 (LensT: SpectralLens<...>::Wave of the
// scalar call's)
template <class LensT, bool kTables>
__global__ __launch_bounds__(kLdBlock) void list_draws_spectral_kernel(ListDrawArgs a, const double *lambdas) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  __shared__ double s_lp[kLdBlock / 64][kMaxExp + 1];
  stage_lens<kTables>(a.lens, a.terms, a.lambda, kLdBlock, s_terms, &s_k, threadIdx.x == 0);
  __syncthreads();
  ld_walk<LensT, kTables, true>(a, s_terms, &s_k, WaveLambda{lambdas, s_lp[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]});
}

// ---------------------------------------------------------------------------------------
// LENTIL_DRAWS_PROBED: the list under the context's occlusion probe.  Seed m = attempt + try of a visit is occluded or it is
// not, whichever attempt looks at it; which seeds a visit reaches depends on the answers, so the list is made in turns.
//
// The answer store.  Two bits per seed 0 ... 5 * samples + max(vignetting_retries, 0) of every redistributed visit, in two
// word arrays A and B: (A, B) = (0, 0) never asked about, (1, 0) asked in this turn, (1, 1) clear, (0, 1) occluded.
// ld_probe_alloc_kernel hands every visit of the range its word offset (a wave scan and one atomic per 64 visits) and its
// LdVisitState; ld_probe_apply_kernel, behind the callback, turns every listed seed's (1, 0) into clear or occluded.
//
// list_draws_probed_kernel, one per turn: list_draws_kernel's walk (the ld_* helpers) over the visits that are not settled,
// trace_attempt with the store's answers (SeedAnswers).  A try at a seed known to be occluded fails without a solve.  A try that gets through the lens at a seed whose
// answer is not known leaves its lane `dirty`: what the attempt comes to is open.  The reference reaches attempt n only
// while fewer than `samples` lower attempts were accepted, and an open attempt may yet be accepted (its seed clear) or not --
// even one whose optimistic trace lands outside the frame, since an occluded seed hands the attempt to the next try, which may
// land inside.  So a dirty lane asks only where accepted + (the successes and the dirty lanes below it) < samples: then the
// reference reaches it whatever the open answers are, and no seed is asked about that the final walk does not reach.  The
// lowest dirty lane of a walk always qualifies (below it everything is known), so every walk of an unsettled visit asks
// about a new seed: at most 5 * samples + vignetting_retries + 1 turns.  Neighbouring attempts share seeds; an atomicOr on the
// A bit elects the lister, the elected lanes take slots by probe_wave_slot, and one whose slot lies beyond the turn's
// buffers takes its A bit back (the seed is asked about in a later turn; the host grows the buffers from the count).
// A slab in which no lane asks is final -- its every consulted seed has its answer -- as long as every slab before it was:
// its records are written as list_draws_kernel writes them and the visit's LdVisitState moves behind it, so a later turn
// resumes there and no record is written twice.  Behind a slab that asked, the walk goes on optimistically with the upper
// bound of the accepted count, only to ask.  A visit whose walk reaches its end with every slab final is settled.
// Every loop is bounded as in list_draws_kernel; the turns are the host's (lentil_hip.hip: list_draws_probed).
// ---------------------------------------------------------------------------------------
constexpr uint32_t kLdSettled = 0xFFFFFFFFu;

struct LdVisitState {               // 16 bytes per visit of the range
  uint32_t off;                     // the visit's first word in A and in B
  uint32_t k0;                      // the first attempt of the first slab that is not final; kLdSettled: nothing left to do
  uint32_t accepted;                // accepted draws below k0
  uint32_t pad;
};

struct ListProbeArgs {
  LdVisitState *st;                 // [v_end - v_begin]
  uint32_t *A, *B;                  // the answer store
  unsigned long long *x;            // [0] words handed out, [1] the most seeds of a visit, [2] occluded answers, [3] a turn's count before the clamp
};

LD_DEV uint32_t ld_seed_count(const lentil_params &P, uint32_t samples) {
  const uint32_t r = P.cameraType == LENTIL_POLYNOMIAL_OPTICS && P.vignetting_retries > 0 ? (uint32_t)P.vignetting_retries : 0u;
  const unsigned long long n = (unsigned long long)(samples * 5u) + r + 1ull;      // (samples * 5u wraps as max_total does)
  return n > 0xFFFFFFE0ull ? 0xFFFFFFE0u : (uint32_t)n;
}

__global__ __launch_bounds__(kLdBlock) void ld_probe_alloc_kernel(PlanArgs a, ListProbeArgs b) {
  const VisitsDev &V = a.V;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kLdBlock / 64) + (threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (kLdBlock / 64);
  const uint64_t n_groups = (a.v_end - a.v_begin + 63u) / 64u;
  unsigned long long most = 0;
  for (uint64_t g = wave; g < n_groups; g += waves) {
    const uint64_t v = a.v_begin + g * 64u + lane;
    const bool valid = v < a.v_end;
    unsigned long long words = 0;
    if (valid) {
      const VisitInfo I = ld_visit_lane(a.P, V, a.lens_length, v).I;
      if (I.redistribute) {
        const uint32_t seeds = ld_seed_count(a.P, (uint32_t)I.samples);
        words = ((unsigned long long)seeds + 31ull) / 32ull;
        if (seeds > most) most = seeds;
      }
    }
    unsigned long long incl = words;
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long t = __shfl_up(incl, off);
      if ((int)lane >= off) incl += t;
    }
    const unsigned long long total = ld_readlane(incl, 63);
    unsigned long long base = 0;
    if (lane == 0u && total) base = atomicAdd(&b.x[0], total);
    base = ld_readlane(base, 0);
    if (valid) {
      LdVisitState s;
      s.off = (uint32_t)(base + incl - words);       // (the host refuses a store of 2^27 words or more per array)
      s.k0 = words ? 0u : kLdSettled;
      s.accepted = 0u; s.pad = 0u;
      b.st[v - a.v_begin] = s;
    }
  }
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long t = __shfl_down(most, off); most = t > most ? t : most; }
  if (lane == 0u && most) atomicMax(&b.x[1], most);
}

// behind the list kernel of a turn: the count the callback reads never exceeds the buffers (what lay beyond took its A bit back)
__global__ void ld_probe_clamp_kernel(unsigned int *count, uint32_t cap, unsigned long long *x) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned int n = *count;
    x[3] = n;
    if (n > cap) *count = cap;
  }
}

// behind the callback: every listed seed has its answer now.  The answer bytes are left zero, as the next list's callback is
// promised them; the occluded ones are counted by wave ballot, one atomic per wave.
__global__ __launch_bounds__(256) void ld_probe_apply_kernel(ListProbeArgs b, const uint32_t *idx, uint8_t *answers, const unsigned int *count, uint32_t cap) {
  const uint32_t n_raw = *count;
  const uint32_t n = n_raw < cap ? n_raw : cap;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t n_up = ((uint64_t)n + 63u) & ~63ull;       // (whole waves go round the loop together)
  uint32_t wave_occ = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
    bool occ = false;
    if (i < n) {
      const uint32_t bit_at = idx[i];
      const uint32_t bit = 1u << (bit_at & 31u);
      occ = answers[i] != 0;
      atomicOr(&b.B[bit_at >> 5], bit);
      if (occ) { atomicAnd(&b.A[bit_at >> 5], ~bit); answers[i] = 0; }
    }
    wave_occ += (uint32_t)__builtin_popcountll(__ballot(occ));
  }
  if ((threadIdx.x & 63u) == 0u && wave_occ) atomicAdd(&b.x[2], (unsigned long long)wave_occ);
}

// a.ctr: [0] the ticket (reset every turn), [1] accepted draws and [2] attempts made (both run over the turns),
// [3] the visits this turn left unsettled (reset every turn).  pr: the turn's list (seg, idx, cap, count) and the camera-to-world.
// The probed list's seed answers (trace_attempt's policy): the visit's words of the answer store.  A visit seen from the
// skydome is `exempt`: nothing of it is occluded, nothing is asked.  A, whose bits the asking lanes of this very turn set
// (atomicOr), is read by a relaxed agent-scope atomic load.
struct SeedAnswers {
  const uint32_t *A, *B;
  bool exempt;
  LD_DEV void look(uint32_t m, bool &occluded, bool &known) const {
    occluded = false; known = true;
    if (!exempt) {
      const uint32_t bit = 1u << (m & 31u);
      const bool sa = (__hip_atomic_load(&A[m >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) != 0u;
      const bool sb = (B[m >> 5] & bit) != 0u;
      occluded = sb && !sa;
      known = sb;
    }
  }
};

// One turn's probed walk: list_draws_probed_spectral_kernel calls it, list_draws_probed_kernel behind it has it written out
// (see there).  Lam: as ld_walk takes it; a visit that a later turn resumes at k_first != 0 stages its row again like any other
// -- nothing of a wave survives a turn.  A segment asked about does not depend on the wavelength; which seeds get through the
// lens does.
template <class LensT, bool kTables, bool PO, class Lam>
LD_DEV void ld_probed_walk(const ListDrawArgs &a, const ProbeArgs &pr, const ListProbeArgs &b, const DevTerm *s_terms, const DevLens *s_k,
                           const Lam &lam) {
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = s_k;
  lam.bind(L);
  const lentil_params &P = a.P;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long n_groups = (a.v_end - a.v_begin + 63u) / 64u;
  unsigned long long wave_attempts = 0, wave_open = 0;
  for (;;) {
    const unsigned long long g = ld_take_ticket(&a.ctr[0], lane);
    if (g >= n_groups) break;
    // ---- the visits of the group that are not settled, lane = visit
    const uint64_t v = a.v_begin + g * 64u + lane;
    LdVisitState S;
    S.off = 0u; S.k0 = kLdSettled; S.accepted = 0u; S.pad = 0u;
    if (v < a.v_end) S = b.st[v - a.v_begin];
    const bool open = S.k0 != kLdSettled;
    unsigned long long todo = __ballot(open);      // (a group with nothing open falls through the empty loop below)
    LdVisitLane x{};
    uint32_t exempt_u = 0u;
    double lam_v = 0.0;
    if (open) {
      x = ld_visit_lane(P, a.V, a.lens_length, v);
      exempt_u = probe_from_skydome(x.pos_z) ? 1u : 0u;
      lam_v = lam.read(v - a.v_begin);                                   // (indexed by the range, not by the stream)
    }
    // ---- the set lanes one after another, lane = attempt
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const LdWaveVisit w = ld_broadcast_visit(x, src, (uint32_t)(a.v_begin + g * 64u));
      const uint32_t samples = w.samples, max_total = w.max_total;
      const uint32_t off = ld_readlane(S.off, src);
      const uint32_t k_first = ld_readlane(S.k0, src);
      const float org[3] = {ld_readlane(x.pos_z.x, src), ld_readlane(x.pos_z.y, src), ld_readlane(x.pos_z.z, src)};
      const float time = ld_readlane(x.raydir_time.w, src);
      const SeedAnswers seeds{b.A + off, b.B + off, ld_readlane(exempt_u, src) != 0u};
      // the visit's wavelength, staged in every turn that walks the visit (k_first != 0 too)
      if constexpr (Lam::kStaged) lam.stage(ld_readlane(lam_v, src), a.lambda, lane);
      uint32_t accepted = ld_readlane(S.accepted, src);                  // exact while `clean`
      uint32_t bound = accepted;                                         // what the accepted count can be at most
      uint32_t made = 0, k_resume = k_first;
      bool clean = true;                                                 // every slab so far is final
      for (uint32_t k0 = k_first; k0 < max_total && bound < samples; k0 = ld_next_slab(k0, max_total)) {
        const uint32_t attempt = k0 + lane;
        const bool commit = max_total - k0 > lane;
        // a pass at a seed whose answer is not known leaves the lane dirty: what the attempt comes to is open
        const AttemptTrace t = trace_attempt<PO>(P, L, a.bokeh, w.cs, w.px, w.py, attempt, commit, seeds);
        const bool dirty = t.open;
        const uint32_t pend_m = attempt + (uint32_t)t.tries;

        // ---- who asks: the dirty lanes the reference reaches whatever the open answers are
        const bool success = commit && !dirty && t.code < LENTIL_POINT_OUTSIDE;
        const unsigned long long okm = __ballot(success);
        const unsigned long long dm = __ballot(dirty);
        const bool ask = dirty && bound + (uint32_t)__builtin_popcountll((okm | dm) & below) < samples;
        const unsigned long long am = __ballot(ask);
        if (am) {
          clean = false;
          probe_ask_seed(P, pr, ask, b.A + off + (pend_m >> 5), 1u << (pend_m & 31u), off * 32u + pend_m, a.V.cam, time, org, t.lx, t.ly, lane);
        }
        if (clean) {
          // ---- the reference's selection, as ld_walk makes it
          const bool take = success && accepted + (uint32_t)__builtin_popcountll(okm & below) < samples;
          const unsigned long long tm = __ballot(take);
          if (tm) {
            const unsigned long long slot = list_wave_slot(&a.ctr[1], tm, lane);
            if (take) ld_store_draw(a, slot, w.visit, attempt, t.code, t.tries, t.xy0, t.xy1);
          }
          accepted += (uint32_t)__builtin_popcountll(tm);
          bound = accepted;
          made = ld_made(k0, max_total, accepted >= samples, (uint32_t)(63 - __builtin_clzll(tm | 1ull)));
          k_resume = ld_next_slab(k0, max_total);
        } else {
          bound += (uint32_t)__builtin_popcountll(okm | dm);
        }
      }
      if (clean) wave_attempts += made; else ++wave_open;
      if ((int)lane == src) {
        LdVisitState s;
        s.off = off; s.k0 = clean ? kLdSettled : k_resume; s.accepted = accepted; s.pad = 0u;
        b.st[v - a.v_begin] = s;
      }
    }
  }
  ld_add_wave_sum(&a.ctr[2], wave_attempts, lane);
  ld_add_wave_sum(&a.ctr[3], wave_open, lane);
}

// a.ctr, pr, b: as above the walk, one launch per turn.  What ld_probed_walk is under FixedLambda, written out: as a call of
// ld_probed_walk the probed list of the compiled-in double gauss measured about 2 % slower than this loop, outside the range
// of the loop's own runs (profiles/one_loop_kernels.txt), and its SGPR spills rose.  A change to the walk above is made here too.
template <class LensT, bool kTables, bool PO>
__global__ __launch_bounds__(kLdBlock) void list_draws_probed_kernel(ListDrawArgs a, ProbeArgs pr, ListProbeArgs b) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  if (PO) {
    stage_lens<kTables>(a.lens, a.terms, a.lambda, kLdBlock, s_terms, &s_k, threadIdx.x == 0);
    __syncthreads();
  }
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  L.k = &s_k;
  const lentil_params &P = a.P;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long n_groups = (a.v_end - a.v_begin + 63u) / 64u;
  unsigned long long wave_attempts = 0, wave_open = 0;
  for (;;) {
    const unsigned long long g = ld_take_ticket(&a.ctr[0], lane);
    if (g >= n_groups) break;
    // ---- the visits of the group that are not settled, lane = visit
    const uint64_t v = a.v_begin + g * 64u + lane;
    LdVisitState S;
    S.off = 0u; S.k0 = kLdSettled; S.accepted = 0u; S.pad = 0u;
    if (v < a.v_end) S = b.st[v - a.v_begin];
    const bool open = S.k0 != kLdSettled;
    unsigned long long todo = __ballot(open);      // (a group with nothing open falls through the empty loop below)
    LdVisitLane x{};
    uint32_t exempt_u = 0u;
    if (open) {
      x = ld_visit_lane(P, a.V, a.lens_length, v);
      exempt_u = probe_from_skydome(x.pos_z) ? 1u : 0u;
    }
    // ---- the set lanes one after another, lane = attempt
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const LdWaveVisit w = ld_broadcast_visit(x, src, (uint32_t)(a.v_begin + g * 64u));
      const uint32_t samples = w.samples, max_total = w.max_total;
      const uint32_t off = ld_readlane(S.off, src);
      const uint32_t k_first = ld_readlane(S.k0, src);
      const float org[3] = {ld_readlane(x.pos_z.x, src), ld_readlane(x.pos_z.y, src), ld_readlane(x.pos_z.z, src)};
      const float time = ld_readlane(x.raydir_time.w, src);
      const SeedAnswers seeds{b.A + off, b.B + off, ld_readlane(exempt_u, src) != 0u};
      uint32_t accepted = ld_readlane(S.accepted, src);                  // exact while `clean`
      uint32_t bound = accepted;                                         // what the accepted count can be at most
      uint32_t made = 0, k_resume = k_first;
      bool clean = true;                                                 // every slab so far is final
      for (uint32_t k0 = k_first; k0 < max_total && bound < samples; k0 = ld_next_slab(k0, max_total)) {
        const uint32_t attempt = k0 + lane;
        const bool commit = max_total - k0 > lane;
        // a pass at a seed whose answer is not known leaves the lane dirty: what the attempt comes to is open
        const AttemptTrace t = trace_attempt<PO>(P, L, a.bokeh, w.cs, w.px, w.py, attempt, commit, seeds);
        const bool dirty = t.open;
        const uint32_t pend_m = attempt + (uint32_t)t.tries;

        // ---- who asks: the dirty lanes the reference reaches whatever the open answers are
        const bool success = commit && !dirty && t.code < LENTIL_POINT_OUTSIDE;
        const unsigned long long okm = __ballot(success);
        const unsigned long long dm = __ballot(dirty);
        const bool ask = dirty && bound + (uint32_t)__builtin_popcountll((okm | dm) & below) < samples;
        const unsigned long long am = __ballot(ask);
        if (am) {
          clean = false;
          // (probe_ask_seed's lines, in place: the call leaves this kernel with other code than the measured one)
          bool win = false;
          const uint32_t bit = 1u << (pend_m & 31u);
          uint32_t *wa = b.A + off + (pend_m >> 5);
          if (ask) win = (atomicOr(wa, bit) & bit) == 0u;
          const unsigned long long wm = __ballot(win);
          if (wm) {
            const uint32_t slot = probe_wave_slot(pr.count, wm, lane);
            if (win) {
              if (slot < pr.cap) {
                float c2w[4][4];
                probe_cam_to_world(a.V.cam, pr, time, c2w);
                float tgt[3];
                probe_target(P, c2w, t.lx, t.ly, 0.0f, tgt);
                lentil_probe_segment sg;
                sg.origin[0] = org[0]; sg.origin[1] = org[1]; sg.origin[2] = org[2];
                sg.target[0] = tgt[0]; sg.target[1] = tgt[1]; sg.target[2] = tgt[2];
                pr.seg[slot] = sg;
                pr.idx[slot] = off * 32u + pend_m;
              } else {
                atomicAnd(wa, ~bit);
              }
            }
          }
        }
        if (clean) {
          // ---- the reference's selection, as ld_walk makes it
          const bool take = success && accepted + (uint32_t)__builtin_popcountll(okm & below) < samples;
          const unsigned long long tm = __ballot(take);
          if (tm) {
            const unsigned long long slot = list_wave_slot(&a.ctr[1], tm, lane);
            if (take) ld_store_draw(a, slot, w.visit, attempt, t.code, t.tries, t.xy0, t.xy1);
          }
          accepted += (uint32_t)__builtin_popcountll(tm);
          bound = accepted;
          made = ld_made(k0, max_total, accepted >= samples, (uint32_t)(63 - __builtin_clzll(tm | 1ull)));
          k_resume = ld_next_slab(k0, max_total);
        } else {
          bound += (uint32_t)__builtin_popcountll(okm | dm);
        }
      }
      if (clean) wave_attempts += made; else ++wave_open;
      if ((int)lane == src) {
        LdVisitState s;
        s.off = off; s.k0 = clean ? kLdSettled : k_resume; s.accepted = accepted; s.pad = 0u;
        b.st[v - a.v_begin] = s;
      }
    }
  }
  ld_add_wave_sum(&a.ctr[2], wave_attempts, lane);
  ld_add_wave_sum(&a.ctr[3], wave_open, lane);
}

// the probed list with a wavelength per visit (lentil_hip_list_draws_spectral with LENTIL_DRAWS_PROBED)
template <class LensT, bool kTables>
__global__ __launch_bounds__(kLdBlock) void list_draws_probed_spectral_kernel(ListDrawArgs a, ProbeArgs pr, ListProbeArgs b, const double *lambdas) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k;
  __shared__ double s_lp[kLdBlock / 64][kMaxExp + 1];
  stage_lens<kTables>(a.lens, a.terms, a.lambda, kLdBlock, s_terms, &s_k, threadIdx.x == 0);
  __syncthreads();
  ld_probed_walk<LensT, kTables, true>(a, pr, b, s_terms, &s_k, WaveLambda{lambdas, s_lp[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]});
}

// ---------------------------------------------------------------------------------------
// LENTIL_DRAWS_CHANNELS: polynomial optics with abb_chromatic != 0 (src/lentil_filter.cpp:248-299).  Attempt n traces three
// colour channels with the same seeds n + try, each with its own vignetting_retries + 1 tries and its own wavelength.  Every
// channel that gets through the lens and lands in the frame is a draw; every one that does not takes one off `count`, and the
// attempt itself adds one: count += successes - 2, a signed count that may go down and below zero.  The loop runs while
// count < samples and n < 5 * samples; steps are at most +1, so `samples` is hit exactly, and an attempt is made iff every
// running count before it was below `samples` (accept_item_chroma, lentil_kernels.h, selects the same way over the pass's
// result pool).  A visit yields up to 11 * samples records: count_final + 2 * attempts.
//
// list_draws_chroma_kernel: list_draws_kernel's walk (the ld_* helpers).  Per slab every lane traces its attempt once per
// channel -- trace_attempt, called in the channel loop -- through one of three DevLens copies in LDS, each staged
// (stage_lens) for its channel's wavelength.  With abb_chromatic < 0 the three channels share one
// wavelength and the three traces are the same trace: it runs once (a wave-uniform decision) and stands for all three.
// Selection: delta = successes - 2 on the lanes that commit, a signed inclusive prefix over the wave, running = count + prefix;
// istar is the first lane whose running count reaches `samples`; the lanes up to istar were executed (all committed lanes if
// none reaches it).  Their channels' records take consecutive slots through one atomic per slab (list_wave_slot3) and carry
// the channel in bits 30-31 of `attempt`, as the pass's draw log does.  `count` is carried across slabs as int32.
// Every loop is bounded as in list_draws_kernel, the channel loop by 3.
// ---------------------------------------------------------------------------------------
struct ListChromaArgs {
  double lambda[3];                 // lentil_hip_draw_channels' wavelengths
  uint32_t n_traces;                // 3: a trace per channel; 1: the channels share their wavelength, one trace stands for all
};

// One wave's wanted records -- up to three per lane, a mask per channel -- take consecutive slots of the list through one
// atomic; a lane's own records lie side by side, channel 0 first.  Called by the whole wave, some mask != 0.  -> the lane's
// first slot.
LD_DEV unsigned long long list_wave_slot3(unsigned long long *count, unsigned long long m0, unsigned long long m1,
                                          unsigned long long m2, uint32_t lane) {
  const unsigned long long below = (1ull << lane) - 1ull;
  const int first = __builtin_ctzll(m0 | m1 | m2);
  unsigned long long base = 0;
  if ((int)lane == first)
    base = atomicAdd(count, (unsigned long long)(__builtin_popcountll(m0) + __builtin_popcountll(m1) + __builtin_popcountll(m2)));
  base = ld_readlane(base, first);
  return base + (unsigned long long)(__builtin_popcountll(m0 & below) + __builtin_popcountll(m1 & below) + __builtin_popcountll(m2 & below));
}

// LensT / kTables: LdsLens with the term table staged into LDS (the interpreter) or GenLens<Gen> of a compiled-in lens.
template <class LensT, bool kTables>
__global__ __launch_bounds__(kLdBlock) void list_draws_chroma_kernel(ListDrawArgs a, ListChromaArgs ch) {
  __shared__ DevTerm s_terms[kTables ? kMaxTerms : 1];
  __shared__ DevLens s_k[3];
  {
    const uint32_t c = threadIdx.x < 3u ? threadIdx.x : 0u;       // a slot per channel, filled by threads 0 ... 2
    stage_lens<kTables>(a.lens, a.terms, ch.lambda[c], kLdBlock, s_terms, &s_k[c], threadIdx.x < 3u);
  }
  __syncthreads();
  LensT L{};
  if constexpr (kTables) L.terms = s_terms;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long n_groups = (a.v_end - a.v_begin + 63u) / 64u;
  const uint32_t n_traces = ch.n_traces == 3u ? 3u : 1u;
  const double qnan = __builtin_nan("");
  unsigned long long wave_attempts = 0;
  for (;;) {
    const unsigned long long g = ld_take_ticket(&a.ctr[0], lane);
    if (g >= n_groups) break;
    // ---- the prologue, lane = visit
    const uint64_t v = a.v_begin + g * 64u + lane;
    LdVisitLane x{};
    if (v < a.v_end) x = ld_visit_lane(a.P, a.V, a.lens_length, v);
    unsigned long long todo = __ballot(x.I.redistribute);
    // ---- the set lanes one after another, lane = attempt
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const LdWaveVisit w = ld_broadcast_visit(x, src, (uint32_t)(a.v_begin + g * 64u));
      const uint32_t samples = w.samples, max_total = w.max_total, visit = w.visit;     // (the host keeps 5 * samples + retries below 2^30)
      int32_t count = 0;                                                 // the reference's `count`: signed, may go down
      uint32_t made = 0;
      for (uint32_t k0 = 0; k0 < max_total && count < (int32_t)samples; k0 = ld_next_slab(k0, max_total)) {
        const uint32_t attempt = k0 + lane;
        const bool commit = max_total - k0 > lane;

        uint32_t code0 = LENTIL_POINT_VIGNETTED, code1 = LENTIL_POINT_VIGNETTED, code2 = LENTIL_POINT_VIGNETTED;
        double xa0 = qnan, xb0 = qnan, xa1 = qnan, xb1 = qnan, xa2 = qnan, xb2 = qnan;
        int tries0 = 0, tries1 = 0, tries2 = 0;
#pragma unroll 1
        for (uint32_t c = 0; c < n_traces; ++c) {
          L.k = &s_k[c];
          const AttemptTrace t = trace_attempt<true>(a.P, L, a.bokeh, w.cs, w.px, w.py, attempt, commit, NoSeedAnswers{});
          // (selects, not an indexed array: the results stay in registers)
          if (c == 0u) { code0 = t.code; xa0 = t.xy0; xb0 = t.xy1; tries0 = t.tries; }
          if (c == 1u) { code1 = t.code; xa1 = t.xy0; xb1 = t.xy1; tries1 = t.tries; }
          if (c == 2u) { code2 = t.code; xa2 = t.xy0; xb2 = t.xy1; tries2 = t.tries; }
        }
        if (n_traces == 1u) {
          code1 = code2 = code0; xa1 = xa2 = xa0; xb1 = xb2 = xb0; tries1 = tries2 = tries0;
        }

        // ---- the reference's selection: count += successes - 2 per attempt, until it reaches `samples`
        const bool ok0 = commit && code0 < LENTIL_POINT_OUTSIDE;
        const bool ok1 = commit && code1 < LENTIL_POINT_OUTSIDE;
        const bool ok2 = commit && code2 < LENTIL_POINT_OUTSIDE;
        const int delta = commit ? (ok0 ? 1 : 0) + (ok1 ? 1 : 0) + (ok2 ? 1 : 0) - 2 : 0;
        int incl = delta;
        for (int off = 1; off < 64; off <<= 1) {
          const int up = __shfl_up(incl, off);
          if ((int)lane >= off) incl += up;
        }
        const int running = count + incl;                               // the count behind this lane's attempt
        const unsigned long long rmask = __ballot(commit && running >= (int32_t)samples);
        const int istar = rmask ? __builtin_ctzll(rmask) : 63;          // (lanes that do not commit have delta 0: lane 63 holds the slab's sum)
        const bool executed = commit && (int)lane <= istar;
        const unsigned long long m0 = __ballot(executed && ok0), m1 = __ballot(executed && ok1), m2 = __ballot(executed && ok2);
        if (m0 | m1 | m2) {
          unsigned long long slot = list_wave_slot3(&a.ctr[1], m0, m1, m2, lane);
          if (executed && ok0) ld_store_draw(a, slot++, visit, attempt, code0, tries0, xa0, xb0);
          if (executed && ok1) ld_store_draw(a, slot++, visit, attempt | (1u << 30), code1, tries1, xa1, xb1);
          if (executed && ok2) ld_store_draw(a, slot, visit, attempt | (2u << 30), code2, tries2, xa2, xb2);
        }
        count = __builtin_amdgcn_readlane(running, istar);
        made = ld_made(k0, max_total, rmask != 0ull, (uint32_t)istar);
      }
      wave_attempts += made;
    }
  }
  ld_add_wave_sum(&a.ctr[2], wave_attempts, lane);
}
