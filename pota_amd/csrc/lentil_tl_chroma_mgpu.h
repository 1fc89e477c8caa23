// lentil_tl_chroma_mgpu.h -- thin lens with abb_chromatic > 0 walked in parallel, in the single-threaded draw order, over
// any number of ranks.  Included by lentil_hip.hip after lentil_kernels.h (the tl_chroma_* kernels there).
//
// Upstream every attempt that survives the optical vignetting test draws its colour channel from ONE xor128 stream
// (src/lentil_filter.cpp:393-406, src/global.h:22-27); the channel decides whether the draw lands in the frame, hence how
// many attempts the item makes and how many generator outputs it uses up.  tl_chroma_walk_kernel follows that chain with
// one block.  Two facts make it parallel:
//   1. Call a surviving attempt slot *uniform* when all three channels land in the frame, or all three land out.  When
//      every surviving slot up to the one at which the item reaches `samples` successes (or up to its last slot) is
//      uniform, the number D of outputs the item consumes does not depend on the generator state
//      (tl_chroma_count_kernel).  The other items are *dependent*: near the frame's border with a large chromatic shift.
//   2. xor128 is linear over GF(2)^128: k outputs ahead is a product with the matrices T^(2^j) of the set bits of k
//      (xor128_jump).
// The dependent items are walked in visit order by one wave (tl_chroma_chain_kernel) from 4-bit signatures of their slots
// (survives, and per channel: lands in the frame), jumping over the independent items between them: one anchor state
// after each.  Every item then starts from jump(anchor before it, D summed since) and is walked on its own
// (tl_chroma_walk_par_kernel).  The host side (which items, the exchange between ranks) is in lentil_comm.h.
#pragma once

constexpr uint64_t kTlcDependent = 1ull << 63;        // tl_chroma_count_kernel: the item's D depends on the channels drawn
constexpr uint64_t kTlcNoSig = ~0ull;                 // tl_chroma_sig_kernel: no signature wanted

// ---- the jump tables (host): rows of T^(2^j), j < 64; row r (uint4: words x, y, z, w of a 128-bit mask) gives output bit r
// (word r / 32, bit r % 32) as the parity of the row AND the state
static void xor128_step_words(uint32_t s[4]) {
  const uint32_t t = s[0] ^ (s[0] << 11);
  s[0] = s[1]; s[1] = s[2]; s[2] = s[3];
  s[3] = s[3] ^ (s[3] >> 19) ^ t ^ (t >> 8);
}
static const std::vector<uint32_t> &xor128_jump_rows() {
  static const std::vector<uint32_t> rows = [] {
    // columns: col[i] = the matrix applied to unit vector i; T's from one step of the generator (linear)
    std::vector<uint32_t> col(128 * 4), sq(128 * 4), out((size_t)64 * 128 * 4, 0u);
    for (int i = 0; i < 128; ++i) {
      uint32_t s[4] = {0, 0, 0, 0};
      s[i >> 5] = 1u << (i & 31);
      xor128_step_words(s);
      memcpy(&col[(size_t)i * 4], s, sizeof s);
    }
    for (int j = 0; j < 64; ++j) {
      for (int i = 0; i < 128; ++i)
        for (int r = 0; r < 128; ++r)
          if (col[(size_t)i * 4 + (r >> 5)] >> (r & 31) & 1u) out[((size_t)j * 128 + r) * 4 + (i >> 5)] |= 1u << (i & 31);
      // squared: column i of M M = M applied to column i of M
      for (int i = 0; i < 128; ++i) {
        uint32_t v[4] = {0, 0, 0, 0};
        for (int k = 0; k < 128; ++k)
          if (col[(size_t)i * 4 + (k >> 5)] >> (k & 31) & 1u)
            for (int w = 0; w < 4; ++w) v[w] ^= col[(size_t)k * 4 + w];
        memcpy(&sq[(size_t)i * 4], v, sizeof v);
      }
      col.swap(sq);
    }
    return out;
  }();
  return rows;
}
constexpr size_t kXorJumpBytes = (size_t)64 * 128 * 16;

// ---- device ---------------------------------------------------------------------------------------------------------------
// `steps` outputs ahead of state s.  The whole wave calls it with the same s and steps; lane l evaluates rows l and 64 + l
// of each matrix, the ballots assemble the new state.
LD_DEV uint4 xor128_jump(uint4 s, uint64_t steps, const uint4 *tab, uint32_t lane) {
  while (steps) {
    const uint32_t j = (uint32_t)__builtin_ctzll(steps);
    steps &= steps - 1ull;
    const uint4 r0 = tab[j * 128u + lane], r1 = tab[j * 128u + 64u + lane];
    const uint32_t p0 = (uint32_t)__builtin_popcount((r0.x & s.x) ^ (r0.y & s.y) ^ (r0.z & s.z) ^ (r0.w & s.w)) & 1u;
    const uint32_t p1 = (uint32_t)__builtin_popcount((r1.x & s.x) ^ (r1.y & s.y) ^ (r1.z & s.z) ^ (r1.w & s.w)) & 1u;
    const unsigned long long b0 = __ballot(p0 != 0u), b1 = __ballot(p1 != 0u);
    s = make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
  }
  return s;
}

// lentil_hip_test_xor128_jump: one wave
__global__ __launch_bounds__(64) void xor128_jump_test_kernel(const uint4 *tab, uint4 *s, uint64_t steps) {
  const uint4 r = xor128_jump(s[0], steps, tab, threadIdx.x & 63u);
  if (threadIdx.x == 0) s[0] = r;
}

// One wave step of the walk: the 64 attempt slots n .. n + step_n - 1 of an item, this lane's slot surviving or not and
// `ok` (bit c: channel c lands in the frame).  Draws the channels from state st in slot order, ranks the successes after
// the item's `acc` so far, stops at the S-th.  st moves past the outputs the made attempts consumed.  (The block-wide form
// of the same bookkeeping is inside tl_chroma_walk_kernel: keep the two in step.)
struct TlWaveStep {
  int channel;          // this lane's channel (surviving slots)
  bool succ, take;      // its draw lands in the frame / is accepted
  uint32_t executed;    // attempts of the step that are made
  uint32_t taken;       // successes accepted
  bool last;            // the item reached S successes in this step
};
LD_DEV TlWaveStep tl_chroma_wave_step(uint4 &st, bool surv, uint32_t ok, uint32_t acc, uint32_t S, uint32_t step_n, uint32_t lane) {
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  const unsigned long long vm = __ballot(surv);
  const uint32_t xi = (uint32_t)__builtin_popcountll(vm & lt_mask), vtotal = (uint32_t)__builtin_popcountll(vm);
  // the step's outputs: every lane runs the generator, keeps the output of its slot and the state after output #lane
  uint32_t x = st.x, y = st.y, z = st.z, w = st.w, mine = 0;
  uint4 after = st;
  for (uint32_t i = 0; i < vtotal; ++i) {
    const uint32_t v = xor128_next(x, y, z, w);
    if (i == xi) mine = v;
    if (i == lane) after = make_uint4(x, y, z, w);
  }
  TlWaveStep r;
  r.channel = surv ? tl_chroma_channel(mine) : 0;
  r.succ = surv && ((ok >> (uint32_t)(r.channel + 1)) & 1u);
  const unsigned long long sm = __ballot(r.succ);
  const uint32_t rank = acc + (uint32_t)__builtin_popcountll(sm & lt_mask);
  r.take = r.succ && rank < S;
  const unsigned long long lm = __ballot(r.take && rank + 1u == S);
  r.last = lm != 0ull;
  r.executed = r.last ? (uint32_t)__builtin_ctzll(lm) + 1u : step_n;
  const unsigned long long ex = r.executed >= 64u ? ~0ull : ((1ull << r.executed) - 1ull);
  const uint32_t consumed = (uint32_t)__builtin_popcountll(vm & ex);
  const uint32_t taken = (uint32_t)__builtin_popcountll(sm & ex);
  r.taken = taken < S - acc ? taken : S - acc;
  if (consumed) {
    const int src = (int)consumed - 1;
    st = make_uint4((uint32_t)__shfl((int)after.x, src), (uint32_t)__shfl((int)after.y, src),
                    (uint32_t)__shfl((int)after.z, src), (uint32_t)__shfl((int)after.w, src));
  }
  return r;
}

// 4-bit signature of attempt slot m: bit 0 survives the vignetting test, bit 1 + c channel c lands in the frame
LD_DEV uint32_t tl_chroma_nibble(const uint32_t *res, uint32_t m) {
  const uint32_t c0 = res[m * 3ull], c1 = res[m * 3ull + 1], c2 = res[m * 3ull + 2];
  if (c0 == kCodeFail && c1 == kCodeFail && c2 == kCodeFail) return 0u;
  return 1u | (c0 < kCodeOut ? 2u : 0u) | (c1 < kCodeOut ? 4u : 0u) | (c2 < kCodeOut ? 8u : 0u);
}

struct TlChromaPar {
  const uint4 *jump;              // [64][128] rows of T^(2^j)
  const uint4 *base;              // states the items start from, after a jump
  const uint32_t *base_idx;       // [n_items] which of them (null: base[item])
  const uint64_t *offset;         // [n_items] outputs to jump over from there (null: none)
  uint4 *entry_out;               // [n_items] the entry state each item walked from (null: not kept)
  uint64_t *val;                  // count: [n_items] D, or kTlcDependent | slots
  const uint64_t *sig_off;        // signatures: [n_items] first word of the item's signature in sig (kTlcNoSig: none)
  uint32_t *sig;                  // 8 slots per word, slot k in bits 4 (k % 8) ..
};

// One wave per item: D, or the item is dependent (a surviving slot whose channels disagree, before the item is through).
__global__ __launch_bounds__(256) void tl_chroma_count_kernel(TlChromaArgs a, TlChromaPar q) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  for (uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6); item < a.n_items; item += gridDim.x * 4u) {
    const uint32_t S = a.work[item].y, max_total = S * 5u;
    const uint32_t *res = a.res + a.att_off[item] * 3ull;
    uint32_t n = 0, acc = 0;
    uint64_t D = 0;
    bool dep = false;
    while (acc < S && n < max_total) {
      const uint32_t my_n = n + lane;
      const uint32_t nib = my_n < max_total ? tl_chroma_nibble(res, my_n) : 0u;
      const bool surv = nib & 1u, all_in = nib == 15u, mixed = surv && nib != 1u && nib != 15u;
      const unsigned long long vm = __ballot(surv), im = __ballot(all_in), mm = __ballot(mixed);
      const uint32_t rank = acc + (uint32_t)__builtin_popcountll(im & lt_mask);
      const unsigned long long lm = __ballot(all_in && rank + 1u == S);
      const uint32_t step_n = (max_total - n) < 64u ? (max_total - n) : 64u;
      const uint32_t executed = lm ? (uint32_t)__builtin_ctzll(lm) + 1u : step_n;
      const unsigned long long ex = executed >= 64u ? ~0ull : ((1ull << executed) - 1ull);
      if (mm & ex) { dep = true; break; }
      D += (uint64_t)__builtin_popcountll(vm & ex);
      acc += (uint32_t)__builtin_popcountll(im & ex);
      n += executed;
      if (lm) break;
    }
    if (lane == 0) q.val[item] = dep ? (kTlcDependent | max_total) : D;
  }
}

// One wave per item with a signature wanted: its slots' nibbles, packed at q.sig + q.sig_off[item].
__global__ __launch_bounds__(256) void tl_chroma_sig_kernel(TlChromaArgs a, TlChromaPar q) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6); item < a.n_items; item += gridDim.x * 4u) {
    const uint64_t off = q.sig_off[item];
    if (off == kTlcNoSig) continue;
    const uint32_t max_total = a.work[item].y * 5u, words = (max_total + 7u) / 8u;
    const uint32_t *res = a.res + a.att_off[item] * 3ull;
    for (uint32_t n = 0; n < max_total; n += 64u) {
      const uint32_t my_n = n + lane;
      uint32_t v = (my_n < max_total ? tl_chroma_nibble(res, my_n) : 0u) << (4u * (lane & 7u));
      v |= (uint32_t)__shfl_xor((int)v, 1);
      v |= (uint32_t)__shfl_xor((int)v, 2);
      v |= (uint32_t)__shfl_xor((int)v, 4);
      const uint32_t wi = (n >> 3) + (lane >> 3);
      if ((lane & 7u) == 0u && wi < words) q.sig[off + wi] = v;
    }
  }
}

// The dependent items of the frame in visit order, one wave: jump over the independent outputs before each (skip[d]),
// walk its signature as tl_chroma_walk_kernel would, and keep the state after it.  anchor[0]: the pass's entry state (in);
// anchor[1 + d]: the state after dependent item d; skip[n_dep]: the outputs after the last one, to the frame's end.
struct TlChainArgs {
  const uint4 *jump;
  uint4 *anchor;                  // [n_dep + 1]
  uint32_t n_dep;
  const uint64_t *skip;           // [n_dep + 1]
  const uint64_t *sig_off;        // [n_dep] first word of each signature in sig
  const uint32_t *slots;          // [n_dep] attempt slots (5 samples)
  const uint32_t *sig;
  uint32_t *final_state;          // [4] the frame's last state
};
__global__ __launch_bounds__(64) void tl_chroma_chain_kernel(TlChainArgs c) {
  const uint32_t lane = threadIdx.x & 63u;
  uint4 st = c.anchor[0];
  for (uint32_t d = 0; d < c.n_dep; ++d) {
    st = xor128_jump(st, c.skip[d], c.jump, lane);
    const uint32_t max_total = c.slots[d], S = max_total / 5u;
    const uint32_t *sig = c.sig + c.sig_off[d];
    uint32_t n = 0, acc = 0;
    while (acc < S && n < max_total) {
      const uint32_t my_n = n + lane;
      const uint32_t nib = my_n < max_total ? (sig[my_n >> 3] >> (4u * (my_n & 7u))) & 15u : 0u;
      const uint32_t step_n = (max_total - n) < 64u ? (max_total - n) : 64u;
      const TlWaveStep r = tl_chroma_wave_step(st, nib & 1u, nib >> 1, acc, S, step_n, lane);
      acc += r.taken;
      n += r.executed;
      if (r.last) break;
    }
    if (lane == 0) c.anchor[1 + d] = st;
  }
  st = xor128_jump(st, c.skip[c.n_dep], c.jump, lane);
  if (lane == 0) { c.final_state[0] = st.x; c.final_state[1] = st.y; c.final_state[2] = st.z; c.final_state[3] = st.w; }
}

// One wave per item, every item from its own entry state: what tl_chroma_walk_kernel does for it, 64 attempts per step.
__global__ __launch_bounds__(256) void tl_chroma_walk_par_kernel(TlChromaArgs a, TlChromaPar q) {
  __shared__ uint32_t s_pix[4][64], s_same[4][64], s_ch[4][64], s_key[4][64];
  __shared__ float s_val[4][4 * LENTIL_MAX_AOVS + 1];
  __shared__ uint32_t s_off[4][4 * LENTIL_MAX_AOVS + 1];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long tot_attempted = 0, tot_accepted = 0;
  uint32_t rmin = 0x7FFFFFFFu, rmax_p1 = 0u;
  for (uint32_t item = blockIdx.x * 4u + wave; item < a.n_items; item += gridDim.x * 4u) {
    const ItemVisit h = load_work_visit(a.P, a.V, a.work[item], 0.0);
    const uint32_t S = h.samples, max_total = S * 5u;
    const unsigned long long zk = (a.F.zkey || a.F.zkey_dbg) ? closest_key_of(a.ctr, h.I.depth, visit_gid(a.V, h.visit)) : 0ull;
    const uint32_t *res = a.res + a.att_off[item] * 3ull;
    wave_sync_lds();                // (the previous item's splats have read the list)
    const uint32_t U = tl_chroma_item_values(a, h, lane, s_val[wave], s_off[wave]);
    wave_sync_lds();
    uint4 st = q.base[q.base_idx ? q.base_idx[item] : item];
    if (q.offset) st = xor128_jump(st, q.offset[item], q.jump, lane);
    if (q.entry_out && lane == 0) q.entry_out[item] = st;
    uint32_t n = 0, acc = 0;
    while (acc < S && n < max_total) {
      const uint32_t my_n = n + lane;
      uint32_t c0 = kCodeFail, c1 = kCodeFail, c2 = kCodeFail;      // (three scalars: an array indexed by the channel lives in scratch)
      if (my_n < max_total) { c0 = res[my_n * 3ull]; c1 = res[my_n * 3ull + 1]; c2 = res[my_n * 3ull + 2]; }
      const bool surv = !(c0 == kCodeFail && c1 == kCodeFail && c2 == kCodeFail);
      const uint32_t ok = (c0 < kCodeOut ? 1u : 0u) | (c1 < kCodeOut ? 2u : 0u) | (c2 < kCodeOut ? 4u : 0u);
      const uint32_t step_n = (max_total - n) < 64u ? (max_total - n) : 64u;
      const TlWaveStep r = tl_chroma_wave_step(st, surv, ok, acc, S, step_n, lane);
      const uint32_t pix = r.take ? (r.channel < 0 ? c0 : (r.channel == 0 ? c1 : c2)) : 0u;
      tl_chroma_accept_wave(a, h.visit, zk, r.take, pix, r.channel, my_n, lane, s_pix[wave], s_same[wave], s_ch[wave], s_key[wave],
                            s_val[wave], s_off[wave], U, rmin, rmax_p1);
      acc += r.taken;
      n += r.executed;
      if (r.last) break;
    }
    tot_attempted += n;            // total_samples_taken when the loop ends
    tot_accepted += acc;
  }
  if (lane == 0) {
    if (tot_attempted) atomicAdd(&a.ctr->attempted, tot_attempted);
    if (tot_accepted) atomicAdd(&a.ctr->accepted, tot_accepted);
  }
  flush_row_range(a.ctr, rmin, rmax_p1);
}
