// lentil_comm.h -- the exchange between the GPUs of one node, native: RCCL over xGMI, called through the C-ABI
// (lentil_hip_comm_* / _allreduce / _exchange_bands in include/lentil_hip.h).  Included by lentil_hip.hip.
//
// The reference has nothing like it (one process, threads sharing one set of buffers, src/lentil.h:823-851);
// SURVEY.md section 8(e) defines the step.  Two partitions, as in pota_amd/distributed.py, whose Python form of the
// same steps the world_size-2/3 gloo tests keep exercising:
//   interleaved rows + all-reduce   every rank holds the whole frame: closest-AOV winner keys are min-reduced
//                                   (ncclUint64 / ncclMin), winners gathered, then one sum all-reduce of the
//                                   accumulator block
//   row bands (tiled output)        touched rows all-gathered (one small ncclAllGather), what a rank added to
//                                   another's band goes there point to point -- a list of pixel entries when the rows
//                                   are mostly empty, packed rows otherwise -- the owner merges and resolves its band
// RCCL is loaded at run time (dlopen): liblentil_hip.so does not depend on it unless a communicator is asked for, and
// a process that already has an RCCL loaded (torch's) gets that same instance by soname.
#pragma once
#include <dlfcn.h>

typedef struct ncclComm *lentil_ncclComm_t;
struct LentilNcclId { char b[128]; };     // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES 128), passed by value
struct LentilRccl {
  void *lib = nullptr;
  int (*GetUniqueId)(void *id) = nullptr;
  int (*CommInitRank)(lentil_ncclComm_t *comm, int nranks, LentilNcclId id, int rank) = nullptr;
  int (*CommDestroy)(lentil_ncclComm_t comm) = nullptr;
  int (*AllReduce)(const void *s, void *r, size_t count, int dtype, int op, lentil_ncclComm_t comm, hipStream_t st) = nullptr;
  int (*AllGather)(const void *s, void *r, size_t sendcount, int dtype, lentil_ncclComm_t comm, hipStream_t st) = nullptr;
  int (*Send)(const void *s, size_t count, int dtype, int peer, lentil_ncclComm_t comm, hipStream_t st) = nullptr;
  int (*Recv)(void *r, size_t count, int dtype, int peer, lentil_ncclComm_t comm, hipStream_t st) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
// rccl.h: ncclSum 0, ncclMin 3; ncclInt8 0, ncclUint8 1, ncclInt64 4, ncclUint64 5, ncclFloat32 7
enum { kNcclSum = 0, kNcclMin = 3, kNcclUint8 = 1, kNcclInt64 = 4, kNcclUint64 = 5, kNcclFloat32 = 7 };

static LentilRccl g_rccl;
static std::mutex g_rccl_mutex;

static const char *load_rccl() {
  std::lock_guard<std::mutex> g(g_rccl_mutex);
  if (g_rccl.lib) return nullptr;
  const char *names[] = {getenv("LENTIL_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void *h = nullptr;
  for (const char *n : names) {
    if (!n || !n[0]) continue;
    h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (h) break;
  }
  if (!h) return "librccl.so not found (LENTIL_RCCL_LIB names it)";
  LentilRccl r;
  r.lib = h;
#define LENTIL_RCCL_SYM(field, name)                                \
  *(void **)(&r.field) = dlsym(h, name);                            \
  if (!r.field) return "librccl.so lacks " name;
  LENTIL_RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
  LENTIL_RCCL_SYM(CommInitRank, "ncclCommInitRank")
  LENTIL_RCCL_SYM(CommDestroy, "ncclCommDestroy")
  LENTIL_RCCL_SYM(AllReduce, "ncclAllReduce")
  LENTIL_RCCL_SYM(AllGather, "ncclAllGather")
  LENTIL_RCCL_SYM(Send, "ncclSend")
  LENTIL_RCCL_SYM(Recv, "ncclRecv")
  LENTIL_RCCL_SYM(GroupStart, "ncclGroupStart")
  LENTIL_RCCL_SYM(GroupEnd, "ncclGroupEnd")
  LENTIL_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef LENTIL_RCCL_SYM
  g_rccl = r;
  return nullptr;
}

struct LentilComm {
  lentil_ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  int64_t *d_meta_mine = nullptr, *d_meta_all = nullptr, *h_meta_all = nullptr;   // [2 + world] / [world][2 + world]
  std::vector<void *> scratch;          // grow-only device buffers, one per use slot
  std::vector<size_t> scratch_bytes;
  uint64_t last_sent = 0, last_received = 0;     // payload bytes of the last exchange_bands / allreduce (lentil_hip_exchange_stats)
  // Fixed-capacity form of the tiled exchange (exchange_bands_fixed): entries the last message of each directed pair
  // carried, as both of its ends know it (-1: none yet) -- the capacity of the next one follows from it on both sides
  std::vector<int64_t> hist_out, hist_in;
  uint32_t *h_hdr = nullptr;                     // pinned: [world] headers to send, [world] sent (read back), [world] received
  uint64_t n_fixed = 0, n_fixed_overflow = 0;    // exchanges in that form / directed pairs whose entries did not fit
  // An exchange in that form that returned an error on this rank.  Its peers' histories have moved on (or will, once their
  // receives time out or complete) while this rank's have not, so the two ends of a pair would size their next message
  // differently: every later exchange on this communicator is refused at once instead of posting sends and receives of
  // unequal length (round-4 ADVICE).  Destroy and re-create the communicators on all ranks.
  bool poisoned = false;
};

// One message of the fixed-capacity form, ONE send per directed pair: 4 header words {entries found, capacity, first row,
// end row of the region the sender compacted}, `cap` pixel indices, `cap` records of 4 n_aovs + 1 floats, `cap` winner keys
// per key plane the frame has.
constexpr uint32_t kHdrWords = 4;
static uint32_t pair_capacity(int64_t hist, uint64_t band_pix) {
  // (LENTIL_EXCHANGE_CAP_FIRST: the capacity of a pair's first message -- tests make first messages overflow with it)
  static const uint64_t first_ = getenv("LENTIL_EXCHANGE_CAP_FIRST") ? (uint64_t)atoll(getenv("LENTIL_EXCHANGE_CAP_FIRST")) : 0ull;
  uint64_t c = hist < 0 ? (first_ ? first_ : band_pix / 16) : 2 * (uint64_t)hist + 256;      // twice what the pair carried last time
  if (c < 1024 && !(hist < 0 && first_)) c = 1024;
  if (c > band_pix) c = band_pix;                                          // (never more entries than the band has pixels)
  return (uint32_t)((c + 1ull) & ~1ull);                                   // (even: the keys behind the records stay 8-byte aligned)
}

#define RCCL_TRY(ctx, call)                                                                           \
  do {                                                                                                \
    const int r_ = (call);                                                                            \
    if (r_ != 0) return fail(ctx, LENTIL_ERR_HIP, std::string(#call) + ": " + g_rccl.GetErrorString(r_)); \
  } while (0)

static int comm_scratch(lentil_hip_ctx *ctx, LentilComm *cm, size_t slot, size_t bytes, void **out) {
  if (cm->scratch.size() <= slot) { cm->scratch.resize(slot + 1, nullptr); cm->scratch_bytes.resize(slot + 1, 0); }
  if (cm->scratch_bytes[slot] < bytes) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // nobody is still using the old buffer
    (void)hipFree(cm->scratch[slot]);
    cm->scratch[slot] = nullptr;
    const size_t want = bytes + bytes / 4 + 4096;
    HIP_TRY(ctx, hipMalloc(&cm->scratch[slot], want));
    cm->scratch_bytes[slot] = want;
  }
  *out = cm->scratch[slot];
  return LENTIL_OK;
}

LENTIL_API int lentil_hip_comm_unique_id(uint8_t id[128]) {
  if (!id) return fail(nullptr, LENTIL_ERR_INVALID, "id is null");
  if (const char *e = load_rccl()) return fail(nullptr, LENTIL_ERR_UNSUPPORTED, e);
  const int r = g_rccl.GetUniqueId(id);
  if (r != 0) return fail(nullptr, LENTIL_ERR_HIP, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
  return LENTIL_OK;
}

LENTIL_API int lentil_hip_comm_destroy(lentil_hip_ctx *ctx) {
  CHECK_CTX(ctx);
  LentilComm *cm = ctx->comm;
  if (!cm) return LENTIL_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (cm->comm) (void)g_rccl.CommDestroy(cm->comm);
  (void)hipFree(cm->d_meta_mine); (void)hipFree(cm->d_meta_all);
  if (cm->h_meta_all) (void)hipHostFree(cm->h_meta_all);
  if (cm->h_hdr) (void)hipHostFree(cm->h_hdr);
  for (void *p : cm->scratch) (void)hipFree(p);
  delete cm;
  ctx->comm = nullptr;
  return LENTIL_OK;
}

LENTIL_API int lentil_hip_comm_init(lentil_hip_ctx *ctx, const uint8_t id[128], int rank, int world) {
  CHECK_CTX(ctx);
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(ctx, LENTIL_ERR_INVALID, "bad communicator arguments");
  if (const char *e = load_rccl()) return fail(ctx, LENTIL_ERR_UNSUPPORTED, e);
  int rc = lentil_hip_comm_destroy(ctx);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  LentilComm *cm = new (std::nothrow) LentilComm();
  if (!cm) return fail(ctx, LENTIL_ERR_NOMEM, "out of host memory");
  cm->rank = rank; cm->world = world;
  LentilNcclId uid;
  memcpy(uid.b, id, 128);
  // (the context only gets a communicator that is complete: a half-built one would be handed to RCCL by the next
  // exchange, and would make the cryptomatte pass refuse the context for being "multi-GPU")
  auto undo = [&]() {
    if (cm->comm) (void)g_rccl.CommDestroy(cm->comm);
    (void)hipFree(cm->d_meta_mine); (void)hipFree(cm->d_meta_all);
    if (cm->h_meta_all) (void)hipHostFree(cm->h_meta_all);
    if (cm->h_hdr) (void)hipHostFree(cm->h_hdr);
    delete cm;
  };
  {
    const int r = g_rccl.CommInitRank(&cm->comm, world, uid, rank);
    if (r != 0) { cm->comm = nullptr; undo(); return fail(ctx, LENTIL_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); }
  }
  const size_t m = (size_t)(2 + world);
  hipError_t e = hipMalloc(&cm->d_meta_mine, m * sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc(&cm->d_meta_all, m * (size_t)world * sizeof(int64_t));
  if (e == hipSuccess) e = hipHostMalloc((void **)&cm->h_meta_all, m * (size_t)world * sizeof(int64_t), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void **)&cm->h_hdr, (size_t)3 * world * kHdrWords * sizeof(uint32_t), hipHostMallocDefault);
  if (e != hipSuccess) { undo(); return fail(ctx, LENTIL_ERR_HIP, std::string("communicator buffers: ") + hipGetErrorString(e)); }
  cm->hist_out.assign((size_t)world, -1);
  cm->hist_in.assign((size_t)world, -1);
  ctx->comm = cm;
  return LENTIL_OK;
}

// payload bytes this rank sent / received in its last lentil_hip_exchange_bands (entries or packed rows, keys included) or
// lentil_hip_allreduce (ring traffic 2 (G - 1) / G of the reduced buffers, both ways)
LENTIL_API int lentil_hip_exchange_stats(lentil_hip_ctx *ctx, uint64_t *bytes_sent, uint64_t *bytes_received) {
  CHECK_CTX(ctx);
  if (!ctx->comm) return fail(ctx, LENTIL_ERR_INVALID, "no communicator (lentil_hip_comm_init)");
  if (bytes_sent) *bytes_sent = ctx->comm->last_sent;
  if (bytes_received) *bytes_received = ctx->comm->last_received;
  return LENTIL_OK;
}

LENTIL_API int lentil_hip_exchange_counts(lentil_hip_ctx *ctx, uint64_t *fixed_form, uint64_t *pairs_overflowed) {
  CHECK_CTX(ctx);
  if (!ctx->comm) return fail(ctx, LENTIL_ERR_INVALID, "no communicator (lentil_hip_comm_init)");
  if (fixed_form) *fixed_form = ctx->comm->n_fixed;
  if (pairs_overflowed) *pairs_overflowed = ctx->comm->n_fixed_overflow;
  return LENTIL_OK;
}

// ---- closest-filtered AOVs with candidates at depth 0 / NaN across GPUs (lentil_closest_replay.h) ------------------------
// The outcome at such a pixel depends on the order of ALL its candidates, on every rank: a min-reduce or a min-merge of the
// keys gets it wrong.  Scratch slots of this step lie behind the 12 per peer of the exchanges.
static size_t deg_slot(const LentilComm *cm, size_t k) { return (size_t)cm->world * 12 + k; }

// One word per rank -- did its pass meet such a candidate -- all-gathered at the start of the exchange, before anything from
// another rank is merged.  When some rank did, every rank needs its pass's draw log: one that kept none (or an incomplete one)
// runs the pass again with one, as on one GPU (its frame holds nothing but that pass yet).  *any: the replay step runs.
static int degenerate_agree(lentil_hip_ctx *ctx, LentilComm *cm, bool *any) {
  *any = false;
  const int64_t word = ctx->degenerate_seen ? 1 : 0;
  HIP_TRY(ctx, hipMemcpyAsync(cm->d_meta_mine, &word, sizeof word, hipMemcpyHostToDevice, ctx->stream));
  RCCL_TRY(ctx, g_rccl.AllGather(cm->d_meta_mine, cm->d_meta_all, 1, kNcclInt64, cm->comm, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(cm->h_meta_all, cm->d_meta_all, (size_t)cm->world * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int q = 0; q < cm->world; ++q)
    if (cm->h_meta_all[q] & 1) *any = true;
  if (!*any) return LENTIL_OK;
  bool complete = false;
  unsigned long long n_log = 0;
  const int rc = closest_log_complete(ctx, &complete, &n_log);
  if (rc || complete) return rc;
  return closest_rerun_with_log(ctx, nullptr);
}

// Sized point-to-point exchange of byte blocks: out[q] (n_out[q] bytes) goes to rank q; what the others send to this rank lands
// in scratch slot `slot` behind `front` bytes, in rank order (n_in[q] bytes from q).  The sizes travel first: one all-gather of
// world words per rank.
static int deg_alltoall(lentil_hip_ctx *ctx, LentilComm *cm, const std::vector<const uint8_t *> &out, const std::vector<uint64_t> &n_out,
                        size_t slot, uint64_t front, uint8_t **in, std::vector<uint64_t> &n_in) {
  const int world = cm->world, rank = cm->rank;
  std::vector<int64_t> mine((size_t)world, 0);
  for (int q = 0; q < world; ++q) mine[(size_t)q] = q == rank ? 0 : (int64_t)n_out[(size_t)q];
  HIP_TRY(ctx, hipMemcpyAsync(cm->d_meta_mine, mine.data(), (size_t)world * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  RCCL_TRY(ctx, g_rccl.AllGather(cm->d_meta_mine, cm->d_meta_all, (size_t)world, kNcclInt64, cm->comm, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(cm->h_meta_all, cm->d_meta_all, (size_t)world * world * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  n_in.assign((size_t)world, 0);
  uint64_t total = front;
  for (int q = 0; q < world; ++q) {
    const int64_t n = q == rank ? 0 : cm->h_meta_all[(size_t)q * world + rank];
    if (n < 0) return fail(ctx, LENTIL_ERR_HIP, "closest-AOV replay across GPUs: a peer announced a negative size");
    n_in[(size_t)q] = (uint64_t)n;
    total += (uint64_t)n;
  }
  void *p;
  int rc;
  if ((rc = comm_scratch(ctx, cm, slot, (size_t)total, &p))) return rc;
  *in = (uint8_t *)p;
  RCCL_TRY(ctx, g_rccl.GroupStart());
  int g_err = 0;
  uint64_t off = front;
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    if (n_out[(size_t)q] && !g_err) g_err = g_rccl.Send(out[(size_t)q], (size_t)n_out[(size_t)q], kNcclUint8, q, cm->comm, ctx->stream);
    if (n_in[(size_t)q] && !g_err) g_err = g_rccl.Recv(*in + off, (size_t)n_in[(size_t)q], kNcclUint8, q, cm->comm, ctx->stream);
    off += n_in[(size_t)q];
  }
  const int r_end = g_rccl.GroupEnd();
  if (g_err) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclSend / ncclRecv: ") + g_rccl.GetErrorString(g_err));
  if (r_end) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(r_end));
  return LENTIL_OK;
}

// The replay over every rank's candidates, after a degenerate_agree that found some rank with a degenerate candidate.
// Interleaved (bands == null): every rank sends its nodes to every other one and writes the same winner keys into the whole
// frame -- call it after the min-reduces, before the gather, whose sum all-reduce then carries the values.  Tiled (`bands`:
// rows [lo, hi) of every rank, 2 world words): a node goes to the owner of its pixel's band with the values its visit gives
// the closest slots, and the owner writes keys and values in its rows [b_lo, b_hi) -- after the merges, before the resolve.
static int degenerate_exchange(lentil_hip_ctx *ctx, LentilComm *cm, const int32_t *bands, int32_t b_lo, int32_t b_hi) {
  const int world = cm->world, rank = cm->rank;
  const uint64_t np = ctx->F.np;
  int rc;
  untrust_touched(ctx);              // (the closest slots of flagged pixels are written below)
  ctx->resolved_valid = false;
  bool complete = false;
  unsigned long long n_log = 0;
  if ((rc = closest_log_complete(ctx, &complete, &n_log))) return rc;
  if (!complete) return fail(ctx, LENTIL_ERR_NOMEM, "closest-AOV replay across GPUs: the draw log did not hold the pass's accepted draws");
  const int n_dest = bands ? world : 1;
  const dim3 grid((unsigned)ctx->num_cu * 8), block(256);
  void *p;
  // control words: [0] flagged pixels, [1, 1 + n_dest) nodes per destination, then first node / nodes of every segment,
  // then (tiled) the bands
  const size_t ctl_words = 1 + 3 * (size_t)n_dest + 2 * (size_t)world;
  if ((rc = comm_scratch(ctx, cm, deg_slot(cm, 0), ctl_words * 4, &p))) return rc;
  unsigned int *ctl = (unsigned int *)p;
  int32_t *d_bands = reinterpret_cast<int32_t *>(ctl + 1 + 3 * (size_t)n_dest);
  if ((rc = comm_scratch(ctx, cm, deg_slot(cm, 1), (size_t)np, &p))) return rc;
  uint8_t *flag = (uint8_t *)p;
  HIP_TRY(ctx, hipMemsetAsync(ctl, 0, (1 + (size_t)n_dest) * 4, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(flag, 0, (size_t)np, ctx->stream));
  if (bands) HIP_TRY(ctx, hipMemcpyAsync(d_bands, bands, 2 * (size_t)world * 4, hipMemcpyHostToDevice, ctx->stream));
  ReplayArgs a{};
  a.P = ctx->P; a.lens_length = ctx->have_lens ? ctx->hlens.length : 0.0; a.V = ctx->V; a.F = ctx->F;
  a.log = ctx->d_log; a.n_log = n_log; a.flag = flag;
  // ---- 1. the pixels this rank's degenerate candidates reached, compacted; every rank's list to every rank
  hipLaunchKernelGGL(replay_mark_visits_kernel, grid, block, 0, ctx->stream, a);
  if (n_log) hipLaunchKernelGGL(replay_mark_log_kernel, grid, block, 0, ctx->stream, a);
  if ((rc = comm_scratch(ctx, cm, deg_slot(cm, 2), 4096 * 4, &p))) return rc;
  uint32_t cap = (uint32_t)(cm->scratch_bytes[deg_slot(cm, 2)] / 4 > 0xFFFFFFFFull ? 0xFFFFFFFFull : cm->scratch_bytes[deg_slot(cm, 2)] / 4);
  hipLaunchKernelGGL(xflag_compact_kernel, grid, block, 0, ctx->stream, flag, np, (uint32_t *)p, cap, ctl);
  HIP_TRY(ctx, hipGetLastError());
  unsigned int n_own = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&n_own, ctl, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (n_own > cap) {
    if ((rc = comm_scratch(ctx, cm, deg_slot(cm, 2), (size_t)n_own * 4, &p))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctl, 0, 4, ctx->stream));
    hipLaunchKernelGGL(xflag_compact_kernel, grid, block, 0, ctx->stream, flag, np, (uint32_t *)p, n_own, ctl);
    HIP_TRY(ctx, hipGetLastError());
  }
  const uint8_t *own_list = (const uint8_t *)p;
  std::vector<const uint8_t *> out((size_t)world, own_list);
  std::vector<uint64_t> n_out((size_t)world, (uint64_t)n_own * 4), n_in;
  uint8_t *got = nullptr;
  if ((rc = deg_alltoall(ctx, cm, out, n_out, deg_slot(cm, 3), 0, &got, n_in))) return rc;
  uint64_t n_got = 0;
  for (uint64_t n : n_in) n_got += n / 4;
  if (n_got) hipLaunchKernelGGL(xflag_set_kernel, grid, block, 0, ctx->stream, flag, np, (const uint32_t *)got, n_got);
  // ---- 2. this rank's candidates at every flagged pixel: counted per destination, then filled into their segments
  HIP_TRY(ctx, hipMemsetAsync(ctl, 0, (1 + (size_t)n_dest) * 4, ctx->stream));
  hipLaunchKernelGGL(xflag_compact_kernel, grid, block, 0, ctx->stream, flag, np, nullptr, 0u, ctl);      // (the count: the stats)
  XNodeArgs x{};
  x.a = a;
  x.words = kXNodeWords + (bands ? 4u * ctx->F.n_aovs : 0u);
  x.n_dest = n_dest;
  x.bands = bands ? d_bands : nullptr;
  x.count = ctl + 1;
  x.seg = ctl + 1 + n_dest;
  x.out = nullptr;
  hipLaunchKernelGGL(xnode_pack_kernel, grid, block, 0, ctx->stream, x);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<unsigned int> cnt(1 + (size_t)n_dest);
  HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), ctl, cnt.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->deg_flagged = cnt[0];
  std::vector<unsigned int> seg(2 * (size_t)n_dest);
  uint64_t n_mine = 0;
  for (int d = 0; d < n_dest; ++d) { seg[(size_t)d] = (unsigned int)n_mine; seg[(size_t)(n_dest + d)] = cnt[(size_t)(1 + d)]; n_mine += cnt[(size_t)(1 + d)]; }
  if (n_mine > 0xFFFFFFFFull / 2) return fail(ctx, LENTIL_ERR_NOMEM, "closest-AOV replay across GPUs: too many candidates");
  const uint64_t node_bytes = (uint64_t)x.words * 4;
  if ((rc = comm_scratch(ctx, cm, deg_slot(cm, 4), (size_t)(n_mine * node_bytes), &p))) return rc;
  x.out = (uint32_t *)p;
  HIP_TRY(ctx, hipMemcpyAsync(ctl + 1 + n_dest, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ctl + 1, 0, (size_t)n_dest * 4, ctx->stream));
  if (n_mine) hipLaunchKernelGGL(xnode_pack_kernel, grid, block, 0, ctx->stream, x);
  HIP_TRY(ctx, hipGetLastError());
  // ---- 3. the nodes travel: interleaved all of them to every rank, tiled each to the owner of its pixel
  const uint8_t *mine_nodes = (const uint8_t *)x.out;
  uint64_t n_keep = n_mine;
  for (int q = 0; q < world; ++q) {
    if (bands) { out[(size_t)q] = mine_nodes + (uint64_t)seg[(size_t)q] * node_bytes; n_out[(size_t)q] = (uint64_t)seg[(size_t)(n_dest + q)] * node_bytes; }
    else { out[(size_t)q] = mine_nodes; n_out[(size_t)q] = n_mine * node_bytes; }
  }
  if (bands) n_keep = seg[(size_t)(n_dest + rank)];
  uint8_t *all = nullptr;
  if ((rc = deg_alltoall(ctx, cm, out, n_out, deg_slot(cm, 5), n_keep * node_bytes, &all, n_in))) return rc;
  if (n_keep) HIP_TRY(ctx, hipMemcpyAsync(all, bands ? out[(size_t)rank] : mine_nodes, (size_t)(n_keep * node_bytes), hipMemcpyDeviceToDevice, ctx->stream));
  uint64_t n_all = n_keep, sent = 0, received = 0;
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    sent += n_out[(size_t)q] / node_bytes;
    received += n_in[(size_t)q] / node_bytes;
  }
  n_all += received;
  ctx->deg_nodes_sent = sent;
  ctx->deg_nodes_received = received;
  if (n_all > 0xFFFFFFF0ull) return fail(ctx, LENTIL_ERR_NOMEM, "closest-AOV replay across GPUs: too many candidates");
  // ---- 4. the per-pixel lists over the union, resolved by the one-GPU rule
  if ((rc = comm_scratch(ctx, cm, deg_slot(cm, 6), (size_t)np * 4, &p))) return rc;
  uint32_t *head = (uint32_t *)p;
  if ((rc = comm_scratch(ctx, cm, deg_slot(cm, 7), (size_t)n_all * sizeof(ReplayNode), &p))) return rc;
  ReplayNode *rnodes = (ReplayNode *)p;
  HIP_TRY(ctx, hipMemsetAsync(head, 0xFF, (size_t)np * 4, ctx->stream));
  if (n_all) hipLaunchKernelGGL(xnode_list_kernel, grid, block, 0, ctx->stream, (const uint32_t *)all, x.words, (uint32_t)n_all, np, head, rnodes);
  const uint64_t p_lo = bands ? (uint64_t)b_lo * ctx->P.xres : 0ull, p_hi = bands ? (uint64_t)b_hi * ctx->P.xres : np;
  if (p_hi > p_lo)
    hipLaunchKernelGGL(xnode_resolve_kernel, grid, block, 0, ctx->stream, ctx->F, (const uint8_t *)flag, p_lo, p_hi < np ? p_hi : np,
                       (const uint32_t *)head, (const ReplayNode *)rnodes, (uint32_t)n_all, (const uint32_t *)all, x.words, bands != nullptr);
  HIP_TRY(ctx, hipGetLastError());
  ++ctx->n_degenerate_replays;
  return LENTIL_OK;
}

// ---- thin lens with abb_chromatic > 0 across GPUs (lentil_tl_chroma_mgpu.h) ----------------------------------------------
// Called inside lentil_hip_redistribute on every rank -- the pass is the collective step here, not the exchange behind it.
// Every rank's items in frame-wide visit order go to every rank as (visit id, D | kTlcDependent) pairs, then the dependent
// items' signatures; every rank merges the lists and runs the same chain over them (the same anchors everywhere), walks its
// own items from them and ends at the whole frame's last generator state.  Scratch slots behind those of the closest-AOV
// replay.
static size_t tlc_slot(const LentilComm *cm, size_t k) { return deg_slot(cm, 8 + k); }

static int tl_chroma_across_ranks(lentil_hip_ctx *ctx, TlChromaArgs &ta, const std::vector<uint32_t> &gids) {
  LentilComm *cm = ctx->comm;
  const int world = cm->world, rank = cm->rank;
  const uint32_t n = ta.n_items;
  int rc;
  void *p;
  TlChromaPar q{};
  q.jump = ctx->d_xor_jump;
  q.val = ctx->d_tlc_val;
  const dim3 grid(tl_chroma_item_blocks(ctx, n)), block(256);
  if (n) hipLaunchKernelGGL(tl_chroma_count_kernel, grid, block, 0, ctx->stream, ta, q);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<uint64_t> val(n);
  if (n) HIP_TRY(ctx, hipMemcpyAsync(val.data(), ctx->d_tlc_val, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  auto sig_words = [](uint64_t v) -> uint64_t { return ((v & 0xFFFFFFFFull) + 7) / 8; };
  // ---- 1. this rank's list to every rank (own first, then the others' in rank order)
  const uint64_t list_bytes = (uint64_t)n * 16;
  std::vector<uint64_t> mine(2 * (size_t)n);
  std::vector<uint64_t> sig_off(n, kTlcNoSig);
  uint64_t my_words = 0;
  for (uint32_t i = 0; i < n; ++i) {
    mine[2 * (size_t)i] = gids[i];
    mine[2 * (size_t)i + 1] = val[i];
    if (val[i] & kTlcDependent) { sig_off[i] = my_words; my_words += sig_words(val[i]); }
  }
  if ((rc = comm_scratch(ctx, cm, tlc_slot(cm, 0), (size_t)list_bytes + 16, &p))) return rc;
  const uint8_t *d_mine = (const uint8_t *)p;
  if (n) HIP_TRY(ctx, hipMemcpyAsync(p, mine.data(), (size_t)list_bytes, hipMemcpyHostToDevice, ctx->stream));
  std::vector<const uint8_t *> out((size_t)world, d_mine);
  std::vector<uint64_t> n_out((size_t)world, list_bytes), n_in;
  uint8_t *got = nullptr;
  if ((rc = deg_alltoall(ctx, cm, out, n_out, tlc_slot(cm, 1), list_bytes, &got, n_in))) return rc;
  if (n) HIP_TRY(ctx, hipMemcpyAsync(got, d_mine, (size_t)list_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  uint64_t total_bytes = list_bytes, received = 0;
  for (int r = 0; r < world; ++r) { if (n_in[(size_t)r] % 16) return fail(ctx, LENTIL_ERR_HIP, "thin-lens abb_chromatic > 0 across GPUs: a torn list"); total_bytes += n_in[(size_t)r]; received += n_in[(size_t)r]; }
  std::vector<uint64_t> all_lists(total_bytes / 8);
  if (total_bytes) HIP_TRY(ctx, hipMemcpyAsync(all_lists.data(), got, (size_t)total_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // ---- 2. the merged list: every entry's rank, index there, and (dependent) the word of its signature in the gathered block,
  // which holds this rank's signatures first, then the others' in rank order
  struct Entry { uint32_t gid; int rank; uint32_t local; uint64_t val, sig; };
  std::vector<Entry> all;
  all.reserve(total_bytes / 16);
  uint64_t pos = 0, sig_base = 0, n_dep = 0;
  for (int k = 0; k < world; ++k) {
    const int r = k == 0 ? rank : (k <= rank ? k - 1 : k);      // (rank order of the blocks behind this rank's own)
    const uint64_t cnt = (r == rank ? list_bytes : n_in[(size_t)r]) / 16;
    for (uint64_t i = 0; i < cnt; ++i, ++pos) {
      const uint64_t v = all_lists[2 * pos + 1];
      Entry e{(uint32_t)all_lists[2 * pos], r, (uint32_t)i, v, kTlcNoSig};
      if (v & kTlcDependent) { e.sig = sig_base; sig_base += sig_words(v); ++n_dep; }
      all.push_back(e);
    }
  }
  std::stable_sort(all.begin(), all.end(), [](const Entry &a, const Entry &b) { return a.gid < b.gid; });
  // The order is the visit ids' own: two items with one id have none (and this rank's block comes first in its own merge, so
  // the ranks would break the tie differently).  Every rank holds the same merged list and refuses it alike -- before any
  // other collective of the pass.
  for (size_t i = 1; i < all.size(); ++i)
    if (all[i].gid == all[i - 1].gid)
      return fail(ctx, LENTIL_ERR_INVALID, "thin-lens abb_chromatic > 0 across GPUs: items of two ranks carry the same frame-wide visit id "
                                           "(a ragged stream numbers its visits from visit_id_base: give every rank its own range, "
                                           "lentil_hip_set_closest_exchange)");
  if (n_dep > 0xFFFFFFF0ull) return fail(ctx, LENTIL_ERR_NOMEM, "thin-lens abb_chromatic > 0 across GPUs: too many dependent items");
  // ---- 3. the dependent items' signatures to every rank (no step at all when no rank has one: every rank knows that now)
  uint32_t *d_sig_all = nullptr;
  if (n_dep) {
    if ((rc = comm_scratch(ctx, cm, tlc_slot(cm, 2), (size_t)n * 8 + 8, &p))) return rc;
    q.sig_off = (const uint64_t *)p;
    if (n) HIP_TRY(ctx, hipMemcpyAsync(p, sig_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = comm_scratch(ctx, cm, tlc_slot(cm, 3), (size_t)my_words * 4 + 4, &p))) return rc;
    q.sig = (uint32_t *)p;
    if (my_words) hipLaunchKernelGGL(tl_chroma_sig_kernel, grid, block, 0, ctx->stream, ta, q);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<const uint8_t *> sout((size_t)world, (const uint8_t *)q.sig);
    std::vector<uint64_t> sn_out((size_t)world, my_words * 4), sn_in;
    uint8_t *sgot = nullptr;
    if ((rc = deg_alltoall(ctx, cm, sout, sn_out, tlc_slot(cm, 4), my_words * 4, &sgot, sn_in))) return rc;
    if (my_words) HIP_TRY(ctx, hipMemcpyAsync(sgot, q.sig, (size_t)my_words * 4, hipMemcpyDeviceToDevice, ctx->stream));
    uint64_t s_total = my_words * 4;
    for (uint64_t b : sn_in) { s_total += b; received += b; }
    if (s_total != sig_base * 4) return fail(ctx, LENTIL_ERR_HIP, "thin-lens abb_chromatic > 0 across GPUs: signatures and lists disagree");
    d_sig_all = (uint32_t *)sgot;
  }
  // ---- 4. the chain's inputs, and every own item's anchor and offset
  std::vector<uint64_t> skip, dsig;
  std::vector<uint32_t> dslots, base_idx(n);
  std::vector<uint64_t> offset(n);
  skip.reserve(n_dep + 1); dsig.reserve(n_dep); dslots.reserve(n_dep);
  uint32_t cur_anchor = 0;
  uint64_t cur_off = 0;
  for (const Entry &e : all) {
    if (e.rank == rank) { base_idx[e.local] = cur_anchor; offset[e.local] = cur_off; }
    if (e.val & kTlcDependent) {
      skip.push_back(cur_off); dsig.push_back(e.sig); dslots.push_back((uint32_t)(e.val & 0xFFFFFFFFull));
      ++cur_anchor;
      cur_off = 0;
    } else {
      cur_off += e.val;
    }
  }
  skip.push_back(cur_off);
  // one block: anchors [n_dep + 1] uint4, skip [n_dep + 1], signature offsets [n_dep], slots [n_dep], own items' anchors / offsets
  const size_t b_anchor = 0, b_skip = b_anchor + (n_dep + 1) * 16, b_dsig = b_skip + (n_dep + 1) * 8, b_base = b_dsig + n_dep * 8,
               b_offset = b_base + ((size_t)n * 8 + 8), b_slots = b_offset + (size_t)n * 8, b_end = b_slots + n_dep * 4 + 4;
  if ((rc = comm_scratch(ctx, cm, tlc_slot(cm, 5), b_end, &p))) return rc;
  uint8_t *blk = (uint8_t *)p;
  std::vector<uint8_t> h(b_end, 0);
  memcpy(h.data() + b_anchor, ctx->xor_state, 16);
  memcpy(h.data() + b_skip, skip.data(), skip.size() * 8);
  if (n_dep) memcpy(h.data() + b_dsig, dsig.data(), n_dep * 8);
  if (n) { memcpy(h.data() + b_base, base_idx.data(), (size_t)n * 4); memcpy(h.data() + b_offset, offset.data(), (size_t)n * 8); }
  if (n_dep) memcpy(h.data() + b_slots, dslots.data(), n_dep * 4);
  HIP_TRY(ctx, hipMemcpyAsync(blk, h.data(), b_end, hipMemcpyHostToDevice, ctx->stream));
  TlChainArgs c{};
  c.jump = ctx->d_xor_jump;
  c.anchor = (uint4 *)(blk + b_anchor);
  c.n_dep = (uint32_t)n_dep;
  c.skip = (const uint64_t *)(blk + b_skip);
  c.sig_off = (const uint64_t *)(blk + b_dsig);
  c.slots = (const uint32_t *)(blk + b_slots);
  c.sig = d_sig_all;
  c.final_state = ctx->d_xor;
  hipLaunchKernelGGL(tl_chroma_chain_kernel, dim3(1), dim3(64), 0, ctx->stream, c);
  HIP_TRY(ctx, hipGetLastError());
  // ---- 5. this rank's items, in parallel, from their anchors; the frame's last state for the next pass
  if (n) {
    q.base = c.anchor;
    q.base_idx = (const uint32_t *)(blk + b_base);
    q.offset = (const uint64_t *)(blk + b_offset);
    q.entry_out = ctx->d_tlc_entry;
    hipLaunchKernelGGL(tl_chroma_walk_par_kernel, grid, block, 0, ctx->stream, ta, q);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->xor_state, ctx->d_xor, sizeof ctx->xor_state, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // (h and the vectors above are the copies' sources)
  ctx->tlc_items = all.size();
  ctx->tlc_dependent = n_dep;
  ctx->tlc_gathered = received;
  return LENTIL_OK;
}

// interleaved partition: every rank ends up with the whole frame's accumulators (distributed.frame_step)
LENTIL_API int lentil_hip_allreduce(lentil_hip_ctx *ctx) {
  CHECK_CTX(ctx);
  ctx->resolved_valid = false;
  LentilComm *cm = ctx->comm;
  if (!cm) return fail(ctx, LENTIL_ERR_INVALID, "no communicator (lentil_hip_comm_init)");
  if (!ctx->have_frame) return fail(ctx, LENTIL_ERR_INVALID, "no frame allocated");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if (ctx->crypto) return fail(ctx, LENTIL_ERR_UNSUPPORTED, "cryptomatte AOVs travel with the tiled exchange only (lentil_hip_exchange_bands)");
  bool degenerate = false;         // some rank's pass met a closest candidate at depth 0 / NaN (a pass run again here has a log)
  if ((ctx->F.zkey || ctx->F.zkey_dbg) && ctx->closest_deferred && (rc = degenerate_agree(ctx, cm, &degenerate))) return rc;
  if ((rc = fold_direct(ctx, 0, ctx->F.np, true))) return rc;        // what the scan kept apart joins the sum
  untrust_touched(ctx);
  if (ctx->F.zkey || ctx->F.zkey_dbg) {
    if (!ctx->closest_deferred)
      return fail(ctx, LENTIL_ERR_INVALID, "closest-filtered AOVs: lentil_hip_set_closest_exchange(ctx, 1, ...) before the pass");
    if (ctx->F.zkey)
      RCCL_TRY(ctx, g_rccl.AllReduce(ctx->F.zkey, ctx->F.zkey, ctx->F.np, kNcclUint64, kNcclMin, cm->comm, ctx->stream));
    if (ctx->F.zkey_dbg)       // lentil_debug: a key plane of its own (src/lentil.h:838-845)
      RCCL_TRY(ctx, g_rccl.AllReduce(ctx->F.zkey_dbg, ctx->F.zkey_dbg, ctx->F.np, kNcclUint64, kNcclMin, cm->comm, ctx->stream));
    if (degenerate && (rc = degenerate_exchange(ctx, cm, nullptr, 0, 0))) return rc;      // the same winner keys on every rank
    if ((rc = lentil_hip_closest_gather(ctx))) return rc;
  }
  RCCL_TRY(ctx, g_rccl.AllReduce(ctx->F.acc, ctx->F.acc, ctx->F.np * ctx->F.stride, kNcclFloat32, kNcclSum, cm->comm, ctx->stream));
  {
    uint64_t bytes = ctx->F.np * ctx->F.stride * 4ull;
    if (ctx->F.zkey) bytes += ctx->F.np * 8ull;
    if (ctx->F.zkey_dbg) bytes += ctx->F.np * 8ull;
    cm->last_sent = cm->last_received = cm->world > 1 ? bytes * 2ull * (uint64_t)(cm->world - 1) / (uint64_t)cm->world : 0ull;
  }
  return LENTIL_OK;
}

// The tiled exchange without a host round trip in its middle.  The form below this one compacts
// per destination, reads every count back (a stream sync each), all-gathers the counts (another sync) and only then knows
// the sizes of its sends and receives.  Here the size of every message is known to both of its ends BEFORE the pass: a
// capacity that follows from what the same directed pair carried in the previous exchange (pair_capacity; both ends saw
// that number -- the sender counted it, the receiver read it in the header), so compaction, sends, receives, merges and
// the band's resolve are enqueued back to back and the merge kernels take the entry count from the header word that
// arrived.  The host looks at the headers once, at the end: they give the next capacities, and a pair whose entries did
// not fit (count > capacity: nothing of it was merged) sends the rows of its region whole, as the sized form does.
static int exchange_bands_fixed(lentil_hip_ctx *ctx, LentilComm *cm, const int32_t *bounds, int32_t visit_rows,
                                int32_t b_lo, int32_t b_hi, int32_t lo, int32_t hi, const int32_t *deg_bands) {
  const int world = cm->world, rank = cm->rank;
  const int32_t yres = (int32_t)ctx->P.yres;
  const uint32_t xres = ctx->P.xres;
  auto band_of = [&](int r, int32_t &l, int32_t &h) {
    if (bounds) { l = bounds[r]; h = bounds[r + 1]; }
    else { l = (int32_t)((int64_t)visit_rows * r / world); h = (int32_t)((int64_t)visit_rows * (r + 1) / world); }
    if (r == world - 1) h = yres;
  };
  const uint32_t used = 4u * ctx->F.n_aovs + 1u;
  const bool keys = ctx->F.zkey != nullptr, dkeys = ctx->F.zkey_dbg != nullptr;
  int rc;
  struct Msg { uint32_t cap = 0; int32_t lo = 0, hi = 0; size_t bytes = 0; uint32_t *idx = nullptr; float *vals = nullptr; unsigned long long *k = nullptr, *kd = nullptr; };
  std::vector<Msg> out((size_t)world), in((size_t)world);
  uint32_t *h_send = cm->h_hdr, *h_sent = cm->h_hdr + (size_t)world * kHdrWords, *h_got = cm->h_hdr + (size_t)2 * world * kHdrWords;
  const uint64_t my_pix = (uint64_t)(b_hi > b_lo ? b_hi - b_lo : 0) * xres;
  auto buffers = [&](Msg &m, int q, size_t slot) -> int {
    m.bytes = ((size_t)kHdrWords + (size_t)m.cap * (1u + used)) * 4 + (size_t)m.cap * 8 * ((keys ? 1u : 0u) + (dkeys ? 1u : 0u));
    void *p;
    const int r = comm_scratch(ctx, cm, (size_t)q * 12 + slot, m.bytes, &p);
    if (r) return r;
    m.idx = (uint32_t *)p;                                   // (the header first: idx[0 .. kHdrWords), entries from idx + kHdrWords)
    m.vals = reinterpret_cast<float *>(m.idx + kHdrWords + m.cap);
    unsigned long long *kp = reinterpret_cast<unsigned long long *>(m.vals + (size_t)m.cap * used);
    if (keys) { m.k = kp; kp += m.cap; }
    if (dkeys) m.kd = kp;
    return LENTIL_OK;
  };
  // ---- what this rank added to every other band: compacted into that pair's message, the count stays on the device
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    int32_t q_lo, q_hi;
    band_of(q, q_lo, q_hi);
    Msg &o = out[(size_t)q];
    o.cap = pair_capacity(cm->hist_out[(size_t)q], (uint64_t)(q_hi > q_lo ? q_hi - q_lo : 0) * xres);
    o.lo = lo > q_lo ? lo : q_lo;
    o.hi = hi < q_hi ? hi : q_hi;
    if (o.hi < o.lo) o.hi = o.lo;
    if ((rc = buffers(o, q, 0))) return rc;
    uint32_t *h = h_send + (size_t)q * kHdrWords;
    h[0] = 0u; h[1] = o.cap; h[2] = (uint32_t)o.lo; h[3] = (uint32_t)o.hi;
    HIP_TRY(ctx, hipMemcpyAsync(o.idx, h, kHdrWords * 4, hipMemcpyHostToDevice, ctx->stream));
    if (o.hi > o.lo && o.cap)
      if ((rc = compact_rows_impl(ctx, (uint32_t)o.lo, (uint32_t)(o.hi - o.lo), o.idx + kHdrWords, o.vals, o.k, o.kd, o.cap, nullptr,
                                  reinterpret_cast<unsigned int *>(o.idx)))) return rc;
    Msg &i = in[(size_t)q];
    i.cap = pair_capacity(cm->hist_in[(size_t)q], my_pix);
    if ((rc = buffers(i, q, 4))) return rc;
  }
  // ---- the exchange: every message has its size on both sides already
  RCCL_TRY(ctx, g_rccl.GroupStart());
  int g_err = 0;
  uint64_t sent = 0, received = 0;
  auto snd = [&](const void *p, size_t n, int type, size_t elem, int q) {
    if (!n) return;
    if (!g_err) g_err = g_rccl.Send(p, n, type, q, cm->comm, ctx->stream);
    sent += (uint64_t)n * elem;
  };
  auto rcv = [&](void *p, size_t n, int type, size_t elem, int q) {
    if (!n) return;
    if (!g_err) g_err = g_rccl.Recv(p, n, type, q, cm->comm, ctx->stream);
    received += (uint64_t)n * elem;
  };
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    snd(out[(size_t)q].idx, out[(size_t)q].bytes, kNcclUint8, 1, q);
    rcv(in[(size_t)q].idx, in[(size_t)q].bytes, kNcclUint8, 1, q);
  }
  {
    const int r_end = g_rccl.GroupEnd();
    if (g_err) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclSend / ncclRecv: ") + g_rccl.GetErrorString(g_err));
    if (r_end) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(r_end));
  }
  // ---- cryptomatte maps: what this rank's draws added outside its band goes to the owners (lentil_crypto.h)
  if (ctx->crypto) {
    std::vector<int32_t> bands((size_t)(2 * world), 0);
    for (int q = 0; q < world; ++q) band_of(q, bands[(size_t)(2 * q)], bands[(size_t)(2 * q + 1)]);
    if ((rc = crypto_exchange_bands(ctx, bands.data(), lo, hi))) return rc;
  }
  // ---- merge what arrived, senders in rank order; the kernels read the count (the rows touched: anywhere in the band)
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    const Msg &i = in[(size_t)q];
    if (i.cap && b_hi > b_lo)
      if ((rc = merge_sparse_impl(ctx, (uint32_t)b_lo, (uint32_t)(b_hi - b_lo), i.cap, i.idx + kHdrWords, i.vals, i.k, i.kd, i.idx))) return rc;
  }
  // (deg_bands: the closest slots of flagged pixels are replayed once every merge is done, the resolve follows that, below)
  if (!deg_bands && (rc = lentil_hip_resolve_rows(ctx, (uint32_t)b_lo, (uint32_t)(b_hi - b_lo)))) return rc;
  // ---- the headers, once everything is on its way
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    HIP_TRY(ctx, hipMemcpyAsync(h_sent + (size_t)q * kHdrWords, out[(size_t)q].idx, kHdrWords * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h_got + (size_t)q * kHdrWords, in[(size_t)q].idx, kHdrWords * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ++cm->n_fixed;
  struct Redo { int q; bool send; int32_t lo, hi; float *packed = nullptr; unsigned long long *key_rows = nullptr, *dkey_rows = nullptr; };
  std::vector<Redo> redo;
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    const uint32_t *hs = h_sent + (size_t)q * kHdrWords, *hg = h_got + (size_t)q * kHdrWords;
    if (hg[1] != in[(size_t)q].cap)
      return fail(ctx, LENTIL_ERR_HIP, "tiled exchange: the ranks disagree about a message's capacity (an exchange failed on one of them: "
                                       "destroy and re-create the communicators)");
    cm->hist_out[(size_t)q] = hs[0];
    cm->hist_in[(size_t)q] = hg[0];
    if (hs[0] > out[(size_t)q].cap) redo.push_back({q, true, out[(size_t)q].lo, out[(size_t)q].hi});
    if (hg[0] > in[(size_t)q].cap) redo.push_back({q, false, (int32_t)hg[2], (int32_t)hg[3]});
  }
  if (!redo.empty()) {
    // entries that did not fit their message: those regions travel as whole rows (both ends of the pair know it)
    cm->n_fixed_overflow += redo.size();
    for (Redo &r : redo) {
      if (r.lo < 0 || r.hi > yres || r.hi <= r.lo) return fail(ctx, LENTIL_ERR_HIP, "tiled exchange: bad region in a message header");
      const uint64_t n_pix = (uint64_t)(r.hi - r.lo) * xres;
      void *p;
      if ((rc = comm_scratch(ctx, cm, (size_t)r.q * 12 + (r.send ? 3 : 5), (size_t)n_pix * used * 4, &p))) return rc;
      r.packed = (float *)p;
      if (r.send) {
        if ((rc = lentil_hip_pack_rows(ctx, (uint32_t)r.lo, (uint32_t)(r.hi - r.lo), r.packed))) return rc;
      } else {
        if (keys) { if ((rc = comm_scratch(ctx, cm, (size_t)r.q * 12 + 6, (size_t)n_pix * 8, &p))) return rc; r.key_rows = (unsigned long long *)p; }
        if (dkeys) { if ((rc = comm_scratch(ctx, cm, (size_t)r.q * 12 + 9, (size_t)n_pix * 8, &p))) return rc; r.dkey_rows = (unsigned long long *)p; }
      }
    }
    RCCL_TRY(ctx, g_rccl.GroupStart());
    for (const Redo &r : redo) {
      const uint64_t n_pix = (uint64_t)(r.hi - r.lo) * xres;
      if (r.send) {
        snd(r.packed, (size_t)n_pix * used, kNcclFloat32, 4, r.q);
        if (keys) snd(ctx->F.zkey + (uint64_t)r.lo * xres, (size_t)n_pix, kNcclUint64, 8, r.q);
        if (dkeys) snd(ctx->F.zkey_dbg + (uint64_t)r.lo * xres, (size_t)n_pix, kNcclUint64, 8, r.q);
      } else {
        rcv(r.packed, (size_t)n_pix * used, kNcclFloat32, 4, r.q);
        if (keys) rcv(r.key_rows, (size_t)n_pix, kNcclUint64, 8, r.q);
        if (dkeys) rcv(r.dkey_rows, (size_t)n_pix, kNcclUint64, 8, r.q);
      }
    }
    {
      const int r_end = g_rccl.GroupEnd();
      if (g_err) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclSend / ncclRecv: ") + g_rccl.GetErrorString(g_err));
      if (r_end) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(r_end));
    }
    bool merged = false;
    for (const Redo &r : redo)
      if (!r.send) {
        if ((rc = merge_rows_impl(ctx, (uint32_t)r.lo, (uint32_t)(r.hi - r.lo), r.packed, r.key_rows, r.dkey_rows, true))) return rc;
        merged = true;
      }
    if (merged && !deg_bands && (rc = lentil_hip_resolve_rows(ctx, (uint32_t)b_lo, (uint32_t)(b_hi - b_lo)))) return rc;
  }
  cm->last_sent = sent; cm->last_received = received;
  if (deg_bands) {
    if ((rc = degenerate_exchange(ctx, cm, deg_bands, b_lo, b_hi))) return rc;
    if ((rc = lentil_hip_resolve_rows(ctx, (uint32_t)b_lo, (uint32_t)(b_hi - b_lo)))) return rc;
  }
  return LENTIL_OK;
}

// row bands (distributed.frame_step_bands): call after lentil_hip_redistribute; ends with the band resolved
LENTIL_API int lentil_hip_exchange_bands(lentil_hip_ctx *ctx, const int32_t *bounds, int32_t visit_rows, int32_t sparse,
                                         int32_t *band_lo, int32_t *band_hi) {
  CHECK_CTX(ctx);
  ctx->resolved_valid = false;
  LentilComm *cm = ctx->comm;
  if (!cm) return fail(ctx, LENTIL_ERR_INVALID, "no communicator (lentil_hip_comm_init)");
  if (!ctx->have_frame || visit_rows <= 0) return fail(ctx, LENTIL_ERR_INVALID, "bad exchange_bands arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int world = cm->world, rank = cm->rank;
  const int32_t yres = (int32_t)ctx->P.yres;
  const uint32_t xres = ctx->P.xres;
  auto band_of = [&](int r, int32_t &lo, int32_t &hi) {
    if (bounds) { lo = bounds[r]; hi = bounds[r + 1]; }
    else { lo = (int32_t)((int64_t)visit_rows * r / world); hi = (int32_t)((int64_t)visit_rows * (r + 1) / world); }
    if (r == world - 1) hi = yres;      // the last band also owns the rows beyond the visits (yres = H + 1)
  };
  int32_t b_lo, b_hi;
  band_of(rank, b_lo, b_hi);
  if (band_lo) *band_lo = b_lo;
  if (band_hi) *band_hi = b_hi;
  int rc;
  int32_t lo = 0, hi = 0;
  if ((rc = lentil_hip_touched_rows(ctx, &lo, &hi))) { if (sparse) cm->poisoned = true; return rc; }      // (the peers go on without this rank's message)
  const uint32_t used = 4u * ctx->F.n_aovs + 1u;
  const bool keys = ctx->F.zkey != nullptr, dkeys = ctx->F.zkey_dbg != nullptr;
  if ((keys || dkeys) && ctx->closest_deferred)
    return fail(ctx, LENTIL_ERR_INVALID, "tiled exchange: the pass must gather its own winners (set_closest_exchange(ctx, 0, ...))");
  // closest candidates at depth 0 / NaN on some rank: agreed on before anything is compacted (a pass run again here changes
  // the frame), replayed after the merges
  std::vector<int32_t> deg_bands;
  if (keys || dkeys) {
    bool degenerate = false;
    const uint64_t reruns = ctx->deg_passes_rerun;
    rc = degenerate_agree(ctx, cm, &degenerate);
    if (!rc && ctx->deg_passes_rerun != reruns) rc = lentil_hip_touched_rows(ctx, &lo, &hi);
    if (rc) { if (sparse) cm->poisoned = true; return rc; }
    if (degenerate) {
      deg_bands.resize((size_t)(2 * world));
      for (int q = 0; q < world; ++q) band_of(q, deg_bands[(size_t)(2 * q)], deg_bands[(size_t)(2 * q + 1)]);
    }
  }

  // (LENTIL_EXCHANGE_FIXED=0: the sized form below, whose sends carry exactly the entries found -- and whose host waits for
  // every count; sparse == 0, whole rows always, is that form too)
  static const bool fixed_form = !(getenv("LENTIL_EXCHANGE_FIXED") && getenv("LENTIL_EXCHANGE_FIXED")[0] == '0');
  if (sparse && fixed_form) {
    if (cm->poisoned)
      return fail(ctx, LENTIL_ERR_INVALID, "tiled exchange: an earlier exchange on this communicator failed on this rank; its message "
                                           "sizes no longer agree with its peers' (lentil_hip_comm_destroy / _comm_init on every rank)");
    rc = exchange_bands_fixed(ctx, cm, bounds, visit_rows, b_lo, b_hi, lo, hi, deg_bands.empty() ? nullptr : deg_bands.data());
    if (rc) cm->poisoned = true;
    return rc;
  }

  // ---- what this rank added to every other band, and the form it will travel in
  struct Out { int form = 0; int32_t s_lo = 0, s_hi = 0; uint32_t *idx = nullptr; float *vals = nullptr; unsigned long long *k = nullptr, *kd = nullptr; float *packed = nullptr; };
  std::vector<Out> out((size_t)world);
  std::vector<int64_t> mine((size_t)(2 + world), 0);
  mine[0] = lo; mine[1] = hi;
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    int32_t q_lo, q_hi;
    band_of(q, q_lo, q_hi);
    Out &o = out[(size_t)q];
    o.s_lo = lo > q_lo ? lo : q_lo;
    o.s_hi = hi < q_hi ? hi : q_hi;
    if (o.s_hi <= o.s_lo) continue;
    o.form = -1;
    const uint64_t n_pix = (uint64_t)(o.s_hi - o.s_lo) * xres;
    if (sparse) {
      const uint32_t cap = (uint32_t)(n_pix / 4 > 1024 ? n_pix / 4 : 1024);
      void *p;
      if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 0, (size_t)cap * 4, &p))) return rc;
      o.idx = (uint32_t *)p;
      if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 1, (size_t)cap * used * 4, &p))) return rc;
      o.vals = (float *)p;
      if (keys) { if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 2, (size_t)cap * 8, &p))) return rc; o.k = (unsigned long long *)p; }
      if (dkeys) { if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 8, (size_t)cap * 8, &p))) return rc; o.kd = (unsigned long long *)p; }
      uint32_t n = 0;
      if ((rc = compact_rows_impl(ctx, (uint32_t)o.s_lo, (uint32_t)(o.s_hi - o.s_lo), o.idx, o.vals, o.k, o.kd, cap, &n, nullptr))) return rc;
      if (n <= cap) o.form = (int)n;
    }
    if (o.form < 0) {
      void *p;
      if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 3, (size_t)n_pix * used * 4, &p))) return rc;
      o.packed = (float *)p;
      if ((rc = lentil_hip_pack_rows(ctx, (uint32_t)o.s_lo, (uint32_t)(o.s_hi - o.s_lo), o.packed))) return rc;
    }
    mine[(size_t)(2 + q)] = o.form;
  }
  // ---- one small all-gather: [touched lo, hi, form per destination] of every rank
  const size_t m = (size_t)(2 + world);
  HIP_TRY(ctx, hipMemcpyAsync(cm->d_meta_mine, mine.data(), m * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  RCCL_TRY(ctx, g_rccl.AllGather(cm->d_meta_mine, cm->d_meta_all, m, kNcclInt64, cm->comm, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(cm->h_meta_all, cm->d_meta_all, m * (size_t)world * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // ---- receive buffers from what the others announced
  struct In { int form = 0; int32_t r_lo = 0, r_hi = 0; uint32_t *idx = nullptr; float *vals = nullptr; unsigned long long *k = nullptr, *kd = nullptr; float *packed = nullptr; unsigned long long *key_rows = nullptr, *dkey_rows = nullptr; };
  std::vector<In> in((size_t)world);
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    const int64_t *info = cm->h_meta_all + (size_t)q * m;
    In &i = in[(size_t)q];
    i.r_lo = (int32_t)(info[0] > b_lo ? info[0] : b_lo);
    i.r_hi = (int32_t)(info[1] < b_hi ? info[1] : b_hi);
    i.form = (int)info[2 + rank];
    if (i.r_hi <= i.r_lo || i.form == 0) { i.form = 0; continue; }
    void *p;
    if (i.form > 0) {
      if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 4, (size_t)i.form * 4, &p))) return rc;
      i.idx = (uint32_t *)p;
      if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 5, (size_t)i.form * used * 4, &p))) return rc;
      i.vals = (float *)p;
      if (keys) { if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 6, (size_t)i.form * 8, &p))) return rc; i.k = (unsigned long long *)p; }
      if (dkeys) { if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 9, (size_t)i.form * 8, &p))) return rc; i.kd = (unsigned long long *)p; }
    } else {
      const uint64_t n_pix = (uint64_t)(i.r_hi - i.r_lo) * xres;
      if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 5, (size_t)n_pix * used * 4, &p))) return rc;
      i.packed = (float *)p;
      if (keys) { if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 6, (size_t)n_pix * 8, &p))) return rc; i.key_rows = (unsigned long long *)p; }
      if (dkeys) { if ((rc = comm_scratch(ctx, cm, (size_t)q * 12 + 9, (size_t)n_pix * 8, &p))) return rc; i.dkey_rows = (unsigned long long *)p; }
    }
  }
  // ---- the exchange itself: every send has its receive on the other side, in the same order per pair
  // (an error inside the group is remembered and returned after GroupEnd: an early return would leave the group open)
  RCCL_TRY(ctx, g_rccl.GroupStart());
  int g_err = 0;
  uint64_t sent = 0, received = 0;
  auto snd = [&](const void *p, size_t n, int type, size_t elem, int q) {
    if (!g_err) g_err = g_rccl.Send(p, n, type, q, cm->comm, ctx->stream);
    sent += (uint64_t)n * elem;
  };
  auto rcv = [&](void *p, size_t n, int type, size_t elem, int q) {
    if (!g_err) g_err = g_rccl.Recv(p, n, type, q, cm->comm, ctx->stream);
    received += (uint64_t)n * elem;
  };
  for (int q = 0; q < world; ++q) {
    if (q == rank) continue;
    const Out &o = out[(size_t)q];
    if (o.form > 0) {
      snd(o.idx, (size_t)o.form * 4, kNcclUint8, 1, q);
      snd(o.vals, (size_t)o.form * used, kNcclFloat32, 4, q);
      if (keys) snd(o.k, (size_t)o.form, kNcclUint64, 8, q);
      if (dkeys) snd(o.kd, (size_t)o.form, kNcclUint64, 8, q);
    } else if (o.form < 0) {
      const uint64_t n_pix = (uint64_t)(o.s_hi - o.s_lo) * xres;
      snd(o.packed, (size_t)n_pix * used, kNcclFloat32, 4, q);
      if (keys) snd(ctx->F.zkey + (uint64_t)o.s_lo * xres, (size_t)n_pix, kNcclUint64, 8, q);
      if (dkeys) snd(ctx->F.zkey_dbg + (uint64_t)o.s_lo * xres, (size_t)n_pix, kNcclUint64, 8, q);
    }
    const In &i = in[(size_t)q];
    if (i.form > 0) {
      rcv(i.idx, (size_t)i.form * 4, kNcclUint8, 1, q);
      rcv(i.vals, (size_t)i.form * used, kNcclFloat32, 4, q);
      if (keys) rcv(i.k, (size_t)i.form, kNcclUint64, 8, q);
      if (dkeys) rcv(i.kd, (size_t)i.form, kNcclUint64, 8, q);
    } else if (i.form < 0) {
      const uint64_t n_pix = (uint64_t)(i.r_hi - i.r_lo) * xres;
      rcv(i.packed, (size_t)n_pix * used, kNcclFloat32, 4, q);
      if (keys) rcv(i.key_rows, (size_t)n_pix, kNcclUint64, 8, q);
      if (dkeys) rcv(i.dkey_rows, (size_t)n_pix, kNcclUint64, 8, q);
    }
  }
  {
    const int r_end = g_rccl.GroupEnd();
    if (g_err) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclSend / ncclRecv: ") + g_rccl.GetErrorString(g_err));
    if (r_end) return fail(ctx, LENTIL_ERR_HIP, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(r_end));
  }
  cm->last_sent = sent; cm->last_received = received;
  // ---- cryptomatte maps: what this rank's draws added outside its band goes to the owners (lentil_crypto.h)
  if (ctx->crypto) {
    std::vector<int32_t> bands((size_t)(2 * world), 0);
    for (int q = 0; q < world; ++q) band_of(q, bands[(size_t)(2 * q)], bands[(size_t)(2 * q + 1)]);
    if ((rc = crypto_exchange_bands(ctx, bands.data(), lo, hi))) return rc;
  }
  // ---- merge what arrived (senders in rank order: the merge of one sender's entries is not atomic against another's)
  for (int q = 0; q < world; ++q) {
    const In &i = in[(size_t)q];
    if (i.form > 0) {
      if ((rc = merge_sparse_impl(ctx, (uint32_t)i.r_lo, (uint32_t)(i.r_hi - i.r_lo), (uint32_t)i.form, i.idx, i.vals, i.k, i.kd))) return rc;
    } else if (i.form < 0) {
      if ((rc = merge_rows_impl(ctx, (uint32_t)i.r_lo, (uint32_t)(i.r_hi - i.r_lo), i.packed, i.key_rows, i.dkey_rows, true))) return rc;
    }
  }
  if (!deg_bands.empty() && (rc = degenerate_exchange(ctx, cm, deg_bands.data(), b_lo, b_hi))) return rc;
  return lentil_hip_resolve_rows(ctx, (uint32_t)b_lo, (uint32_t)(b_hi - b_lo));
}

// the last pass and the exchange behind it: see include/lentil_hip.h
LENTIL_API int lentil_hip_degenerate_stats(lentil_hip_ctx *ctx, uint32_t *degenerate, uint64_t *flagged_pixels, uint64_t *nodes_sent,
                                           uint64_t *nodes_received, uint64_t *passes_rerun) {
  CHECK_CTX(ctx);
  if (degenerate) *degenerate = ctx->degenerate_seen ? 1u : 0u;
  if (flagged_pixels) *flagged_pixels = ctx->deg_flagged;
  if (nodes_sent) *nodes_sent = ctx->deg_nodes_sent;
  if (nodes_received) *nodes_received = ctx->deg_nodes_received;
  if (passes_rerun) *passes_rerun = ctx->deg_passes_rerun;
  return LENTIL_OK;
}
