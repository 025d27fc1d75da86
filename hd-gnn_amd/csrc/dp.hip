// dp.hip -- data-parallel tail of a training step over xGMI (include/hdgnn.h hdg_*_dp;
// SURVEY 8(e)): the mailbox API, hdg_dp_allreduce, hdg_adam_dp and the tail launch of
// hdg_train_step_dp (hdgnn.hip).
//
// Every rank owns a mailbox of uncached device memory that each peer maps through HIP
// IPC.  Block k of the tail kernel owns gradient slots [16k, 16k + 16): it forms its
// local values (the fixed-order sum of the partial rows, or the rank's reduced gradient),
// writes each as an 8-byte (value, tag) word with a system-scope write-through store into
// slot (parity, rank, p) of EVERY peer's mailbox (xGMI, one hop, all peers at once; the
// 8-byte word is single-copy atomic, as in RCCL's LL protocol), polls its own mailbox for
// the peers' words with L2-bypassing loads, and sums the world's values in rank order
// 0..W-1: every rank holds the same bits, so the replicas stay bitwise equal.
//   tag = epoch << 1 | fault: epoch is a per-block launch counter kept in the own mailbox
//   (all ranks issue the same launches); parity = epoch & 1 double-buffers the words, so
//   a rank one launch ahead writes over words every peer has already read (it needed the
//   peers' words of its previous launch, which they sent after reading theirs).  A peer
//   that never arrives ends the wait after wait_ticks: HDG_STATUS_DP_TIMEOUT, NaN loss,
//   no update on that block -- never a hang.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hdgnn.h"
#include "hdgnn_internal.h"
#include "fused_tail.h"

namespace {

using namespace hdg;

namespace dpk {
constexpr int MAXW = HDG_DP_MAX_WORLD;
constexpr int GLENP = HDG_DP_MAX_LEN;               // >= every variant's grad length, x16
constexpr int NBLK = GLENP / RED_P;
constexpr size_t DATA_WORDS = 2ull * MAXW * GLENP;  // u64 (value, tag) words
constexpr size_t OFF_EPOCH = DATA_WORDS * 8;        // u32 [256] per-block launch counters
constexpr size_t OFF_AUX = OFF_EPOCH + 256 * 4;     // f32 [8] loss terms + Adam factor
constexpr size_t OFF_GLOC = OFF_AUX + 8 * 4;        // f32 [GLENP] the rank's own gradient
constexpr size_t BYTES = OFF_GLOC + GLENP * 4;      //   (general path, hdg_train_step_dp)
constexpr unsigned long long WAIT_DEFAULT = 1000000000ull;   // 10 s of s_memrealtime
static_assert(GLENP % RED_P == 0 && NBLK <= 256 && AUX_LEN <= 8, "mailbox layout");
static_assert(GLENP >= 3129 + HDG_TRAILER, "every variant's gradient fits a mailbox row");
enum { SUM = 0, PART = 1, GRAD = 2 };
}  // namespace dpk
// SUM / GRAD blocks only move 16 words per rank: 256 threads (16 ranks x 16 slots), so
// the grid stays small and resident even when several ranks share one device (tests);
// PART runs k_reduce_adam's 1024-thread reduction first
constexpr int DP_NT_LIGHT = dpk::MAXW * RED_P;

struct DpArgs {
  uint32_t* box[dpk::MAXW];
  int rank, world;
  unsigned long long wait;
};

typedef uint32_t xu2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void dstore2(uint32_t* p, const xu2 w) {
  asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" ::"v"(p), "v"(w) : "memory");
}
__device__ __forceinline__ xu2 dload2(const uint32_t* p) {
  xu2 w;
  asm volatile("global_load_dwordx2 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
               : "=v"(w) : "v"(p) : "memory");
  return w;
}
__device__ __forceinline__ uint32_t* dp_slot(uint32_t* box, uint32_t par, int src, int p) {
  return box + 2 * (((size_t)par * dpk::MAXW + src) * dpk::GLENP + p);
}

// A peer's word of epoch e from the own mailbox: polled until its tag arrives or `wait`
// ticks have passed (late; the value is then whatever the slot held).  bad = the peer's
// fault bit.
__device__ __forceinline__ float dp_recv(const uint32_t* in, const uint32_t e,
                                         const unsigned long long wait, bool& late, bool& bad) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  xu2 wd = dload2(in);
  while ((wd.y >> 1) != (e & 0x7FFFFFFFu)) {
    if (__builtin_amdgcn_s_memrealtime() - t0 > wait) { late = true; break; }
    __builtin_amdgcn_s_sleep(1);
    wd = dload2(in);
  }
  bad = (wd.y & 1u) != 0u;
  return __uint_as_float(wd.x);
}

// What the owner of slot p (thread l of its group) does once the world's words are in
// vals: the rank-order sum -> gout (a NaN CE and the status word when a peer was late) and,
// with ADAM, the count / fault slots and the loss stats into stats, TF1 ApplyAdam of a
// parameter slot (adam_tf.h; skipped after a late or faulted peer) and, on the step's first
// slot, the new beta powers.
template <bool ADAM>
__device__ __forceinline__ void dp_own_slot(
    const float (*vals)[RED_P], const int world, const int l, const int p, const int np,
    const bool first, const bool anylate, const bool anybad, bool upd, const float w,
    const float m0, const float v0, float* __restrict__ gout, float* __restrict__ params,
    float* __restrict__ mm, float* __restrict__ vv, float* __restrict__ bpow,
    const float* __restrict__ aux, const float lr, const float inv_pairs,
    float* __restrict__ stats, uint32_t* __restrict__ status) {
  float tot = 0.f;
  for (int q = 0; q < world; ++q) tot += vals[q][l];
  if (ADAM && p == np + HDG_TR_CE && anylate) tot = __builtin_nanf("");
  gout[p] = tot;
  if (anylate && threadIdx.x == 0 && status) xstore1(status, HDG_STATUS_DP_TIMEOUT);
  if constexpr (ADAM) {
    if (stats && p >= np + HDG_TR_COUNT && p <= np + HDG_TR_FAULT)   // count parts, fault
      stats[4 + (p - np - HDG_TR_COUNT)] = tot;
    if (p == np + HDG_TR_CE && stats)
      step_stats_store(stats, tot, inv_pairs, aux[AUX_LMAP], aux[AUX_LPARA]);
    if (anylate || anybad) upd = false;
    if (upd)
      adam_tf_slot(p, np, tot, w, m0, v0, lr * aux[AUX_LRF], aux[AUX_N1], aux[AUX_N2], params, mm,
                   vv);
    if (first && upd) {
      bpow[0] = aux[AUX_B1P];
      bpow[1] = aux[AUX_B2P];
    }
  }
}

// MODE SUM:  gout = world sum of src[0..glen)                       (hdg_dp_allreduce)
// MODE PART: local = fixed-order sum of R partial rows (k_reduce_adam's reduction), then
//            world sum -> gout, TF Adam with aux from k_commit_step   (hdg_train_step_dp)
// MODE GRAD: local = src[0..glen) (a rank's reduced gradient), aux from k_dp_aux (hdg_adam_dp)
template <int MODE>
__global__ __launch_bounds__(1024) void k_dp_tail(const float* __restrict__ src, const int R,
                                                  const int np, const int glen,
                                                  float* __restrict__ gout,
                                                  float* __restrict__ params,
                                                  float* __restrict__ mm, float* __restrict__ vv,
                                                  float* __restrict__ bpow,
                                                  const float* __restrict__ aux, const float lr,
                                                  const float inv_pairs,
                                                  float* __restrict__ stats,
                                                  uint32_t* __restrict__ status,
                                                  const int fault_rows, const DpArgs d) {
  __shared__ RedShared sh;
  __shared__ float gl[RED_P];
  __shared__ float vals[dpk::MAXW][RED_P];
  __shared__ uint32_t s_ep, s_cnt;
  const int t = threadIdx.x, blk = blockIdx.x;
  const int l = t & (RED_P - 1), r = t / RED_P;
  const int p = blk * RED_P + l;
  uint32_t* own = d.box[d.rank];
  uint32_t* ep = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(own) + dpk::OFF_EPOCH);
  if (t == 0) s_ep = ep[blk] + 1u;
  // the update's operands are fetched first so their latency overlaps the reduction
  bool upd = MODE != dpk::SUM && t < RED_P && p < np;
  const float w = upd ? params[p] : 0.f, m0 = upd ? mm[p] : 0.f, v0 = upd ? vv[p] : 0.f;
  float g = 0.f;
  bool bad = false;
  if constexpr (MODE == dpk::PART) {
    for (int q = t; q < fault_rows; q += 1024)             // k_commit_step's fsl
      bad |= src[(size_t)fault_rows * NPART + q] != 0.f;
    uint32_t cnt;
    g = reduce_commits(src, R, p, p < glen, sh, cnt);
    if (t < RED_P && p == CNT_SLOT) s_cnt = cnt;
  } else {
    if (t < RED_P && p < glen) g = src[p];
    if constexpr (MODE == dpk::GRAD) bad = t == 0 && src[np + HDG_TR_FAULT] != 0.f;
  }
  bad = __syncthreads_or(bad);               // also publishes s_ep and s_cnt
  if (t < RED_P) {
    if (MODE == dpk::PART && p >= CNT_SLOT && p <= CNT_SLOT + 2)   // three 16-bit parts
      g = p == CNT_SLOT ? (float)(s_cnt & 0xFFFFu) : (p == CNT_SLOT + 1 ? (float)(s_cnt >> 16) : 0.f);
    gl[l] = g;
  }
  __syncthreads();
  const uint32_t e = s_ep, par = e & 1u;
  const bool mine = r < d.world && p < glen;
  if (mine && r != d.rank)                    // to every peer at once
    dstore2(dp_slot(d.box[r], par, d.rank, p),
            (xu2){__float_as_uint(gl[l]), (e << 1) | (bad ? 1u : 0u)});
  bool late = false, rbad = false;
  if (mine) {
    float v = gl[l];
    if (r != d.rank) v = dp_recv(dp_slot(own, par, r, p), e, d.wait, late, rbad);
    vals[r][l] = v;
  }
  const bool anylate = __syncthreads_or(late);
  const bool anybad = __syncthreads_or(rbad) || bad;
  if (t == 0) ep[blk] = e;                    // this block's launch is consumed
  if (t >= RED_P || p >= glen) return;
  dp_own_slot<MODE != dpk::SUM>(vals, d.world, l, p, np, blk == 0 && t == 0, anylate, anybad,
                                upd, w, m0, v0, gout, params, mm, vv, bpow, aux, lr, inv_pairs,
                                stats, status);
}

// k_dp_tail's SUM / GRAD modes for ranks that share a device (hdg_dp.flags HDG_DP_SHARED):
// G blocks per rank (dp_shared_grid: (W - 1) G <= CUs / 2, G >= HDG_DP_SHARED_BLOCKS),
// block b owning the slot groups b, b + G, ... .  A
// block first sends the words of all its groups (the values are src[p], the epoch of group
// k is ep[k] + 1 as in k_dp_tail), then receives, sums and updates its groups in order:
// the same words, tags, rank-order sums and Adam arithmetic as one k_dp_tail block per
// group (both call dp_recv and dp_own_slot), so the two kernels give the same bits and keep
// the same per-group launch counters.
// Only G blocks per rank spin, so the W-1 ranks waiting for the last one cover at most
// half the CUs and the last rank's step kernel always finds CUs to run on.
template <int MODE>
__global__ __launch_bounds__(DP_NT_LIGHT) void k_dp_tail_shared(
    const float* __restrict__ src, const int np, const int glen, float* __restrict__ gout,
    float* __restrict__ params, float* __restrict__ mm, float* __restrict__ vv,
    float* __restrict__ bpow, const float* __restrict__ aux, const float lr,
    const float inv_pairs, float* __restrict__ stats, uint32_t* __restrict__ status,
    const DpArgs d) {
  static_assert(MODE != dpk::PART, "the shared-device tail exchanges a reduced gradient");
  __shared__ float vals[dpk::MAXW][RED_P];
  const int t = threadIdx.x, l = t & (RED_P - 1), r = t / RED_P;
  const int ngrp = (glen + RED_P - 1) / RED_P;
  uint32_t* own = d.box[d.rank];
  uint32_t* ep = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(own) + dpk::OFF_EPOCH);
  const bool bad = MODE == dpk::GRAD && src[np + HDG_TR_FAULT] != 0.f;
  // 1. every word of this block's groups to every peer
  if (r < d.world && r != d.rank) {
    for (int k = blockIdx.x; k < ngrp; k += gridDim.x) {
      const int p = k * RED_P + l;
      const uint32_t e = ep[k] + 1u;
      if (p < glen)
        dstore2(dp_slot(d.box[r], e & 1u, d.rank, p),
                (xu2){__float_as_uint(src[p]), (e << 1) | (bad ? 1u : 0u)});
    }
  }
  // 2. per group: the peers' words, the rank-order sum, TF Adam
  for (int k = blockIdx.x; k < ngrp; k += gridDim.x) {
    const int p = k * RED_P + l;
    const uint32_t e = ep[k] + 1u, par = e & 1u;
    bool upd = MODE != dpk::SUM && t < RED_P && p < np;
    const float w = upd ? params[p] : 0.f, m0 = upd ? mm[p] : 0.f, v0 = upd ? vv[p] : 0.f;
    bool late = false, rbad = false;
    if (r < d.world && p < glen)
      vals[r][l] =
          r != d.rank ? dp_recv(dp_slot(own, par, r, p), e, d.wait, late, rbad) : src[p];
    const bool anylate = __syncthreads_or(late);
    const bool anybad = __syncthreads_or(rbad) || bad;
    if (t == 0) ep[k] = e;                      // this group's launch is consumed
    if (t < RED_P && p < glen)
      dp_own_slot<MODE == dpk::GRAD>(vals, d.world, l, p, np, k == 0 && t == 0, anylate, anybad,
                                     upd, w, m0, v0, gout, params, mm, vv, bpow, aux, lr,
                                     inv_pairs, stats, status);
    __syncthreads();                            // vals is rewritten by the next group
  }
}

// aux for MODE GRAD (k_commit_step's block 0 writes it on the fused path): loss terms of
// the pre-update parameters (model_2.py:123-130, 326-333) and TF ApplyAdam's lr factor,
// summed by adam_sq_sums, as k_adam_tf does
__global__ __launch_bounds__(1024) void k_dp_aux(const float* __restrict__ params, const int np,
                                                 const float* __restrict__ bpow,
                                                 float* __restrict__ aux) {
  __shared__ float red[16 * 4];
  __shared__ float sh[4];
  const int t = threadIdx.x;
  float w[ADAM_PT];
#pragma unroll
  for (int u = 0; u < ADAM_PT; ++u) w[u] = t + u * 1024 < np ? params[t + u * 1024] : 0.f;
  adam_sq_sums(w, np, red, sh);
  if (t == 0) adam_aux_store(aux, sh[0], sqrtf(sh[1]), sqrtf(sh[2]), bpow[0], bpow[1]);
}

int dp_args(const hdg_dp* dp, DpArgs& a) {
  if (!dp) return fail(HDG_EINVAL, "NULL hdg_dp");
  if (dp->world < 1 || dp->world > HDG_DP_MAX_WORLD || dp->rank < 0 || dp->rank >= dp->world)
    return fail(HDG_EINVAL, "hdg_dp: rank %d / world %d out of range (world <= %d)", dp->rank,
                dp->world, HDG_DP_MAX_WORLD);
  if (dp->flags & ~HDG_DP_SHARED) return fail(HDG_EINVAL, "hdg_dp: unknown flags 0x%x", dp->flags);
  memset(&a, 0, sizeof(a));
  for (int r = 0; r < dp->world; ++r) {
    if (!dp->mailbox[r]) return fail(HDG_EINVAL, "hdg_dp: mailbox of rank %d is NULL", r);
    a.box[r] = (uint32_t*)dp->mailbox[r];
  }
  a.rank = dp->rank;
  a.world = dp->world;
  a.wait = dp->wait_ticks ? dp->wait_ticks : dpk::WAIT_DEFAULT;
  return 0;
}
// blocks per rank of the shared-device tail: as many as keep the W - 1 waiting ranks'
// spinning blocks on at most half of the CUs (at least HDG_DP_SHARED_BLOCKS: 15 x 8 = 120
// <= 128 at HDG_DP_MAX_WORLD), at most one per slot group
unsigned dp_shared_grid(int n, int world) {
  const int groups = (n + RED_P - 1) / RED_P;
  const int cus = cu_count() > 0 ? cu_count() : 256;
  int g = cus / (2 * (world > 1 ? world - 1 : 1));
  if (g < HDG_DP_SHARED_BLOCKS) g = HDG_DP_SHARED_BLOCKS;
  return (unsigned)(groups < g ? groups : g);
}
float* dp_aux(const hdg_dp* dp) {
  return (float*)((char*)dp->mailbox[dp->rank] + dpk::OFF_AUX);
}

}  // namespace

extern "C" {

static_assert(sizeof(hipIpcMemHandle_t) == HDG_DP_HANDLE_BYTES, "IPC handle size");

size_t hdg_dp_mailbox_bytes(void) { return dpk::BYTES; }

int hdg_dp_mailbox_alloc(void** mailbox, void* handle) {
  if (!mailbox || !handle) return fail(HDG_EINVAL, "NULL mailbox/handle pointer");
  *mailbox = nullptr;
  // uncached: the peers' write-through words and this rank's polling loads meet in memory
  HIP_TRY(hipExtMallocWithFlags(mailbox, dpk::BYTES, hipDeviceMallocUncached));
  hipIpcMemHandle_t h;
  hipError_t e = hipMemset(*mailbox, 0, dpk::BYTES);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipIpcGetMemHandle(&h, *mailbox);
  if (e != hipSuccess) {
    (void)hipFree(*mailbox);
    *mailbox = nullptr;
    return fail((int)e, "mailbox setup: %s", hipGetErrorString(e));
  }
  memcpy(handle, &h, sizeof(h));
  return 0;
}

int hdg_dp_mailbox_open(const void* handle, void** mailbox) {
  if (!mailbox || !handle) return fail(HDG_EINVAL, "NULL mailbox/handle pointer");
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  *mailbox = nullptr;
  HIP_TRY(hipIpcOpenMemHandle(mailbox, h, hipIpcMemLazyEnablePeerAccess));
  return 0;
}

int hdg_dp_mailbox_close(void* mailbox) {
  HIP_TRY(hipIpcCloseMemHandle(mailbox));
  return 0;
}

int hdg_dp_mailbox_free(void* mailbox) {
  HIP_TRY(hipFree(mailbox));
  return 0;
}

int hdg_dp_allreduce(const hdg_dp* dp, const float* in, float* out, int32_t n, uint32_t* status,
                     void* stream) {
  DpArgs a;
  if (int rc = dp_args(dp, a)) return rc;
  if (!in || !out || n < 1 || n > HDG_DP_MAX_LEN)
    return fail(HDG_EINVAL, "hdg_dp_allreduce: NULL buffer or n=%d outside [1, %d]", n,
                HDG_DP_MAX_LEN);
  if (dp_shared(dp))
    hipLaunchKernelGGL(k_dp_tail_shared<dpk::SUM>, dim3(dp_shared_grid(n, a.world)), dim3(DP_NT_LIGHT), 0,
                       (hipStream_t)stream, in, 0, n, out, nullptr, nullptr, nullptr, nullptr,
                       nullptr, 0.f, 0.f, nullptr, status, a);
  else
    hipLaunchKernelGGL(k_dp_tail<dpk::SUM>, dim3((n + RED_P - 1) / RED_P), dim3(DP_NT_LIGHT), 0,
                       (hipStream_t)stream, in, 1, 0, n, out, nullptr, nullptr, nullptr, nullptr,
                       nullptr, 0.f, 0.f, nullptr, status, 0, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int hdg_adam_dp(const hdg_shape* s, hdg_state* state, const float* grad_local, float* grad_out,
                float lr, float* stats, uint32_t* status, const hdg_dp* dp, void* stream) {
  RESOLVE(s, path);
  (void)path;
  DpArgs a;
  if (int rc = dp_args(dp, a)) return rc;
  if (!state || !state->params || !state->adam_m || !state->adam_v || !state->beta_pow ||
      !grad_local || !grad_out)
    return fail(HDG_EINVAL, "NULL state/grad pointer");
  const int np = hdg::param_offsets(s->variant).NP, glen = np + HDG_TRAILER;
  hipStream_t st = (hipStream_t)stream;
  float* aux = dp_aux(dp);
  hipLaunchKernelGGL(k_dp_aux, dim3(1), dim3(1024), 0, st, state->params, np, state->beta_pow,
                     aux);
  if (dp_shared(dp))
    hipLaunchKernelGGL(k_dp_tail_shared<dpk::GRAD>, dim3(dp_shared_grid(glen, a.world)), dim3(DP_NT_LIGHT),
                       0, st, grad_local, np, glen, grad_out, state->params, state->adam_m,
                       state->adam_v, state->beta_pow, aux, lr, 1.f / pair_count(s), stats,
                       status, a);
  else
    hipLaunchKernelGGL(k_dp_tail<dpk::GRAD>, dim3((glen + RED_P - 1) / RED_P), dim3(DP_NT_LIGHT),
                       0, st, grad_local, 1, np, glen, grad_out, state->params, state->adam_m,
                       state->adam_v, state->beta_pow, aux, lr, 1.f / pair_count(s), stats,
                       status, 0, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"

namespace hdg {

int dp_check(const hdg_dp* dp) {
  DpArgs a;
  return dp_args(dp, a);
}
bool dp_shared(const hdg_dp* dp) { return (dp->flags & HDG_DP_SHARED) != 0; }
float* dp_local_grad(const hdg_dp* dp) {
  return (float*)((char*)dp->mailbox[dp->rank] + dpk::OFF_GLOC);
}

int launch_dp_tail_part(const hdg_dp* dp, const float* part, int rows, int fault_rows,
                        float* grad, hdg_state* state, const float* aux, float lr,
                        float inv_pairs, float* stats, uint32_t* status, hipStream_t st) {
  DpArgs a;
  if (int rc = dp_args(dp, a)) return rc;
  hipLaunchKernelGGL(k_dp_tail<dpk::PART>, dim3((GRAD_LEN + RED_P - 1) / RED_P), dim3(1024), 0,
                     st, part, rows, m2::NP, GRAD_LEN, grad, state->params,
                     state->adam_m, state->adam_v, state->beta_pow, aux, lr, inv_pairs,
                     stats, status, fault_rows, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace hdg
