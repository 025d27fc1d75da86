// eval.hip -- on-device evaluation of the hunk-edge classifier (hdg_eval, include/hdgnn.h).
//
// From the probabilities a forward or training launch left on the device ([B][2][Ncr],
// C_edge_output2) and the batch's label bits, per commit: the confusion counts of the
// argmax prediction (np.argmax tie rule, as the gradient trailer's top_ACC count) and
// U2 = sum over (positive p, negative n) pairs of 2 [s_p > s_n] + [s_p == s_n], the
// Mann-Whitney statistic doubled, so ROC-AUC = U2 / (2 P N) exactly (ties count half, as
// sklearn.metrics.roc_auc_score).  Only B x HDG_EV_SLOTS integers ever leave the device;
// the reference scores on the host (EvaluationFuncs.py) after fetching every probability.
//
// One launch, grid (ceil(Ncr / HDG_EVAL_CHUNK), B), 1024 threads.  Block (c, b):
//   1. walks the relations of chunk c of commit b once: counts TP / FP / FN / TN / NAN
//      (one integer atomicAdd per slot) and writes each relation's sort key into LDS -- the
//      order-preserving bit pattern of s = probs[b][1][r] for a negative without NaN, the
//      all-ones sentinel for everything else and for the padding;
//   2. bitonic-sorts the keys ascending (64 KiB of LDS: two blocks per CU); the m real
//      keys (m = the chunk's FP + TN) end up in front;
//   3. streams ALL positives of commit b (label words 32 at a time, zero words skipped),
//      and for each one without NaN adds lb + ub of its key among the m sorted negatives
//      (lower / upper bound: 2 lb + (ub - lb)); one 64-bit atomicAdd of the block's sum.
// Every relation lies in one chunk, every (positive, negative) pair is seen by the one block
// that holds the negative, and all sums are integers: the result is exact and the same bits
// whatever order the blocks run in.  No block waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"

namespace {

using hdg::fail;

constexpr int EV_NT = 1024;                 // threads per block
constexpr int EV_WAVES = EV_NT / 64;
constexpr uint32_t EV_PAD = 0xFFFFFFFFu;    // sorts behind every real key

// float -> u32 whose unsigned order is the float order (-0.0 and +0.0 one key; NaN never
// gets here).  For the probabilities of a softmax (>= 0) this is the raw pattern with the
// top bit set.
__device__ __forceinline__ uint32_t ev_key(const float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}

__device__ __forceinline__ uint32_t ev_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned long long ev_wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(EV_NT) void k_eval(const float* __restrict__ probs,
                                                const uint32_t* __restrict__ ybits,
                                                unsigned long long* __restrict__ ev,
                                                const int nc, const int ncr) {
  __shared__ uint32_t keys[HDG_EVAL_CHUNK];
  __shared__ uint32_t red[EV_WAVES][5];
  __shared__ unsigned long long red64[EV_WAVES];
  __shared__ uint32_t m_sh;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const int W = (nc + 31) >> 5, n1 = nc - 1;
  const uint32_t* yb = ybits + (size_t)b * nc * W;
  const float* p0 = probs + (size_t)b * 2 * ncr;
  const float* p1 = p0 + ncr;
  unsigned long long* evb = ev + (size_t)b * HDG_EV_SLOTS;

  // the chunk's relations, and the power of two the sort covers (the keys behind it would
  // all be padding: already in place)
  const int r0 = c * HDG_EVAL_CHUNK;
  const int nrel = min(HDG_EVAL_CHUNK, ncr - r0);
  int nsort = 2;
  while (nsort < nrel) nsort <<= 1;

  // ---- 1. counts + keys ---------------------------------------------------------------
  uint32_t cnt[5] = {0u, 0u, 0u, 0u, 0u};   // slots TP FP FN TN, then NAN at [4]
  for (int k = tid; k < nsort; k += EV_NT) {
    uint32_t key = EV_PAD;
    if (k < nrel) {
      const int r = r0 + k;
      const int i = r / n1, jj = r - i * n1;
      const int j = jj + (jj >= i);
      const uint32_t lab = (yb[i * W + (j >> 5)] >> (j & 31)) & 1u;
      const float a = p0[r], s = p1[r];
      if (a != a || s != s) {
        ++cnt[4];
      } else {
        const uint32_t pred = s > a ? 1u : 0u;
        cnt[HDG_EV_TP] += lab & pred;
        cnt[HDG_EV_FP] += (lab ^ 1u) & pred;
        cnt[HDG_EV_FN] += lab & (pred ^ 1u);
        cnt[HDG_EV_TN] += (lab ^ 1u) & (pred ^ 1u);
        if (!lab) key = ev_key(s);
      }
    }
    keys[k] = key;
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const uint32_t v = ev_wave_sum(cnt[q]);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (tid < 5) {
    uint32_t v = 0;
    for (int w = 0; w < EV_WAVES; ++w) v += red[w][tid];
    if (v) atomicAdd(&evb[tid < 4 ? tid : HDG_EV_NAN], (unsigned long long)v);
  }
  if (tid == 0) {
    uint32_t v = 0;
    for (int w = 0; w < EV_WAVES; ++w) v += red[w][HDG_EV_FP] + red[w][HDG_EV_TN];
    m_sh = v;
  }
  __syncthreads();
  const int m = (int)m_sh;       // real keys: the chunk's negatives without NaN
  if (m == 0) return;            // the whole block leaves together

  // ---- 2. bitonic sort of keys[0 .. nsort) ascending ------------------------------------
  for (int k = 2; k <= nsort; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (nsort >> 1); t += EV_NT) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const uint32_t x = keys[lo], y = keys[hi];
        if ((x > y) == ((lo & k) == 0)) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
  }

  // ---- 3. every positive of the commit against the m sorted negatives -------------------
  unsigned long long acc = 0;
  const int nwords = nc * W;
  for (int w = tid; w < nwords; w += EV_NT) {
    uint32_t bits = yb[w];
    if (!bits) continue;
    const int i = w / W, jb = (w - i * W) << 5;
    while (bits) {
      const int j = jb + __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (j >= nc || j == i) continue;        // stray pad / diagonal bits: not relations
      const int r = i * n1 + j - (j > i);
      const float s = p1[r], a = p0[r];
      if (a != a || s != s) continue;
      const uint32_t key = ev_key(s);
      int lb = 0, n = m;                      // lb = #keys < key
      while (n > 0) {
        const int h = n >> 1;
        if (keys[lb + h] < key) {
          lb += h + 1;
          n -= h + 1;
        } else {
          n = h;
        }
      }
      int ub = lb;                            // ub = #keys <= key
      n = m - lb;
      while (n > 0) {
        const int h = n >> 1;
        if (keys[ub + h] <= key) {
          ub += h + 1;
          n -= h + 1;
        } else {
          n = h;
        }
      }
      acc += (unsigned long long)(lb + ub);   // 2 lb + (ub - lb)
    }
  }
  acc = ev_wave_sum64(acc);
  if (lane == 0) red64[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    unsigned long long v = 0;
    for (int w = 0; w < EV_WAVES; ++w) v += red64[w];
    if (v) atomicAdd(&evb[HDG_EV_U2], v);
  }
}

}  // namespace

extern "C" int hdg_eval(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                        uint64_t* ev, void* stream) {
  if (!s) return fail(HDG_EINVAL, "hdg_eval: shape is NULL");
  if (s->batch < 1 || s->batch > 65535)
    return fail(HDG_EINVAL, "hdg_eval: batch must be in [1, 65535] (got %d)", s->batch);
  if (s->nc < 2 || s->nc > 2048)
    return fail(HDG_EINVAL, "hdg_eval: nc must be in [2, 2048] (got %d)", s->nc);
  if (!bt || !bt->ybits || !probs || !ev)
    return fail(HDG_EINVAL, "hdg_eval: NULL pointer (batch, batch->ybits, probs or ev)");
  hipStream_t st = (hipStream_t)stream;
  const int ncr = s->nc * (s->nc - 1);
  hipError_t e = hipMemsetAsync(ev, 0, (size_t)s->batch * HDG_EV_SLOTS * sizeof(uint64_t), st);
  if (e != hipSuccess) return fail((int)e, "hdg_eval: hipMemsetAsync: %s", hipGetErrorString(e));
  const dim3 grid((unsigned)((ncr + HDG_EVAL_CHUNK - 1) / HDG_EVAL_CHUNK), (unsigned)s->batch);
  hipLaunchKernelGGL(k_eval, grid, dim3(EV_NT), 0, st, probs, bt->ybits,
                     (unsigned long long*)ev, s->nc, ncr);
  e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "hdg_eval: launch: %s", hipGetErrorString(e));
  return 0;
}
