// refine.hip -- best-move refinement of a commit's hunk groups (hdg_refine, include/hdgnn.h):
// local search on the correlation-clustering objective the linkages approximate, from any
// starting partition.  The definitions (fixed-point gains, start, sweep, tie rules, outputs)
// are the header's; every result is an integer and independent of summation order.
//
// Two launches, neither waits for another block:
//   k_rf_weights  grid (tile pairs, B), 512 threads: k_ag_weights' staging of the I x J segment
//                 of the scores and its mirror through two 64 x 65 LDS tiles, one tile pair
//                 per block.  Every p < q of the tile gets its weight (ut_weight) and from it
//                 the gain a_pq = rint(clamp(w - t') * 2^18), 0 for a pair that is no edge.
//                 The commit's region of the workspace holds the full nc x nc int32 matrix,
//                 written at (p, q) by rows of the segment and, through the second LDS tile,
//                 at (q, p) by rows of the mirror: both stores are row-coalesced, and the
//                 sweep reads a hunk's whole row contiguously.  The diagonal is written as 0.
//                 The block's count of pairs that are no edge follows the matrix.
//   k_rf_sweep    grid B, 1024 threads (thread h owns hunk h and slot h, and h + 1024 above
//                 1024).  Slots, slot sizes and two buffers of per-slot sums live in LDS; a
//                 thread keeps its own hunks' slots in registers.  The step over p is
//                 sequential.  A step: every q adds a_pq (row p of the workspace matrix,
//                 loaded one step ahead) into S[slot[q]] with an int32 LDS atomicAdd; barrier;
//                 every non-empty slot h != g offers (S[h], h), every empty one (0, h) if p is
//                 not alone, packed into one 64-bit key whose maximum is the header's choice
//                 (value, then non-empty before empty, then the lowest slot): wave maxima by
//                 DPP, the other buffer of sums is zeroed for the next step; barrier;
//                 every thread reads the wave maxima and reaches the same decision, the
//                 owner of p and thread 0 apply it.  Two barriers per step; what a step
//                 writes is read only after the next step's first barrier.  The sweep loop is
//                 bounded by max_sweeps, the step loop by nc, every inner loop by nc.  Then
//                 the final slots and the label graph are labelled (ut_label), the pairs
//                 counted as k_ut_close counts them, and groups, ut and rq written.
// Integer results only; the same bits on every run.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "unionfind.h"

namespace {

using hdg::fail;
typedef unsigned long long u64;

constexpr int RF_NT = UT_CLOSE_NT;
constexpr int RF_WAVES = RF_NT / 64;
constexpr float RF_SCALE = 262144.f;         // 2^18: a = rint(d * 2^18), |a| <= 2^19
static_assert(RF_NT * UT_PER == UT_MAXN, "a thread owns UT_PER hunks and slots");
static_assert((UT_MAXN - 1) * (1ll << 19) < (1ll << 31), "a node sum fits int32");
static_assert(UT_MAXN <= 2048, "the key's tie field holds two ranges of 2048 slots");

__host__ __device__ inline int rf_tiles(const int nc) {
  const int T = (nc + UT_T - 1) / UT_T;
  return T * (T + 1) / 2;
}
// workspace, in 4-byte words per commit: the nc x nc matrix of gains, then rf_tiles(nc)
// no-edge counts, rounded up to an even number of words
__host__ __device__ inline size_t rf_commit_words(const int nc) {
  return ((size_t)nc * (size_t)nc + (size_t)rf_tiles(nc) + 1) & ~(size_t)1;
}

// the fixed-point gain of a pair of weight w against the link bound tp (finite)
__device__ __forceinline__ int32_t rf_gain(const float w, const float tp) {
  const float d = w - tp;
  return (int32_t)rintf(fminf(fmaxf(d, -2.f), 2.f) * RF_SCALE);
}

__global__ __launch_bounds__(UT_LINK_NT) void k_rf_weights(const float* __restrict__ probs,
                                                           int32_t* __restrict__ ws, const int nc,
                                                           const int rule, const float tp) {
  __shared__ float sa[UT_T * UT_LD];       // sa[a][c] = s(64 I + a, 64 J + c)
  __shared__ float sb[UT_T * UT_LD];       // sb[c][a] = s(64 J + c, 64 I + a), then a's bits
  __shared__ uint32_t red[UT_LINK_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int n1 = nc - 1;
  const size_t ncr = (size_t)nc * n1;
  const float* s = probs + (size_t)b * 2 * ncr + ncr;     // channel 1
  const int T = (nc + UT_T - 1) / UT_T;
  int I = 0, rem = (int)blockIdx.x;        // this block's tile pair, row-major over I <= J
  while (rem >= T - I) {
    rem -= T - I;
    ++I;
  }
  const int p0 = I * UT_T, q0 = (I + rem) * UT_T;
  for (int idx = tid; idx < UT_T * UT_T; idx += UT_LINK_NT) {
    const int row = idx >> 6, col = idx & 63;
    int p = p0 + row, q = q0 + col;        // a row of the I x J segment
    float v = 0.f;
    if (p < nc && q < nc && p != q) v = s[(size_t)p * n1 + q - (q > p)];
    sa[row * UT_LD + col] = v;
    p = q0 + row, q = p0 + col;            // a row of the mirror segment
    v = 0.f;
    if (p < nc && q < nc && p != q) v = s[(size_t)p * n1 + q - (q > p)];
    sb[row * UT_LD + col] = v;
  }
  __syncthreads();
  int32_t* wb = ws + (size_t)b * rf_commit_words(nc);
  uint32_t nans = 0;
  for (int idx = tid; idx < UT_T * UT_T; idx += UT_LINK_NT) {
    const int a = idx >> 6, c = idx & 63;
    const int p = p0 + a, q = q0 + c;
    if (p < q && q < nc) {                 // only this thread reads or writes sb[c][a]
      float w;
      int32_t g = 0;
      if (ut_weight(rule, sa[a * UT_LD + c], sb[c * UT_LD + a], w)) g = rf_gain(w, tp);
      else ++nans;
      wb[(size_t)p * nc + q] = g;
      sb[c * UT_LD + a] = __int_as_float(g);
    } else if (p == q && q < nc) {
      wb[(size_t)p * nc + q] = 0;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < UT_T * UT_T; idx += UT_LINK_NT) {
    const int c = idx >> 6, a = idx & 63;  // a row of the mirror: (q, p) for the p < q above
    const int p = p0 + a, q = q0 + c;
    if (p < q && q < nc) wb[(size_t)q * nc + p] = __float_as_int(sb[c * UT_LD + a]);
  }
  nans = ut_wave_sum(nans);
  if (lane == 0) red[wave] = nans;
  __syncthreads();
  if (tid == 0) {
    uint32_t v = 0;
    for (int w = 0; w < UT_LINK_WAVES; ++w) v += red[w];
    reinterpret_cast<uint32_t*>(wb)[(size_t)nc * nc + blockIdx.x] = v;
  }
}

// a candidate of a step as one key: the larger key wins.  Value, then a non-empty slot
// before an empty one, then the lower slot.  0 is no candidate (|v| < 2^30).
__device__ __forceinline__ u64 rf_key(const int32_t v, const bool empty, const int h) {
  return ((u64)((uint32_t)v ^ 0x80000000u) << 12) | (u64)((empty ? 0 : 2048) + (2047 - h));
}

// max(k, the key CTRL brings from another lane); a lane without a source, or in a row ROWS
// masks out, gets 0, the identity
template <int CTRL, int ROWS>
__device__ __forceinline__ u64 rf_dpp_max(const u64 k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, ROWS, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, ROWS,
                                                            0xF, false);
  const u64 other = ((u64)hi << 32) | lo;
  return other > k ? other : k;
}

// the wave's largest key, in lane 63: DPP in the VALU, no LDS round trips
__device__ __forceinline__ u64 rf_wave_max(u64 k) {
  k = rf_dpp_max<0x111, 0xF>(k);           // row_shr:1
  k = rf_dpp_max<0x112, 0xF>(k);           // row_shr:2
  k = rf_dpp_max<0x114, 0xF>(k);           // row_shr:4
  k = rf_dpp_max<0x118, 0xF>(k);           // row_shr:8: lane 15 of a row holds the row's
  k = rf_dpp_max<0x142, 0xA>(k);           // row_bcast:15 into rows 1 and 3
  k = rf_dpp_max<0x143, 0xC>(k);           // row_bcast:31 into rows 2 and 3
  return k;
}

__device__ __forceinline__ long long rf_wave_sum64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// groups_in and groups may be the same array: a commit's ids are all read before the first
// barrier and written after the last
__global__ __launch_bounds__(RF_NT) void k_rf_sweep(const int32_t* __restrict__ ws,
                                                    const uint32_t* __restrict__ ybits,
                                                    const int32_t* gin, int32_t* groups,
                                                    u64* __restrict__ ut,
                                                    long long* __restrict__ rq, const int nc,
                                                    const int max_sweeps) {
  __shared__ int32_t S[2][UT_MAXN];        // the per-slot sums of this step and the next
  __shared__ int32_t slot[UT_MAXN];
  __shared__ int32_t size[UT_MAXN];
  __shared__ int32_t first[UT_MAXN];       // smallest member of a starting id / a final slot
  __shared__ uint32_t g[UT_MAXN];
  __shared__ uint32_t t[UT_MAXN];
  __shared__ u64 wkey[RF_WAVES];
  __shared__ long long wq[RF_WAVES];
  __shared__ uint32_t wsum[UT_CLOSE_WAVES];
  __shared__ uint32_t red[UT_CLOSE_WAVES][3];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int32_t* wb = ws + (size_t)b * rf_commit_words(nc);

  // ---- start: a group sits in the slot of its smallest member -------------------------------
  int32_t id[UT_PER], my[UT_PER], nx[UT_PER];
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    id[u] = -1;
    nx[u] = 0;
    if (i < nc) {
      if (gin) id[u] = gin[(size_t)b * nc + i];
      nx[u] = wb[i];                       // row 0 of the matrix, for step 0
      first[i] = 0x7FFFFFFF;
      size[i] = 0;
      S[0][i] = S[1][i] = 0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    if (i < nc && (uint32_t)id[u] < (uint32_t)nc) atomicMin(&first[id[u]], i);
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * RF_NT;
    my[u] = i;
    if (i < nc) {
      if ((uint32_t)id[u] < (uint32_t)nc) my[u] = first[id[u]];
      slot[i] = my[u];
      atomicAdd(&size[my[u]], 1);
    }
  }
  __syncthreads();

  // ---- Q at the start: this thread's q against every p < q of its slot ----------------------
  long long q_start = 0;
  if (gin) {                               // uniform; singletons have Q = 0
    for (int p = 0; p < nc - 1; ++p) {
      const int32_t sp = slot[p];
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int q = tid + u * RF_NT;
        if (q > p && q < nc && my[u] == sp) q_start += wb[(size_t)p * nc + q];
      }
    }
    q_start = rf_wave_sum64(q_start);
    if (lane == 0) wq[wave] = q_start;
    __syncthreads();
    q_start = 0;
    for (int w = 0; w < RF_WAVES; ++w) q_start += wq[w];
  }

  // ---- sweeps ------------------------------------------------------------------------------
  const int nwav = nc >= RF_NT ? RF_WAVES : (nc + 63) >> 6;     // the waves that own a slot
  int cur = 0, sweeps = 0, converged = 0;
  uint32_t moves = 0;
  long long gain = 0;
  for (int sw = 0; sw < max_sweeps; ++sw) {
    bool moved = false;
    for (int p = 0; p < nc; ++p) {
      int32_t a[UT_PER];
      const int32_t* nrow = wb + (size_t)(p + 1 < nc ? p + 1 : 0) * nc;
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int q = tid + u * RF_NT;
        a[u] = nx[u];
        nx[u] = q < nc ? nrow[q] : 0;      // the next step's row
        if (q < nc && q != p && a[u] != 0) atomicAdd(&S[cur][my[u]], a[u]);
      }
      __syncthreads();
      const int gs = slot[p];
      const int32_t stay = S[cur][gs];
      const bool roomy = size[gs] > 1;
      if (wave < nwav) {
        u64 key = 0;
#pragma unroll
        for (int u = 0; u < UT_PER; ++u) {
          const int h = tid + u * RF_NT;
          if (h < nc) {
            u64 k = 0;
            if (size[h] > 0) {
              if (h != gs) k = rf_key(S[cur][h], false, h);
            } else if (roomy) {
              k = rf_key(0, true, h);
            }
            key = k > key ? k : key;
          }
        }
        key = rf_wave_max(key);
        if (lane == 63) wkey[wave] = key;
      }
#pragma unroll
      for (int u = 0; u < UT_PER; ++u) {
        const int h = tid + u * RF_NT;
        if (h < nc) S[cur ^ 1][h] = 0;
      }
      __syncthreads();
      u64 best = 0;
      for (int w = 0; w < nwav; ++w) best = wkey[w] > best ? wkey[w] : best;
      const int32_t val = (int32_t)((uint32_t)(best >> 12) ^ 0x80000000u);
      if (best != 0 && val > stay) {       // uniform: every thread holds the same decision
        const int h = 2047 - (int)(best & 2047u);
#pragma unroll
        for (int u = 0; u < UT_PER; ++u)
          if (tid + u * RF_NT == p) my[u] = h;
        if (tid == 0) {
          slot[p] = h;
          size[gs] -= 1;
          size[h] += 1;
        }
        ++moves;
        gain += (long long)val - (long long)stay;
        moved = true;
      }
      cur ^= 1;
    }
    ++sweeps;
    if (!moved) {
      converged = 1;
      break;
    }
  }
  __syncthreads();

  // ---- predicted groups: the final slots, as a forest of smallest members -------------------
  uint32_t* par = reinterpret_cast<uint32_t*>(S[0]);      // the sums are done with
  uint32_t* rnk = reinterpret_cast<uint32_t*>(S[1]);
  for (int i = tid; i < nc; i += RF_NT) first[i] = 0x7FFFFFFF;
  __syncthreads();
  for (int i = tid; i < nc; i += RF_NT) atomicMin(&first[slot[i]], i);
  __syncthreads();
  for (int i = tid; i < nc; i += RF_NT) par[i] = (uint32_t)first[slot[i]];
  __syncthreads();
  const uint32_t G = ut_label(par, rnk, g, wsum, nc);

  // ---- true groups: the set bits of the commit's label rows ---------------------------------
  for (int i = tid; i < nc; i += RF_NT) par[i] = (uint32_t)i;
  __syncthreads();
  ut_unite_labels(par, ybits + (size_t)b * nc * ((nc + 31) >> 5), nc);
  __syncthreads();
  const uint32_t TG = ut_label(par, rnk, t, wsum, nc);

  // ---- pair counts: this thread's q against every p < q, as k_ut_close ----------------------
  uint32_t gq[UT_PER], tq[UT_PER];
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int q = tid + u * RF_NT;
    gq[u] = q < nc ? g[q] : 0u;
    tq[u] = q < nc ? t[q] : 0u;
  }
  uint32_t same_p = 0, same_t = 0, ss = 0;
  for (int p = 0; p < nc - 1; ++p) {
    const uint32_t gp = g[p], tp = t[p];
#pragma unroll
    for (int u = 0; u < UT_PER; ++u) {
      const int q = tid + u * RF_NT;
      if (q > p && q < nc) {
        const uint32_t ep = gq[u] == gp, et = tq[u] == tp;
        same_p += ep;
        same_t += et;
        ss += ep & et;
      }
    }
  }
  same_p = ut_wave_sum(same_p);
  same_t = ut_wave_sum(same_t);
  ss = ut_wave_sum(ss);
  if (lane == 0) {
    red[wave][0] = same_p;
    red[wave][1] = same_t;
    red[wave][2] = ss;
  }

  // ---- outputs ------------------------------------------------------------------------------
  for (int i = tid; i < nc; i += RF_NT) groups[(size_t)b * nc + i] = (int32_t)g[i];
  __syncthreads();
  if (tid == 0) {
    u64 sp = 0, st = 0, s2 = 0, nans = 0;
    for (int w = 0; w < UT_CLOSE_WAVES; ++w) {
      sp += red[w][0];
      st += red[w][1];
      s2 += red[w][2];
    }
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(wb) + (size_t)nc * nc;
    const int tiles = rf_tiles(nc);
    for (int f = 0; f < tiles; ++f) nans += cnt[f];
    const u64 all = (u64)nc * (u64)(nc - 1) / 2ull;
    u64* row = ut + (size_t)b * HDG_RF_SLOTS;
    row[HDG_UT_GROUPS] = G;
    row[HDG_UT_TGROUPS] = TG;
    row[HDG_UT_SS] = s2;
    row[HDG_UT_SD] = sp - s2;
    row[HDG_UT_DS] = st - s2;
    row[HDG_UT_DD] = all - sp - st + s2;
    row[HDG_RF_MOVES] = moves;
    row[HDG_RF_NAN] = nans;
    long long* qrow = rq + (size_t)b * HDG_RF_Q_SLOTS;
    qrow[HDG_RF_Q_START] = q_start;
    qrow[HDG_RF_Q_END] = q_start + gain;
    qrow[HDG_RF_Q_SWEEPS] = sweeps;
    qrow[HDG_RF_Q_CONVERGED] = converged;
  }
}

}  // namespace

extern "C" size_t hdg_refine_workspace_bytes(const hdg_shape* s, int32_t flags) {
  if (ut_check_shape(s, "hdg_refine_workspace_bytes")) return 0;
  (void)flags;                             // no flag is defined; hdg_refine rejects any bit
  return (size_t)s->batch * rf_commit_words(s->nc) * sizeof(int32_t);
}

extern "C" int hdg_refine(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                          float threshold, int32_t rule, int32_t max_sweeps, int32_t flags,
                          const int32_t* groups_in, int32_t* groups, uint64_t* ut, int64_t* rq,
                          void* workspace, void* stream) {
  if (const int rc = ut_check_shape(s, "hdg_refine")) return rc;
  if (rule != HDG_UT_RULE_MEAN && rule != HDG_UT_RULE_ANY && rule != HDG_UT_RULE_BOTH)
    return fail(HDG_EINVAL, "hdg_refine: unknown rule %d (HDG_UT_RULE_MEAN / _ANY / _BOTH)",
                (int)rule);
  if (max_sweeps < 1 || max_sweeps > HDG_RF_MAX_SWEEPS)
    return fail(HDG_EINVAL, "hdg_refine: max_sweeps must be in [1, %d] (got %d)",
                HDG_RF_MAX_SWEEPS, (int)max_sweeps);
  if (flags != 0) return fail(HDG_EINVAL, "hdg_refine: unknown flag bits 0x%x", (unsigned)flags);
  volatile float two = threshold;          // fl32(threshold + threshold), once, as hdg_untangle
  const float tp = rule == HDG_UT_RULE_MEAN ? two + two : threshold;
  if (!std::isfinite(threshold) || !std::isfinite(tp))
    return fail(HDG_EINVAL, "hdg_refine: threshold %g gives no finite link bound",
                (double)threshold);
  if (!bt || !bt->ybits || !probs || !groups || !ut || !rq || !workspace)
    return fail(HDG_EINVAL, "hdg_refine: NULL pointer (batch, batch->ybits, probs, groups, ut, "
                            "rq or workspace)");
  if ((uintptr_t)workspace & 7u)
    return fail(HDG_EINVAL, "hdg_refine: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nc = s->nc;
  hipLaunchKernelGGL(k_rf_weights, dim3((unsigned)rf_tiles(nc), (unsigned)s->batch),
                     dim3(UT_LINK_NT), 0, st, probs, (int32_t*)workspace, nc, (int)rule, tp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return fail((int)e, "hdg_refine: launch (weights): %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_rf_sweep, dim3((unsigned)s->batch), dim3(RF_NT), 0, st,
                     (const int32_t*)workspace, bt->ybits, groups_in, groups, (u64*)ut,
                     (long long*)rq, nc, (int)max_sweeps);
  e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "hdg_refine: launch (sweep): %s", hipGetErrorString(e));
  return 0;
}
