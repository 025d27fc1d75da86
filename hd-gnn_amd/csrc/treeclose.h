// treeclose.h -- the closing phase of a merge tree, shared by linkage.hip (hdg_linkage) and
// agglo.hip (hdg_agglomerate): from a commit's M merges in array order and its label bits,
// the true groups, the dendrogram order of the hunks, the pairs each merge joins and their
// inclusive scan -- curve, tgroups and the lk row of include/hdgnn.h, slot for slot.
//
// One thread walks the merges, appending the list of the cluster with the larger minimum to
// the other's tail and storing k on the boundary (the cluster's root under min-root hooking
// is its list's head); two hunks at positions i < j then join at merge
// max(boundary[i .. j-1]): every thread sweeps j upward from its i with a running maximum,
// counts pairs and same-true pairs in registers and flushes them to dsp[k] / dss[k] when the
// maximum changes; an inclusive scan over k gives the curve.  Integer results only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "unionfind.h"

namespace {

constexpr uint32_t TC_NEVER = 0xFFFFFFFFu;            // a boundary no merge crosses
static_assert(UT_PER == 2, "the scan of the curve takes two rows per thread");

// Whole block of UT_CLOSE_NT threads, uniform control flow, block synchronised on entry.
//   par, comp   UT_MAXN words each, free on entry (the walk's forest; ranks, then boundaries)
//   nxt         2 * UT_MAXN words, free on entry (the lists' links | their tails)
//   yb          the commit's label rows (ut_label_rows)
//   pq(k, x, y) the ends of merge k < M, read by thread 0 only
//   nans        the commit's not-an-edge pairs (thread 0's value is used)
// The function's own arrays (true groups, positions, the per-merge counts) are LDS of the
// calling kernel.
template <class PQ>
__device__ __forceinline__ void tc_close(uint32_t* par, uint32_t* comp, uint32_t* nxt, const PQ pq,
                                         const int M, const unsigned long long nans,
                                         const uint32_t* __restrict__ yb,
                                         uint32_t* __restrict__ cv, int32_t* __restrict__ tg,
                                         unsigned long long* __restrict__ row, const int nc) {
  __shared__ uint32_t t[UT_MAXN];          // true group ids
  __shared__ uint32_t bseq[UT_MAXN];       // bseq[i]: the merge that joins positions i, i + 1
  __shared__ uint32_t tpos[UT_MAXN];       // true group of the hunk at position i
  __shared__ uint32_t dsp[UT_MAXN];        // pairs first joined by merge k
  __shared__ uint32_t dss[UT_MAXN];        // ... that are also in one true group
  __shared__ uint32_t wsum[UT_CLOSE_WAVES];
  __shared__ uint32_t wsum2[UT_CLOSE_WAVES][2];
  __shared__ uint32_t red[UT_CLOSE_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = nc - 1;

  const uint32_t TG = ut_true_groups(par, comp, t, wsum, yb, nc);
  if (tg)
    for (int i = tid; i < nc; i += UT_CLOSE_NT) tg[i] = (int32_t)t[i];

  // ---- dendrogram order: one thread walks the merges ----------------------------------------
  uint32_t* tail = nxt + UT_MAXN;
  uint32_t* bnd = comp;
  for (int i = tid; i < nc; i += UT_CLOSE_NT) {
    par[i] = (uint32_t)i;
    tail[i] = (uint32_t)i;
    nxt[i] = TC_NEVER;
    bnd[i] = TC_NEVER;
    dsp[i] = 0u;
    dss[i] = 0u;
  }
  __syncthreads();
#ifdef HDG_LK_STAMP_WALK     // diagnostic build: the walk's 100 MHz ticks go to lk slot 7
  unsigned long long walk_ticks = 0;
  if (tid == 0) walk_ticks = __builtin_amdgcn_s_memrealtime();
#endif
  if (tid == 0) {
    for (int k = 0; k < M; ++k) {
      uint32_t x, y;
      pq(k, x, y);
      while (par[x] != x) {
        par[x] = par[par[x]];
        x = par[x];
      }
      while (par[y] != y) {
        par[y] = par[par[y]];
        y = par[y];
      }
      if (x == y) continue;                // not reached: the merges are a forest
      const uint32_t lo = x < y ? x : y, hi = x < y ? y : x;
      const uint32_t tl = tail[lo];
      nxt[tl] = hi;                        // hi is the head of its list: its cluster's minimum
      bnd[tl] = (uint32_t)k;
      tail[lo] = tail[hi];
      par[hi] = lo;
    }
    if (M < n1) {                          // several trees: chain them, no merge between them
      uint32_t prev = 0;
      for (int i = 1; i < nc; ++i)
        if (par[i] == (uint32_t)i) {
          nxt[tail[prev]] = (uint32_t)i;
          prev = (uint32_t)i;
        }
    }
    uint32_t node = 0;
    for (int pos = 0; pos < nc && node < (uint32_t)nc; ++pos) {
      tpos[pos] = t[node];
      bseq[pos] = bnd[node];
      node = nxt[node];
    }
  }
#ifdef HDG_LK_STAMP_WALK
  if (tid == 0) walk_ticks = __builtin_amdgcn_s_memrealtime() - walk_ticks;
#endif
  __syncthreads();

  // ---- the pairs each merge joins: position i against every j > i --------------------------
  uint32_t st = 0;
  for (int i = tid; i < n1; i += UT_CLOSE_NT) {
    const uint32_t ti = tpos[i];
    uint32_t mx = bseq[i], cnt = 0, same = 0;
    for (int j = i + 1; j < nc; ++j) {
      const uint32_t bj = bseq[j - 1];
      if (bj > mx) {
        if (cnt && mx < (uint32_t)M) {
          atomicAdd(&dsp[mx], cnt);
          if (same) atomicAdd(&dss[mx], same);
        }
        mx = bj;
        cnt = same = 0;
      }
      const uint32_t e = tpos[j] == ti;
      ++cnt;
      same += e;
      st += e;
    }
    if (cnt && mx < (uint32_t)M) {
      atomicAdd(&dsp[mx], cnt);
      if (same) atomicAdd(&dss[mx], same);
    }
  }
  ut_count_put(red, st);
  __syncthreads();

  // ---- curve: inclusive scan over k, rows 2 tid and 2 tid + 1 ------------------------------
  const int k0 = 2 * tid;
  const uint32_t p0 = k0 < M ? dsp[k0] : 0u, p1 = k0 + 1 < M ? dsp[k0 + 1] : 0u;
  const uint32_t s0 = k0 < M ? dss[k0] : 0u, s1 = k0 + 1 < M ? dss[k0 + 1] : 0u;
  uint32_t ip = p0 + p1, is = s0 + s1;     // -> inclusive over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t vp = (uint32_t)__shfl_up((int)ip, o, 64), vs = (uint32_t)__shfl_up((int)is, o, 64);
    if (lane >= o) {
      ip += vp;
      is += vs;
    }
  }
  if (lane == 63) {
    wsum2[wave][0] = ip;
    wsum2[wave][1] = is;
  }
  __syncthreads();
  uint32_t offp = 0, offs = 0, totp = 0, tots = 0;
  for (int w = 0; w < UT_CLOSE_WAVES; ++w) {
    const uint32_t vp = wsum2[w][0], vs = wsum2[w][1];
    offp += w < wave ? vp : 0u;
    offs += w < wave ? vs : 0u;
    totp += vp;
    tots += vs;
  }
  const uint32_t cp0 = offp + ip - p1, cs0 = offs + is - s1;     // row k0; row k0 + 1 adds p1, s1
  if (k0 < n1) {
    cv[2 * k0] = k0 < M ? cp0 : totp;
    cv[2 * k0 + 1] = k0 < M ? cs0 : tots;
  }
  if (k0 + 1 < n1) {
    cv[2 * k0 + 2] = k0 + 1 < M ? cp0 + p1 : totp;
    cv[2 * k0 + 3] = k0 + 1 < M ? cs0 + s1 : tots;
  }
  if (tid == 0) {
    const unsigned long long sts = ut_count_sum<unsigned long long, UT_CLOSE_WAVES>(red, 0);
    row[HDG_LK_MERGES] = (unsigned long long)M;
    row[HDG_LK_TGROUPS] = TG;
    row[HDG_LK_ST] = sts;
    row[HDG_LK_NAN] = nans;
    row[HDG_LK_PAIRS] = (unsigned long long)nc * (unsigned long long)n1 / 2ull;
    row[5] = row[6] = row[7] = 0ull;
#ifdef HDG_LK_STAMP_WALK
    row[7] = walk_ticks;
#endif
  }
}

}  // namespace
