// unionfind.h -- the lock-free union-find in LDS, the component labelling, the tile geometry
// and the pair weight that untangle.hip (hdg_untangle), linkage.hip (hdg_linkage) and
// agglo.hip (hdg_agglomerate, hdg_cut) share.
//
// Union-find, lock-free with min-root hooking.  Invariant: parent[i] <= i, and parent[i]
// is always a node of i's own component.  find walks parent to a root (parent[r] == r) with
// atomic LDS loads; union finds both roots, returns when they are equal, else tries
// atomicCAS(&parent[hi], hi, lo) with hi > lo and on failure goes on from the value it read.
// A CAS fails only because another thread lowered that word, and words only ever decrease
// towards 0: the pair (hi, lo) a union holds strictly decreases with every failure, so every
// loop ends within 2 Nc steps and none waits for a particular thread.  Path halving stores
// parent[x] <- a value read as x's grandparent: a smaller node of the same tree, written only
// to non-roots (a non-root never becomes a root again, and the CAS only ever changes roots).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"

namespace {

constexpr int UT_T = HDG_UT_TILE;            // tile side
constexpr int UT_LD = UT_T + 1;              // padded LDS row stride (words)
constexpr int UT_MAXN = 2048;                // nc limit of the ABI
constexpr int UT_LINK_NT = 512;
constexpr int UT_LINK_WAVES = UT_LINK_NT / 64;
constexpr int UT_CLOSE_NT = 1024;
constexpr int UT_CLOSE_WAVES = UT_CLOSE_NT / 64;
constexpr int UT_PER = UT_MAXN / UT_CLOSE_NT;   // nodes per thread of the closing block

static_assert(UT_T == 64, "the tile visit maps one wave to one tile row");

__host__ __device__ inline int ut_blocks(const int nc) {
  const int T = (nc + UT_T - 1) / UT_T;
  const int tiles = T * (T + 1) / 2;
  const int n = (tiles + HDG_UT_TILES_PER_BLOCK - 1) / HDG_UT_TILES_PER_BLOCK;
  return n < HDG_UT_MAX_BLOCKS ? n : HDG_UT_MAX_BLOCKS;
}

// The weight of the unordered pair {p, q} under `rule` from its two scores (include/hdgnn.h,
// hdg_linkage) -> w, -0 taken as +0; false when the pair is not an edge: a NaN score in
// either direction, or +inf and -inf under MEAN.  The one statement hdg_linkage and
// hdg_agglomerate share.
__device__ __forceinline__ bool ut_weight(const int rule, const float spq, const float sqp,
                                          float& w) {
  if (rule == HDG_UT_RULE_MEAN) w = spq + sqp;
  else if (rule == HDG_UT_RULE_ANY) w = spq > sqp ? spq : sqp;
  else w = spq < sqp ? spq : sqp;
  if (__float_as_uint(w) == 0x80000000u) w = 0.f;
  return !(spq != spq || sqp != sqp || w != w);
}

__device__ __forceinline__ uint32_t ut_ld(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t ut_find(uint32_t* parent, uint32_t x) {
  uint32_t p = ut_ld(&parent[x]);
  while (p != x) {
    const uint32_t g = ut_ld(&parent[p]);
    if (g != p) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void ut_union(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = ut_find(parent, a);
    b = ut_find(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return;
    a = old;       // parent[hi] was lowered by someone else: old < hi, same component
    b = lo;
  }
}

__device__ __forceinline__ uint32_t ut_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o, 64);
  return v;
}

// par holds a forest over 0 .. nc-1 (all unions done, block synchronised).  Flattens it,
// numbers the roots in ascending order (the dense id of a root = the roots below it: a
// block-wide exclusive scan of the root flags) and writes every node's id to out.
// Returns the number of components.  Whole block of UT_CLOSE_NT threads, uniform control flow.
__device__ __forceinline__ uint32_t ut_label(uint32_t* par, uint32_t* rnk, uint32_t* out,
                                             uint32_t* wsum, const int nc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t r[UT_PER];
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * UT_CLOSE_NT;
    r[u] = i < nc ? ut_find(par, (uint32_t)i) : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * UT_CLOSE_NT;
    if (i < nc) par[i] = r[u];
  }
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    if (u * UT_CLOSE_NT >= nc) break;                       // uniform
    const int i = tid + u * UT_CLOSE_NT;
    const bool root = i < nc && r[u] == (uint32_t)i;
    const unsigned long long m = __ballot(root);
    const uint32_t pre = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = base, tot = 0;
    for (int w = 0; w < UT_CLOSE_WAVES; ++w) {
      const uint32_t v = wsum[w];
      off += w < wave ? v : 0u;
      tot += v;
    }
    if (i < nc) rnk[i] = off + pre;
    base += tot;
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int i = tid + u * UT_CLOSE_NT;
    if (i < nc) out[i] = rnk[r[u]];
  }
  __syncthreads();
  return base;
}

// Unites the set bits of a commit's label rows into par (identity on entry, block
// synchronised): the label graph y_pq | y_qp.  The caller synchronises afterwards.
__device__ __forceinline__ void ut_unite_labels(uint32_t* par, const uint32_t* __restrict__ yb,
                                                const int nc) {
  const int W = (nc + 31) >> 5, nwords = nc * W;
  for (int w = threadIdx.x; w < nwords; w += UT_CLOSE_NT) {
    uint32_t bits = yb[w];
    if (!bits) continue;
    const int i = w / W, jb = (w - i * W) << 5;
    while (bits) {
      const int j = jb + __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (j >= nc || j == i) continue;        // stray pad / diagonal bits: not relations
      ut_union(par, (uint32_t)i, (uint32_t)j);
    }
  }
}

inline int ut_check_shape(const hdg_shape* s, const char* who) {
  if (!s) return hdg::fail(HDG_EINVAL, "%s: shape is NULL", who);
  if (s->batch < 1 || s->batch > 65535)
    return hdg::fail(HDG_EINVAL, "%s: batch must be in [1, 65535] (got %d)", who, s->batch);
  if (s->nc < 2 || s->nc > UT_MAXN)
    return hdg::fail(HDG_EINVAL, "%s: nc must be in [2, 2048] (got %d)", who, s->nc);
  return 0;
}

}  // namespace
