// unionfind.h -- what the decoders of the pair scores share: untangle.hip (hdg_untangle),
// linkage.hip (hdg_linkage), agglo.hip (hdg_agglomerate, hdg_cut) and refine.hip (hdg_refine).
//   tiles         ut_tiles, ut_blocks, ut_tile_pair: the 64 x 64 tile pairs of the hunk grid
//   staging       ut_scores, ut_stage: a tile pair's scores and their mirror into two LDS tiles
//   visit         ut_visit: every p < q of a staged tile pair with its two scores; ut_weight
//   counts        ut_count_put, ut_count_sum: a block-wide count, fixed order, one writer
//   union-find    ut_find, ut_union, ut_label, ut_unite_labels, ut_true_groups
//   pair table    ut_pair_counts, ut_pair_table: slots HDG_UT_GROUPS .. HDG_UT_DD of a row
//   host          ut_check_shape, ut_check_rule, ut_check_workspace, ut_link_bound, ut_launched
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

// the slots every pair table shares: ut_pair_table fills HDG_UT_GROUPS .. HDG_UT_DD of
// hdg_refine's row, and hdg_cut's row is hdg_untangle's slot for slot
static_assert(HDG_UT_GROUPS == 0 && HDG_UT_TGROUPS == 1 && HDG_UT_SS == 2 && HDG_UT_SD == 3 &&
              HDG_UT_DS == 4 && HDG_UT_DD == 5, "the table slots are 0 .. 5");
static_assert(HDG_CUT_GROUPS == HDG_UT_GROUPS && HDG_CUT_TGROUPS == HDG_UT_TGROUPS &&
              HDG_CUT_SS == HDG_UT_SS && HDG_CUT_SD == HDG_UT_SD && HDG_CUT_DS == HDG_UT_DS &&
              HDG_CUT_DD == HDG_UT_DD && HDG_CUT_SLOTS == HDG_UT_SLOTS, "hdg_cut's row");
static_assert(HDG_RF_MOVES == HDG_UT_DD + 1 && HDG_RF_NAN == HDG_UT_DD + 2 &&
              HDG_RF_SLOTS == HDG_UT_SLOTS, "hdg_refine's row: HDG_UT_* in slots 0 .. 5");

// ---- tiles: the hunk grid cut into UT_T x UT_T tiles, the tile pairs (I, J), I <= J ----------
__host__ __device__ inline int ut_tiles(const int nc) {
  const int T = (nc + UT_T - 1) / UT_T;
  return T * (T + 1) / 2;
}
__host__ __device__ inline int ut_blocks(const int nc) {
  const int n = (ut_tiles(nc) + HDG_UT_TILES_PER_BLOCK - 1) / HDG_UT_TILES_PER_BLOCK;
  return n < HDG_UT_MAX_BLOCKS ? n : HDG_UT_MAX_BLOCKS;
}
// tile pair k < ut_tiles(nc), row-major over I <= J -> its first hunks p0 = 64 I, q0 = 64 J
__device__ __forceinline__ void ut_tile_pair(const int k, const int nc, int& p0, int& q0) {
  const int T = (nc + UT_T - 1) / UT_T;
  int I = 0, rem = k;
  while (rem >= T - I) {
    rem -= T - I;
    ++I;
  }
  p0 = I * UT_T;
  q0 = (I + rem) * UT_T;
}

// commit b's scores (channel 1 of probs [B][2][nc (nc - 1)]) and its label rows
__device__ __forceinline__ const float* ut_scores(const float* __restrict__ probs, const int b,
                                                  const int nc) {
  const size_t ncr = (size_t)nc * (nc - 1);
  return probs + (size_t)b * 2 * ncr + ncr;
}
__device__ __forceinline__ const uint32_t* ut_label_rows(const uint32_t* __restrict__ ybits,
                                                         const int b, const int nc) {
  return ybits + (size_t)b * nc * ((nc + 31) >> 5);
}

// Stages the I x J segment of the scores s and its mirror J x I segment into two tiles of
// UT_T * UT_LD words: sa[a][c] = s(p0 + a, q0 + c), sb[c][a] = s(q0 + c, p0 + a), 0 off the
// grid and on the diagonal.  Row-coalesced loads; the [q > p] shift of r(p, q) moves inside
// a row where the tile crosses the diagonal.  Rows are 65 words apart, so a half-wave hits 32
// banks by row and by column.  Block of UT_LINK_NT threads; the barriers are the caller's.
__device__ __forceinline__ void ut_stage(const float* __restrict__ s, const int nc, const int p0,
                                         const int q0, float* sa, float* sb) {
  const int n1 = nc - 1;
  for (int idx = threadIdx.x; idx < UT_T * UT_T; idx += UT_LINK_NT) {
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
}

// Visits every p < q < nc of a staged tile pair once: f(u, a, c, p, q, s_pq, s_qp) with
// p = p0 + a, q = q0 + c and u < UT_VISITS the thread's visit number (unrolled: an array
// indexed by u stays in registers).  A wave takes a row of the I x J segment, or with
// MIRROR a row of the mirror segment (c by wave, a by lane: stores at (q, p) coalesce).
constexpr int UT_VISITS = UT_T * UT_T / UT_LINK_NT;
template <bool MIRROR = false, class F>
__device__ __forceinline__ void ut_visit(const int nc, const int p0, const int q0, const float* sa,
                                         const float* sb, F&& f) {
#pragma unroll
  for (int u = 0; u < UT_VISITS; ++u) {
    const int idx = (int)threadIdx.x + u * UT_LINK_NT;
    const int a = MIRROR ? idx & 63 : idx >> 6, c = MIRROR ? idx >> 6 : idx & 63;
    const int p = p0 + a, q = q0 + c;
    if (p < q && q < nc) f(u, a, c, p, q, sa[a * UT_LD + c], sb[c * UT_LD + a]);
  }
}

// The weight of the unordered pair {p, q} under `rule` from its two scores (include/hdgnn.h,
// hdg_linkage) -> w, -0 taken as +0; false when the pair is not an edge: a NaN score in
// either direction, or +inf and -inf under MEAN.  The one statement of the rule: hdg_linkage,
// hdg_agglomerate and hdg_refine count what is no edge; hdg_untangle links w > t' and counts
// NaN scores alone (w is NaN for +inf and -inf under MEAN, which compares false).
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

// Block-wide counts in a fixed order with a single writer, no atomics: every wave leaves its
// sums of the N values v... in red (WAVES * N words); the caller synchronises; ut_count_sum
// adds the waves' sums of value i up as a T, in any thread that wants the total.
template <class... V>
__device__ __forceinline__ void ut_count_put(uint32_t* red, const V... v) {
  constexpr int N = sizeof...(V);
  const int tid = threadIdx.x;
  const uint32_t sum[N] = {ut_wave_sum(v)...};
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[(tid >> 6) * N + i] = sum[i];
  }
}
template <class T, int WAVES, int N = 1>
__device__ __forceinline__ T ut_count_sum(const uint32_t* red, const int i) {
  T v = 0;
  for (int w = 0; w < WAVES; ++w) v += (T)red[w * N + i];
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

// The true groups of a commit: the components of its label graph (yb: ut_label_rows) as dense
// ids in t; returns their number.  par, rnk, wsum as ut_label's, free on entry.  Whole block of
// UT_CLOSE_NT threads, synchronised on entry and on return.
__device__ __forceinline__ uint32_t ut_true_groups(uint32_t* par, uint32_t* rnk, uint32_t* t,
                                                   uint32_t* wsum, const uint32_t* __restrict__ yb,
                                                   const int nc) {
  for (int i = threadIdx.x; i < nc; i += UT_CLOSE_NT) par[i] = (uint32_t)i;
  __syncthreads();
  ut_unite_labels(par, yb, nc);
  __syncthreads();
  return ut_label(par, rnk, t, wsum, nc);
}

// The pair counts of two labelings g, t of 0 .. nc-1 (LDS, block synchronised): this thread's
// q against every p < q -> the waves' sums of same-g, same-t and same-both in red
// (UT_CLOSE_WAVES * 3 words).  The caller synchronises; then one thread calls ut_pair_table.
__device__ __forceinline__ void ut_pair_counts(const uint32_t* g, const uint32_t* t, uint32_t* red,
                                               const int nc) {
  const int tid = threadIdx.x;
  uint32_t gq[UT_PER], tq[UT_PER];
#pragma unroll
  for (int u = 0; u < UT_PER; ++u) {
    const int q = tid + u * UT_CLOSE_NT;
    gq[u] = q < nc ? g[q] : 0u;
    tq[u] = q < nc ? t[q] : 0u;
  }
  uint32_t same_p = 0, same_t = 0, ss = 0;
  for (int p = 0; p < nc - 1; ++p) {
    const uint32_t gp = g[p], tp = t[p];
#pragma unroll
    for (int u = 0; u < UT_PER; ++u) {
      const int q = tid + u * UT_CLOSE_NT;
      if (q > p && q < nc) {
        const uint32_t ep = gq[u] == gp, et = tq[u] == tp;
        same_p += ep;
        same_t += et;
        ss += ep & et;
      }
    }
  }
  ut_count_put(red, same_p, same_t, ss);
}
// ... and slots HDG_UT_GROUPS .. HDG_UT_DD of a table row from them; slots 6 and 7 are the
// caller's.
__device__ __forceinline__ void ut_pair_table(const uint32_t* red, const uint32_t G,
                                              const uint32_t TG, const int nc,
                                              unsigned long long* row) {
  typedef unsigned long long u64;
  const u64 sp = ut_count_sum<u64, UT_CLOSE_WAVES, 3>(red, 0);
  const u64 st = ut_count_sum<u64, UT_CLOSE_WAVES, 3>(red, 1);
  const u64 s2 = ut_count_sum<u64, UT_CLOSE_WAVES, 3>(red, 2);
  const u64 all = (u64)nc * (u64)(nc - 1) / 2ull;
  row[HDG_UT_GROUPS] = G;
  row[HDG_UT_TGROUPS] = TG;
  row[HDG_UT_SS] = s2;
  row[HDG_UT_SD] = sp - s2;
  row[HDG_UT_DS] = st - s2;
  row[HDG_UT_DD] = all - sp - st + s2;
}

// ---- host side of an entry point: `who` is its name, the prefix of every message ------------
inline int ut_check_shape(const hdg_shape* s, const char* who) {
  if (!s) return hdg::fail(HDG_EINVAL, "%s: shape is NULL", who);
  if (s->batch < 1 || s->batch > 65535)
    return hdg::fail(HDG_EINVAL, "%s: batch must be in [1, 65535] (got %d)", who, s->batch);
  if (s->nc < 2 || s->nc > UT_MAXN)
    return hdg::fail(HDG_EINVAL, "%s: nc must be in [2, 2048] (got %d)", who, s->nc);
  return 0;
}
inline int ut_check_rule(const int32_t rule, const char* who) {
  if (rule != HDG_UT_RULE_MEAN && rule != HDG_UT_RULE_ANY && rule != HDG_UT_RULE_BOTH)
    return hdg::fail(HDG_EINVAL, "%s: unknown rule %d (HDG_UT_RULE_MEAN / _ANY / _BOTH)", who,
                     (int)rule);
  return 0;
}
inline int ut_check_workspace(const void* workspace, const char* who) {
  if ((uintptr_t)workspace & 7u)
    return hdg::fail(HDG_EINVAL, "%s: workspace must be 8-byte aligned", who);
  return 0;
}
// The link bound t' of (rule, threshold): fl32(threshold + threshold) under MEAN, threshold
// otherwise.  The volatile makes the sum one fp32 addition of a stored fp32 value, rounded
// once, whatever the host compiler would fold or keep in a wider register.
inline float ut_link_bound(const int32_t rule, const float threshold) {
  volatile float two = threshold;
  return rule == HDG_UT_RULE_MEAN ? two + two : threshold;
}
// After a launch: 0, or the launch error as "<who>: launch (<stage>): ..." (stage may be NULL).
inline int ut_launched(const char* who, const char* stage) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  if (!stage) return hdg::fail((int)e, "%s: launch: %s", who, hipGetErrorString(e));
  return hdg::fail((int)e, "%s: launch (%s): %s", who, stage, hipGetErrorString(e));
}

}  // namespace
