// linkage.hip -- the single-linkage merge tree of a commit's hunks (hdg_linkage,
// include/hdgnn.h): every partition hdg_untangle can cut out of the pair scores, at every
// threshold at once, with the pair counts of each against the true groups.
//
// The partition is a step function of the threshold and changes only at the edge weights of
// the maximum spanning forest of the pair weights.  An edge is a 64-bit key: the
// order-preserving bit pattern of its weight in the high word, the complement of
// p * 2048 + q in the low word, so a larger key is an earlier edge of the header's total
// order (w descending, p ascending, q ascending) and 0 is no edge.  Because the order is
// total the forest is unique, and Boruvka rounds (every component takes its largest
// outgoing key) can never close a cycle, whatever order the threads run in.
//
// Two launches, neither waits for another block:
//   k_lk_forest  grid (ut_blocks(nc), B), 512 threads: the tile pairs, staging and visit
//                k_ut_link uses (ut_tile_pair, ut_stage, ut_visit), the weight by ut_weight.
//                The block keeps a running forest of at most nc - 1 keys in LDS (the forest
//                of a union of edge sets is the forest of the union of their forests) and,
//                per tile pair, runs Boruvka rounds over {that forest} + {the tile's <= 4096
//                keys, held in registers}.  The forest (padded with 0) and the block's NaN
//                count go to the workspace.
//   k_lk_close   grid B, 1024 threads.  Boruvka over the keys of the commit's block forests,
//                a bitonic sort of the M survivors (descending: Kruskal's acceptance order)
//                -> merges, levels; then the closing phase hdg_agglomerate shares
//                (treeclose.h): the true groups (ut_true_groups), the dendrogram
//                order of the hunks, the pairs each merge joins, and their inclusive scan
//                over k, the curve.
// Integer and bit results only; the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "treeclose.h"
#include "unionfind.h"

namespace {

using hdg::fail;
typedef unsigned long long u64;

constexpr int LK_MAX_ROUNDS = 32;                     // > ceil(log2 2048) + 1: never reached
static_assert(UT_MAXN == 2048, "the key's low word packs p * 2048 + q");

// workspace, in 8-byte words per commit: nblk forests of nc - 1 keys, then nblk NaN counts
__host__ __device__ inline size_t lk_commit_words(const int nc, const int nblk) {
  return (size_t)nblk * (size_t)nc;
}

__device__ __forceinline__ u64 lk_key(const float w, const int p, const int q) {
  uint32_t u = __float_as_uint(w);
  if (u == 0x80000000u) u = 0u;                       // -0 is taken as +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((u64)u << 32) | (u64)(~(uint32_t)(p * UT_MAXN + q));
}
__device__ __forceinline__ float lk_level(const u64 key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ uint32_t lk_p(const u64 key) { return (~(uint32_t)key) >> 11; }
__device__ __forceinline__ uint32_t lk_q(const u64 key) { return (~(uint32_t)key) & (UT_MAXN - 1); }

// A round's first half: comp <- every node's root, best <- 0.  The caller synchronises.
template <int NT>
__device__ __forceinline__ void lk_snapshot(uint32_t* parent, uint32_t* comp, u64* best,
                                            const int nc) {
  for (int i = threadIdx.x; i < nc; i += NT) {
    comp[i] = ut_find(parent, (uint32_t)i);
    best[i] = 0ull;
  }
}
// Offers a key to the components of both its ends; false when it lies inside one.
__device__ __forceinline__ bool lk_offer(const uint32_t* comp, u64* best, const u64 key) {
  const uint32_t cp = comp[lk_p(key)], cq = comp[lk_q(key)];
  if (cp == cq) return false;
  atomicMax(&best[cp], key);
  atomicMax(&best[cq], key);
  return true;
}
// A round's second half (block synchronised after the offers): every component unites
// along its best key and the key is appended to out once -- by the smaller root where both
// ends chose it.  Reads comp and best only, so the unions of other threads do not disturb
// it.  The caller synchronises and reads *count.
template <int NT>
__device__ __forceinline__ void lk_take(uint32_t* parent, const uint32_t* comp, const u64* best,
                                        u64* out, uint32_t* count, const int nc) {
  for (int c = threadIdx.x; c < nc; c += NT) {
    if (comp[c] != (uint32_t)c) continue;
    const u64 key = best[c];
    if (!key) continue;
    const uint32_t p = lk_p(key), q = lk_q(key);
    const uint32_t cp = comp[p], other = cp == (uint32_t)c ? comp[q] : cp;
    if (best[other] != key || (uint32_t)c < other) {
      const uint32_t slot = atomicAdd(count, 1u);
      if (slot < (uint32_t)(nc - 1)) out[slot] = key;     // a forest has at most nc - 1 edges
    }
    ut_union(parent, p, q);
  }
}

__global__ __launch_bounds__(UT_LINK_NT) void k_lk_forest(const float* __restrict__ probs,
                                                          u64* __restrict__ ws, const int nc,
                                                          const int nblk, const int rule) {
  __shared__ float sa[UT_T * UT_LD];       // sa[a][c] = s(64 I + a, 64 J + c)
  __shared__ float sb[UT_T * UT_LD];       // sb[c][a] = s(64 J + c, 64 I + a)
  __shared__ u64 forest[2][UT_MAXN];       // the running forest, and the one being built
  __shared__ u64 best[UT_MAXN];
  __shared__ uint32_t parent[UT_MAXN];
  __shared__ uint32_t comp[UT_MAXN];
  __shared__ uint32_t red[UT_LINK_WAVES];
  __shared__ uint32_t count;

  const int tid = threadIdx.x;
  const int blk = blockIdx.x, b = blockIdx.y;
  const int n1 = nc - 1;
  const float* s = ut_scores(probs, b, nc);
  const int tiles = ut_tiles(nc);

  uint32_t nans = 0, m = 0;                // m: keys of the running forest, forest[cur]
  int cur = 0;
  for (int k = blk; k < tiles; k += nblk) {
    int p0, q0;
    ut_tile_pair(k, nc, p0, q0);
    __syncthreads();                       // the last tile pair's rounds are over
    ut_stage(s, nc, p0, q0, sa, sb);
    for (int i = tid; i < nc; i += UT_LINK_NT) parent[i] = (uint32_t)i;
    if (tid == 0) count = 0u;
    __syncthreads();
    u64 key[UT_VISITS] = {};               // this thread's edges of the tile pair, 0 = none
    ut_visit(nc, p0, q0, sa, sb,
             [&](const int u, int, int, const int p, const int q, const float spq,
                 const float sqp) {
               float w;
               if (!ut_weight(rule, spq, sqp, w)) ++nans;
               else key[u] = lk_key(w, p, q);
             });
    const u64* old = forest[cur];
    u64* out = forest[cur ^ 1];
    uint32_t have = 0;
    for (int round = 0; round < LK_MAX_ROUNDS; ++round) {
      lk_snapshot<UT_LINK_NT>(parent, comp, best, nc);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < UT_VISITS; ++u)  // a key inside one component stays inside it
        if (key[u] && !lk_offer(comp, best, key[u])) key[u] = 0ull;
      for (uint32_t i = tid; i < m; i += UT_LINK_NT) lk_offer(comp, best, old[i]);
      __syncthreads();
      lk_take<UT_LINK_NT>(parent, comp, best, out, &count, nc);
      __syncthreads();
      const uint32_t now = count;          // the next write to it is two barriers away
      if (now == have) break;              // uniform: nothing crosses two components
      have = now;
    }
    m = have < (uint32_t)n1 ? have : (uint32_t)n1;
    cur ^= 1;
  }
  __syncthreads();

  u64* wb = ws + (size_t)b * lk_commit_words(nc, nblk);
  const u64* f = forest[cur];
  for (int i = tid; i < n1; i += UT_LINK_NT) wb[(size_t)blk * n1 + i] = (uint32_t)i < m ? f[i] : 0ull;
  ut_count_put(red, nans);
  __syncthreads();
  if (tid == 0) wb[(size_t)nblk * n1 + blk] = ut_count_sum<u64, UT_LINK_WAVES>(red, 0);
}

__global__ __launch_bounds__(UT_CLOSE_NT) void k_lk_close(const u64* __restrict__ ws,
                                                          const uint32_t* __restrict__ ybits,
                                                          int32_t* __restrict__ merges,
                                                          float* __restrict__ levels,
                                                          uint32_t* __restrict__ curve,
                                                          int32_t* __restrict__ tgroups,
                                                          u64* __restrict__ lk, const int nc,
                                                          const int nblk) {
  __shared__ u64 fk[UT_MAXN];              // the commit's merges, sorted
  __shared__ u64 best[UT_MAXN];            // after the rounds: nxt | tail
  __shared__ uint32_t par[UT_MAXN];
  __shared__ uint32_t comp[UT_MAXN];       // then ut_label's ranks, then bnd
  __shared__ uint32_t count;

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int n1 = nc - 1;
  const u64* wb = ws + (size_t)b * lk_commit_words(nc, nblk);

  // ---- the commit's forest: Boruvka over the blocks' forests ------------------------------
  for (int i = tid; i < nc; i += UT_CLOSE_NT) par[i] = (uint32_t)i;
  if (tid == 0) count = 0u;
  __syncthreads();
  const int nkeys = nblk * n1;
  uint32_t have = 0;
  for (int round = 0; round < LK_MAX_ROUNDS; ++round) {
    lk_snapshot<UT_CLOSE_NT>(par, comp, best, nc);
    __syncthreads();
    for (int i = tid; i < nkeys; i += UT_CLOSE_NT) {
      const u64 key = wb[i];
      if (key) lk_offer(comp, best, key);
    }
    __syncthreads();
    lk_take<UT_CLOSE_NT>(par, comp, best, fk, &count, nc);
    __syncthreads();
    const uint32_t now = count;
    if (now == have) break;                // uniform
    have = now;
  }
  const int M = (int)(have < (uint32_t)n1 ? have : (uint32_t)n1);

  // ---- Kruskal's order: bitonic sort, descending, over the next power of two --------------
  int n2 = 1;
  while (n2 < n1) n2 <<= 1;
  for (int i = M + tid; i < n2; i += UT_CLOSE_NT) fk[i] = 0ull;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += UT_CLOSE_NT) {
        const int x = i ^ j;
        if (x > i) {
          const u64 a = fk[i], c = fk[x];
          if ((i & k) == 0 ? a < c : a > c) {
            fk[i] = c;
            fk[x] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int k = tid; k < n1; k += UT_CLOSE_NT) {
    const size_t o = (size_t)b * n1 + k;
    const u64 key = fk[k];
    merges[2 * o] = k < M ? (int32_t)lk_p(key) : -1;
    merges[2 * o + 1] = k < M ? (int32_t)lk_q(key) : -1;
    levels[o] = k < M ? lk_level(key) : __uint_as_float(0x7FC00000u);
  }

  // ---- true groups, dendrogram order, pair counts, curve and the lk row: treeclose.h --------
  unsigned long long nans = 0;             // fk is read-only from the sort's last barrier on
  if (tid == 0)
    for (int f = 0; f < nblk; ++f) nans += wb[(size_t)nblk * n1 + f];
  tc_close(par, comp, reinterpret_cast<uint32_t*>(best),
           [&](const int k, uint32_t& x, uint32_t& y) {
             const u64 key = fk[k];
             x = lk_p(key);
             y = lk_q(key);
           },
           M, nans, ut_label_rows(ybits, b, nc), curve + (size_t)b * n1 * 2,
           tgroups ? tgroups + (size_t)b * nc : nullptr, lk + (size_t)b * HDG_LK_SLOTS, nc);
}

}  // namespace

extern "C" size_t hdg_linkage_workspace_bytes(const hdg_shape* s) {
  if (ut_check_shape(s, "hdg_linkage_workspace_bytes")) return 0;
  return (size_t)s->batch * lk_commit_words(s->nc, ut_blocks(s->nc)) * sizeof(u64);
}

extern "C" int hdg_linkage(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                           int32_t rule, int32_t* merges, float* levels, uint32_t* curve,
                           int32_t* tgroups, uint64_t* lk, void* workspace, void* stream) {
  if (const int rc = ut_check_shape(s, "hdg_linkage")) return rc;
  if (const int rc = ut_check_rule(rule, "hdg_linkage")) return rc;
  if (!bt || !bt->ybits || !probs || !merges || !levels || !curve || !lk || !workspace)
    return fail(HDG_EINVAL, "hdg_linkage: NULL pointer (batch, batch->ybits, probs, merges, "
                            "levels, curve, lk or workspace)");
  if (const int rc = ut_check_workspace(workspace, "hdg_linkage")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ut_blocks(s->nc);
  hipLaunchKernelGGL(k_lk_forest, dim3((unsigned)nblk, (unsigned)s->batch), dim3(UT_LINK_NT), 0, st,
                     probs, (u64*)workspace, s->nc, nblk, (int)rule);
  if (const int rc = ut_launched("hdg_linkage", "forest")) return rc;
  hipLaunchKernelGGL(k_lk_close, dim3((unsigned)s->batch), dim3(UT_CLOSE_NT), 0, st,
                     (const u64*)workspace, bt->ybits, merges, levels, curve, tgroups,
                     (u64*)lk, s->nc, nblk);
  return ut_launched("hdg_linkage", "close");
}
