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
//   k_lk_forest  grid (ut_blocks(nc), B), 512 threads: k_ut_link's tile pairs and staging.
//                The block keeps a running forest of at most nc - 1 keys in LDS (the forest
//                of a union of edge sets is the forest of the union of their forests) and,
//                per tile pair, runs Boruvka rounds over {that forest} + {the tile's <= 4096
//                keys, held in registers}.  The forest (padded with 0) and the block's NaN
//                count go to the workspace.
//   k_lk_close   grid B, 1024 threads.  Boruvka over the keys of the commit's block forests,
//                a bitonic sort of the M survivors (descending: Kruskal's acceptance order)
//                -> merges, levels; the true groups as k_ut_close builds them; the
//                dendrogram order of the hunks (one thread walks the merges, appending the
//                list of the cluster with the larger minimum to the other's tail and storing
//                k on the boundary; the cluster's root under min-root hooking is its list's
//                head); then two hunks at positions i < j join at merge
//                max(boundary[i .. j-1]): every thread sweeps j upward from its i with a
//                running maximum, counts pairs and same-true pairs in registers and flushes
//                them to dSP[k] / dSS[k] when the maximum changes; an inclusive scan over k
//                gives the curve.
// Integer and bit results only; the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "unionfind.h"

namespace {

using hdg::fail;
typedef unsigned long long u64;

constexpr int LK_EPT = UT_T * UT_T / UT_LINK_NT;      // tile edges per thread of k_lk_forest
constexpr int LK_MAX_ROUNDS = 32;                     // > ceil(log2 2048) + 1: never reached
constexpr uint32_t LK_NEVER = 0xFFFFFFFFu;            // a boundary no merge crosses
static_assert(UT_MAXN == 2048, "the key's low word packs p * 2048 + q");
static_assert(UT_PER == 2, "the scan of the curve takes two rows per thread");

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

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, b = blockIdx.y;
  const int n1 = nc - 1;
  const size_t ncr = (size_t)nc * n1;
  const float* s = probs + (size_t)b * 2 * ncr + ncr;     // channel 1
  const int T = (nc + UT_T - 1) / UT_T, tiles = T * (T + 1) / 2;

  uint32_t nans = 0, m = 0;                // m: keys of the running forest, forest[cur]
  int cur = 0;
  for (int k = blk; k < tiles; k += nblk) {
    int I = 0, rem = k;                    // tile pair k, row-major over I <= J
    while (rem >= T - I) {
      rem -= T - I;
      ++I;
    }
    const int p0 = I * UT_T, q0 = (I + rem) * UT_T;
    __syncthreads();                       // the last tile pair's rounds are over
    for (int idx = tid; idx < UT_T * UT_T; idx += UT_LINK_NT) {
      const int row = idx >> 6, col = idx & 63;
      int p = p0 + row, q = q0 + col;      // a row of the I x J segment
      float v = 0.f;
      if (p < nc && q < nc && p != q) v = s[(size_t)p * n1 + q - (q > p)];
      sa[row * UT_LD + col] = v;
      p = q0 + row, q = p0 + col;          // a row of the mirror segment
      v = 0.f;
      if (p < nc && q < nc && p != q) v = s[(size_t)p * n1 + q - (q > p)];
      sb[row * UT_LD + col] = v;
    }
    for (int i = tid; i < nc; i += UT_LINK_NT) parent[i] = (uint32_t)i;
    if (tid == 0) count = 0u;
    __syncthreads();
    u64 key[LK_EPT];                       // this thread's edges of the tile pair, 0 = none
#pragma unroll
    for (int u = 0; u < LK_EPT; ++u) {
      const int idx = tid + u * UT_LINK_NT;
      const int a = idx >> 6, c = idx & 63;
      const int p = p0 + a, q = q0 + c;
      key[u] = 0ull;
      if (p < q && q < nc) {
        const float spq = sa[a * UT_LD + c], sqp = sb[c * UT_LD + a];
        float w;
        if (rule == HDG_UT_RULE_MEAN) w = spq + sqp;
        else if (rule == HDG_UT_RULE_ANY) w = spq > sqp ? spq : sqp;
        else w = spq < sqp ? spq : sqp;
        // a NaN score in either direction, or +inf and -inf under MEAN: not an edge
        if (spq != spq || sqp != sqp || w != w) ++nans;
        else key[u] = lk_key(w, p, q);
      }
    }
    const u64* old = forest[cur];
    u64* out = forest[cur ^ 1];
    uint32_t have = 0;
    for (int round = 0; round < LK_MAX_ROUNDS; ++round) {
      lk_snapshot<UT_LINK_NT>(parent, comp, best, nc);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < LK_EPT; ++u)     // a key inside one component stays inside it
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
  nans = ut_wave_sum(nans);
  if (lane == 0) red[wave] = nans;
  __syncthreads();
  if (tid == 0) {
    u64 v = 0;
    for (int w = 0; w < UT_LINK_WAVES; ++w) v += red[w];
    wb[(size_t)nblk * n1 + blk] = v;
  }
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
  __shared__ uint32_t t[UT_MAXN];          // true group ids
  __shared__ uint32_t bseq[UT_MAXN];       // bseq[i]: the merge that joins positions i, i + 1
  __shared__ uint32_t tpos[UT_MAXN];       // true group of the hunk at position i
  __shared__ uint32_t dsp[UT_MAXN];        // pairs first joined by merge k
  __shared__ uint32_t dss[UT_MAXN];        // ... that are also in one true group
  __shared__ uint32_t wsum[UT_CLOSE_WAVES];
  __shared__ uint32_t wsum2[UT_CLOSE_WAVES][2];
  __shared__ uint32_t red[UT_CLOSE_WAVES];
  __shared__ uint32_t count;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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

  // ---- true groups: the set bits of the commit's label rows -------------------------------
  for (int i = tid; i < nc; i += UT_CLOSE_NT) par[i] = (uint32_t)i;
  __syncthreads();
  ut_unite_labels(par, ybits + (size_t)b * nc * ((nc + 31) >> 5), nc);
  __syncthreads();
  const uint32_t TG = ut_label(par, comp, t, wsum, nc);
  if (tgroups)
    for (int i = tid; i < nc; i += UT_CLOSE_NT) tgroups[(size_t)b * nc + i] = (int32_t)t[i];

  // ---- dendrogram order: one thread walks the merges ----------------------------------------
  uint32_t* nxt = reinterpret_cast<uint32_t*>(best);
  uint32_t* tail = nxt + UT_MAXN;
  uint32_t* bnd = comp;
  for (int i = tid; i < nc; i += UT_CLOSE_NT) {
    par[i] = (uint32_t)i;
    tail[i] = (uint32_t)i;
    nxt[i] = LK_NEVER;
    bnd[i] = LK_NEVER;
    dsp[i] = 0u;
    dss[i] = 0u;
  }
  __syncthreads();
#ifdef HDG_LK_STAMP_WALK     // diagnostic build: the walk's 100 MHz ticks go to lk slot 7
  u64 walk_ticks = 0;
  if (tid == 0) walk_ticks = __builtin_amdgcn_s_memrealtime();
#endif
  if (tid == 0) {
    for (int k = 0; k < M; ++k) {
      const u64 key = fk[k];
      uint32_t x = lk_p(key), y = lk_q(key);
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
  st = ut_wave_sum(st);
  if (lane == 0) red[wave] = st;
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
  uint32_t* cv = curve + (size_t)b * n1 * 2;
  if (k0 < n1) {
    cv[2 * k0] = k0 < M ? cp0 : totp;
    cv[2 * k0 + 1] = k0 < M ? cs0 : tots;
  }
  if (k0 + 1 < n1) {
    cv[2 * k0 + 2] = k0 + 1 < M ? cp0 + p1 : totp;
    cv[2 * k0 + 3] = k0 + 1 < M ? cs0 + s1 : tots;
  }
  if (tid == 0) {
    u64 sts = 0, nans = 0;
    for (int w = 0; w < UT_CLOSE_WAVES; ++w) sts += red[w];
    for (int f = 0; f < nblk; ++f) nans += wb[(size_t)nblk * n1 + f];
    u64* row = lk + (size_t)b * HDG_LK_SLOTS;
    row[HDG_LK_MERGES] = (u64)M;
    row[HDG_LK_TGROUPS] = TG;
    row[HDG_LK_ST] = sts;
    row[HDG_LK_NAN] = nans;
    row[HDG_LK_PAIRS] = (u64)nc * (u64)n1 / 2ull;
    row[5] = row[6] = row[7] = 0ull;
#ifdef HDG_LK_STAMP_WALK
    row[7] = walk_ticks;
#endif
  }
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
  if (rule != HDG_UT_RULE_MEAN && rule != HDG_UT_RULE_ANY && rule != HDG_UT_RULE_BOTH)
    return fail(HDG_EINVAL, "hdg_linkage: unknown rule %d (HDG_UT_RULE_MEAN / _ANY / _BOTH)",
                (int)rule);
  if (!bt || !bt->ybits || !probs || !merges || !levels || !curve || !lk || !workspace)
    return fail(HDG_EINVAL, "hdg_linkage: NULL pointer (batch, batch->ybits, probs, merges, "
                            "levels, curve, lk or workspace)");
  if ((uintptr_t)workspace & 7u)
    return fail(HDG_EINVAL, "hdg_linkage: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ut_blocks(s->nc);
  hipLaunchKernelGGL(k_lk_forest, dim3((unsigned)nblk, (unsigned)s->batch), dim3(UT_LINK_NT), 0, st,
                     probs, (u64*)workspace, s->nc, nblk, (int)rule);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "hdg_linkage: launch (forest): %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_lk_close, dim3((unsigned)s->batch), dim3(UT_CLOSE_NT), 0, st,
                     (const u64*)workspace, bt->ybits, merges, levels, curve, tgroups,
                     (u64*)lk, s->nc, nblk);
  e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "hdg_linkage: launch (close): %s", hipGetErrorString(e));
  return 0;
}
