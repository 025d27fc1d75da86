// agglo.hip -- agglomerative merge trees of a commit's hunks under single, complete and
// average linkage (hdg_agglomerate), and the groups of any merge tree at a threshold
// (hdg_cut).  The definitions are include/hdgnn.h's; the outputs are hdg_linkage's, slot for
// slot.
//
// hdg_agglomerate, three launches, neither waits for another block:
//   k_ag_weights  grid (ut_tiles(nc), B), 512 threads: the staging of the I x J segment of the
//                 scores and its mirror through two 64 x 65 LDS tiles (ut_stage), one tile
//                 pair per block.  Every p < q of the tile (ut_visit) gets its weight under the
//                 rule (ut_weight, the statement k_lk_forest uses; NaN stands for "no edge") at
//                 its place in the commit's region of the workspace: the upper triangle
//                 packed by rows, (x, y), x < y, at x nc - x (x + 1) / 2 + y - x - 1, so the
//                 partners c > x of a row are contiguous.  The block's count of pairs that
//                 are no edge follows the triangle.
//   k_ag_merge    grid B, 1024 threads, templated on the home of the cluster-pair matrix: a
//                 copy of the triangle in LDS (nc <= HDG_AG_LDS_MAX_NC) or the workspace
//                 region itself.  The matrix holds, for two live clusters, their fp32 weight
//                 (SINGLE, COMPLETE) or sum S (AVERAGE) at the place of their names.  Every
//                 live row a caches its best partner c > a under (D descending, c
//                 ascending).  A step: block arg-max over the caches under (D descending, a
//                 ascending); every other live x combines its entries with a and c into the
//                 one with a (max / NaN-absorbing min / one fp32 add) and, if x < a,
//                 compares the new entry with its cache in the full order; c retires; the
//                 rows whose cached partner was a or c, and row a, are rescanned, one wave
//                 per row.  At most nc - 1 steps; every inner loop runs over at most nc
//                 entries.
//   k_ag_close    grid B, 1024 threads: the merges in array order through treeclose.h, the
//                 closing phase k_lk_close runs -> curve, tgroups, lk.
// hdg_cut, one launch: k_cut, grid B, unites the merges above the bound in unionfind.h's
// forest and labels it with ut_label; its table comes off the curve, slot for slot
// hdg_untangle's (the static_asserts of unionfind.h).
// Integer and bit results only; the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "treeclose.h"
#include "unionfind.h"

namespace {

using hdg::fail;
typedef unsigned long long u64;

constexpr int AG_NT = 1024;
constexpr int AG_WAVES = AG_NT / 64;
constexpr int AG_LDS_N = HDG_AG_LDS_MAX_NC;
constexpr int AG_LDS_TRI = AG_LDS_N * (AG_LDS_N - 1) / 2;
static_assert(AG_LDS_N >= 160, "every fused-path shape keeps its matrix in LDS");
static_assert(AG_LDS_TRI * 4 + AG_LDS_N * 20 + 1024 <= 160 * 1024, "k_ag_merge's LDS budget");
static_assert(UT_MAXN * (UT_MAXN - 1) / 2 < (1 << 22), "the packed index fits 32 bits");

__host__ __device__ inline uint32_t ag_tri(const int nc) {
  return (uint32_t)nc * (uint32_t)(nc - 1) / 2u;
}
// workspace, in 4-byte words per commit: the packed triangle, then ut_tiles(nc) no-edge
// counts; nc (nc + 1) / 2 >= ut_tiles(nc) words are left after the triangle
__host__ __device__ inline size_t ag_commit_words(const int nc) { return (size_t)nc * (size_t)nc; }
__device__ __forceinline__ uint32_t ag_idx(const int x, const int y, const int nc) {   // x < y
  return (uint32_t)x * (uint32_t)nc - (uint32_t)x * (uint32_t)(x + 1) / 2u + (uint32_t)(y - x - 1);
}

__global__ __launch_bounds__(UT_LINK_NT) void k_ag_weights(const float* __restrict__ probs,
                                                           float* __restrict__ ws, const int nc,
                                                           const int rule) {
  __shared__ float sa[UT_T * UT_LD];       // sa[a][c] = s(64 I + a, 64 J + c)
  __shared__ float sb[UT_T * UT_LD];       // sb[c][a] = s(64 J + c, 64 I + a)
  __shared__ uint32_t red[UT_LINK_WAVES];

  const int b = blockIdx.y;
  int p0, q0;                              // this block's tile pair
  ut_tile_pair((int)blockIdx.x, nc, p0, q0);
  ut_stage(ut_scores(probs, b, nc), nc, p0, q0, sa, sb);
  __syncthreads();
  float* wb = ws + (size_t)b * ag_commit_words(nc);
  uint32_t nans = 0;
  ut_visit(nc, p0, q0, sa, sb,
           [&](int, int, int, const int p, const int q, const float spq, const float sqp) {
             float w;
             if (!ut_weight(rule, spq, sqp, w)) {
               ++nans;
               w = __uint_as_float(0x7FC00000u);
             }
             wb[ag_idx(p, q, nc)] = w;
           });
  ut_count_put(red, nans);
  __syncthreads();
  if (threadIdx.x == 0)
    reinterpret_cast<uint32_t*>(wb)[ag_tri(nc) + blockIdx.x] =
        ut_count_sum<uint32_t, UT_LINK_WAVES>(red, 0);
}

// (v, i) before (ov, oi) in the order (value descending, index ascending); an index < 0 is
// no candidate
__device__ __forceinline__ bool ag_before(const double v, const int i, const double ov, const int oi) {
  return i >= 0 && (oi < 0 || v > ov || (v == ov && i < oi));
}
__device__ __forceinline__ void ag_wave_first(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(v, o, 64);
    const int oi = __shfl_down(i, o, 64);
    if (ag_before(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}

template <bool LDS>
__global__ __launch_bounds__(AG_NT) void k_ag_merge(float* ws, int32_t* __restrict__ merges,
                                                    float* __restrict__ levels, const int nc,
                                                    const int method) {
  constexpr int MAXN = LDS ? AG_LDS_N : UT_MAXN;
  __shared__ float lmat[LDS ? AG_LDS_TRI : 1];
  __shared__ double bd[MAXN];              // D of row a and its cached partner
  __shared__ int bp[MAXN];                 // the cached partner c > a, -1: none
  __shared__ uint32_t sz[MAXN];            // members of cluster a, 0: retired
  __shared__ int list[MAXN];               // rows to rescan
  __shared__ int nlist;
  __shared__ double rd[AG_WAVES];
  __shared__ int ra[AG_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int n1 = nc - 1;
  float* gmat = ws + (size_t)b * ag_commit_words(nc);
  float* mat;
  if constexpr (LDS) {
    const uint32_t tri = ag_tri(nc);
    for (uint32_t i = tid; i < tri; i += AG_NT) lmat[i] = gmat[i];
    mat = lmat;
  } else {
    mat = gmat;
  }
  for (int i = tid; i < nc; i += AG_NT) {
    sz[i] = 1u;
    bp[i] = -1;
    bd[i] = 0.0;
  }
  if (tid == 0) nlist = 0;
  __syncthreads();

  const bool avg = method == HDG_AG_AVERAGE;
  // D of the live clusters x < y as a double; NaN: no edge
  auto val = [&](const int x, const int y) -> double {
    const double v = (double)mat[ag_idx(x, y, nc)];
    return avg ? v / (double)(sz[x] * sz[y]) : v;
  };
  // one wave: row x's first partner under (D descending, c ascending) -> its cache
  auto scan_row = [&](const int x) {
    double v = 0.0;
    int c = -1;
    for (int y = x + 1 + lane; y < nc; y += 64) {
      if (!sz[y]) continue;
      const double d = val(x, y);
      if (d == d && (c < 0 || d > v)) {    // y ascends: a tie keeps the smaller
        v = d;
        c = y;
      }
    }
    ag_wave_first(v, c);
    if (lane == 0) {
      bd[x] = v;
      bp[x] = c;
    }
  };
  for (int x = wave; x < n1; x += AG_WAVES) scan_row(x);
  __syncthreads();

  float run = 0.f;
  int M = 0;
  for (int k = 0; k < n1; ++k) {
    // ---- the first cluster pair under (D descending, a ascending) ---------------------------
    {
      double v = 0.0;
      int a = -1;
      for (int x = tid; x < n1; x += AG_NT) {
        if (!sz[x] || bp[x] < 0) continue;
        const double d = bd[x];
        if (a < 0 || d > v) {
          v = d;
          a = x;
        }
      }
      ag_wave_first(v, a);
      if (lane == 0) {
        rd[wave] = v;
        ra[wave] = a;
      }
      if (tid == 0) nlist = 0;
    }
    __syncthreads();
    double D = 0.0;
    int a = -1;
    for (int w = 0; w < AG_WAVES; ++w)
      if (ag_before(rd[w], ra[w], D, a)) {
        D = rd[w];
        a = ra[w];
      }
    if (a < 0) break;                      // uniform: no cluster pair has an edge
    const int c = bp[a];
    const uint32_t na = sz[a], ncl = sz[c];
    const float r = (float)D;
    run = k == 0 || r < run ? r : run;
    if (tid == 0) {
      const size_t o = (size_t)b * n1 + k;
      merges[2 * o] = a;
      merges[2 * o + 1] = c;
      levels[o] = run;
    }
    M = k + 1;

    // ---- a absorbs c: every other live x combines its two entries ---------------------------
    for (int x = tid; x < nc; x += AG_NT) {
      const uint32_t nx = sz[x];
      if (!nx || x == a || x == c) continue;
      const uint32_t ia = x < a ? ag_idx(x, a, nc) : ag_idx(a, x, nc);
      const float ma = mat[ia], mc = mat[x < c ? ag_idx(x, c, nc) : ag_idx(c, x, nc)];
      float m;
      if (avg) m = ma + mc;
      else if (method == HDG_AG_SINGLE) m = ma != ma ? mc : (mc != mc ? ma : (ma > mc ? ma : mc));
      else m = (ma != ma || mc != mc) ? __uint_as_float(0x7FC00000u) : (ma < mc ? ma : mc);
      mat[ia] = m;
      if (x > c) continue;                 // row x holds neither a nor c
      const int px = bp[x];
      if (px == c || (x < a && px == a)) {
        list[atomicAdd(&nlist, 1)] = x;    // its cached entry changed or is gone
      } else if (x < a) {                  // the new (x, a) against the cache, in the full order
        const double d = avg ? (double)m / (double)((na + ncl) * nx) : (double)m;
        if (d == d && ag_before(d, a, bd[x], px)) {
          bd[x] = d;
          bp[x] = a;
        }
      }
    }
    if (tid == 0) list[atomicAdd(&nlist, 1)] = a;
    __syncthreads();
    if (tid == 0) {
      sz[a] = na + ncl;
      sz[c] = 0u;
      bp[c] = -1;
    }
    __syncthreads();
    const int nl = nlist;                  // <= nc - 1: each row at most once
    for (int i = wave; i < nl; i += AG_WAVES) scan_row(list[i]);
    __syncthreads();
  }
  for (int k = M + tid; k < n1; k += AG_NT) {
    const size_t o = (size_t)b * n1 + k;
    merges[2 * o] = merges[2 * o + 1] = -1;
    levels[o] = __uint_as_float(0x7FC00000u);
  }
}

__global__ __launch_bounds__(UT_CLOSE_NT) void k_ag_close(const float* __restrict__ ws,
                                                          const uint32_t* __restrict__ ybits,
                                                          const int32_t* __restrict__ merges,
                                                          uint32_t* __restrict__ curve,
                                                          int32_t* __restrict__ tgroups,
                                                          u64* __restrict__ lk, const int nc) {
  __shared__ uint32_t mp[UT_MAXN];         // the commit's merges, in array order
  __shared__ uint32_t mq[UT_MAXN];
  __shared__ uint32_t par[UT_MAXN];
  __shared__ uint32_t comp[UT_MAXN];
  __shared__ uint32_t nxt[2 * UT_MAXN];
  __shared__ uint32_t cnt[UT_CLOSE_WAVES];

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int n1 = nc - 1;
  uint32_t have = 0;
  for (int k = tid; k < n1; k += UT_CLOSE_NT) {
    const int32_t p = merges[2 * ((size_t)b * n1 + k)], q = merges[2 * ((size_t)b * n1 + k) + 1];
    const bool real = p >= 0 && q > p && q < nc;
    mp[k] = real ? (uint32_t)p : 0u;
    mq[k] = real ? (uint32_t)q : 0u;
    have += real;
  }
  ut_count_put(cnt, have);
  __syncthreads();
  const int M = ut_count_sum<int, UT_CLOSE_WAVES>(cnt, 0);       // the real rows are a prefix
  u64 nans = 0;
  if (tid == 0) {
    const uint32_t* c = reinterpret_cast<const uint32_t*>(ws + (size_t)b * ag_commit_words(nc)) +
                        ag_tri(nc);
    const int tiles = ut_tiles(nc);
    for (int f = 0; f < tiles; ++f) nans += c[f];
  }
  tc_close(par, comp, nxt,
           [&](const int k, uint32_t& x, uint32_t& y) {
             x = mp[k];
             y = mq[k];
           },
           M, nans, ut_label_rows(ybits, b, nc), curve + (size_t)b * n1 * 2,
           tgroups ? tgroups + (size_t)b * nc : nullptr, lk + (size_t)b * HDG_LK_SLOTS, nc);
}

__global__ __launch_bounds__(UT_CLOSE_NT) void k_cut(const int32_t* __restrict__ merges,
                                                     const float* __restrict__ levels,
                                                     const uint32_t* __restrict__ curve,
                                                     const u64* __restrict__ lk, const float bound,
                                                     int32_t* __restrict__ groups,
                                                     u64* __restrict__ ut, const int nc) {
  __shared__ uint32_t par[UT_MAXN];
  __shared__ uint32_t rnk[UT_MAXN];
  __shared__ uint32_t g[UT_MAXN];
  __shared__ uint32_t wsum[UT_CLOSE_WAVES];
  __shared__ uint32_t red[UT_CLOSE_WAVES];

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int n1 = nc - 1;
  for (int i = tid; i < nc; i += UT_CLOSE_NT) par[i] = (uint32_t)i;
  __syncthreads();
  uint32_t done = 0;
  for (int k = tid; k < n1; k += UT_CLOSE_NT) {
    const size_t o = (size_t)b * n1 + k;
    const int32_t p = merges[2 * o], q = merges[2 * o + 1];
    if (levels[o] > bound && p >= 0 && q >= 0 && p < nc && q < nc) {     // NaN compares false
      ut_union(par, (uint32_t)p, (uint32_t)q);
      ++done;
    }
  }
  ut_count_put(red, done);
  __syncthreads();
  const uint32_t G = ut_label(par, rnk, g, wsum, nc);
  for (int i = tid; i < nc; i += UT_CLOSE_NT) groups[(size_t)b * nc + i] = (int32_t)g[i];
  if (ut && tid == 0) {
    uint32_t k = ut_count_sum<uint32_t, UT_CLOSE_WAVES>(red, 0);
    if (k > (uint32_t)n1) k = (uint32_t)n1;
    const u64 sp = k ? curve[2 * ((size_t)b * n1 + k - 1)] : 0ull;
    const u64 ss = k ? curve[2 * ((size_t)b * n1 + k - 1) + 1] : 0ull;
    const u64* in = lk + (size_t)b * HDG_LK_SLOTS;
    const u64 st = in[HDG_LK_ST];
    u64* row = ut + (size_t)b * HDG_CUT_SLOTS;
    row[HDG_CUT_GROUPS] = G;
    row[HDG_CUT_TGROUPS] = in[HDG_LK_TGROUPS];
    row[HDG_CUT_SS] = ss;
    row[HDG_CUT_SD] = sp - ss;
    row[HDG_CUT_DS] = st - ss;
    row[HDG_CUT_DD] = in[HDG_LK_PAIRS] - sp - st + ss;
    row[HDG_CUT_MERGES] = k;
    row[HDG_CUT_NAN] = in[HDG_LK_NAN];
  }
}

}  // namespace

extern "C" size_t hdg_agglomerate_workspace_bytes(const hdg_shape* s, int32_t flags) {
  if (ut_check_shape(s, "hdg_agglomerate_workspace_bytes")) return 0;
  (void)flags;                             // both homes of the matrix take the same region
  return (size_t)s->batch * ag_commit_words(s->nc) * sizeof(float);
}

extern "C" int hdg_agglomerate(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                               int32_t rule, int32_t method, int32_t flags, int32_t* merges,
                               float* levels, uint32_t* curve, int32_t* tgroups, uint64_t* lk,
                               void* workspace, void* stream) {
  if (const int rc = ut_check_shape(s, "hdg_agglomerate")) return rc;
  if (const int rc = ut_check_rule(rule, "hdg_agglomerate")) return rc;
  if (method != HDG_AG_SINGLE && method != HDG_AG_COMPLETE && method != HDG_AG_AVERAGE)
    return fail(HDG_EINVAL, "hdg_agglomerate: unknown method %d (HDG_AG_SINGLE / _COMPLETE / "
                            "_AVERAGE)", (int)method);
  if (flags & ~HDG_AG_FLAG_GLOBAL)
    return fail(HDG_EINVAL, "hdg_agglomerate: unknown flag bits 0x%x", (unsigned)flags);
  if (!bt || !bt->ybits || !probs || !merges || !levels || !curve || !lk || !workspace)
    return fail(HDG_EINVAL, "hdg_agglomerate: NULL pointer (batch, batch->ybits, probs, merges, "
                            "levels, curve, lk or workspace)");
  if (const int rc = ut_check_workspace(workspace, "hdg_agglomerate")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nc = s->nc;
  hipLaunchKernelGGL(k_ag_weights, dim3((unsigned)ut_tiles(nc), (unsigned)s->batch),
                     dim3(UT_LINK_NT), 0, st, probs, (float*)workspace, nc, (int)rule);
  if (const int rc = ut_launched("hdg_agglomerate", "weights")) return rc;
  if (nc <= HDG_AG_LDS_MAX_NC && !(flags & HDG_AG_FLAG_GLOBAL))
    hipLaunchKernelGGL(k_ag_merge<true>, dim3((unsigned)s->batch), dim3(AG_NT), 0, st,
                       (float*)workspace, merges, levels, nc, (int)method);
  else
    hipLaunchKernelGGL(k_ag_merge<false>, dim3((unsigned)s->batch), dim3(AG_NT), 0, st,
                       (float*)workspace, merges, levels, nc, (int)method);
  if (const int rc = ut_launched("hdg_agglomerate", "merge")) return rc;
  hipLaunchKernelGGL(k_ag_close, dim3((unsigned)s->batch), dim3(UT_CLOSE_NT), 0, st,
                     (const float*)workspace, bt->ybits, (const int32_t*)merges, curve, tgroups,
                     (u64*)lk, nc);
  return ut_launched("hdg_agglomerate", "close");
}

extern "C" int hdg_cut(const hdg_shape* s, const int32_t* merges, const float* levels,
                       const uint32_t* curve, const uint64_t* lk, float threshold, int32_t rule,
                       int32_t* groups, uint64_t* ut, void* stream) {
  if (const int rc = ut_check_shape(s, "hdg_cut")) return rc;
  if (const int rc = ut_check_rule(rule, "hdg_cut")) return rc;
  if (threshold != threshold) return fail(HDG_EINVAL, "hdg_cut: threshold is NaN");
  if (!merges || !levels || !groups)
    return fail(HDG_EINVAL, "hdg_cut: NULL pointer (merges, levels or groups)");
  if (ut && (!curve || !lk)) return fail(HDG_EINVAL, "hdg_cut: ut needs curve and lk");
  hipLaunchKernelGGL(k_cut, dim3((unsigned)s->batch), dim3(UT_CLOSE_NT), 0, (hipStream_t)stream,
                     merges, levels, curve, (const u64*)lk, ut_link_bound(rule, threshold), groups,
                     (u64*)ut, s->nc);
  return ut_launched("hdg_cut", nullptr);
}
