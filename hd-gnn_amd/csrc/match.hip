// match.hip -- on-device matching of hunk groups (hdg_match, include/hdgnn.h).
//
// From sets of predicted group ids ([n_sets][B][nc], any decoder's output) and the batch's
// label bits, per set and commit: the contingency table of the predicted and the true groups
// (n_gt = hunks in predicted group g and true group t), never built densely, and from it the
// hunks in the right group under the best one-to-one assignment of predicted to true groups
// (HDG_MT_MATCHED), purity, cover, the cell counts and, on request, one optimal assignment.
// The definitions are the header's.
//
// Two launches, neither waits for another block:
//   k_mt_truth  grid B, 1024 threads.  The true groups of a commit (ut_true_groups), once for
//               all sets, into the workspace ([B][nc] i32) and into tgroups when given.
//   k_mt_match  grid (n_sets, B), 256 threads, all state in LDS, three instances by the nc they
//               hold (128, 512, 2048) so that small commits share a CU.  (1) a predicted group
//               is named by its smallest member (one LDS atomicMin per hunk); (2) one walk over
//               the hunks counts for every hunk q the hunks with q's key (g, t) and those of
//               them below q: q leads its cell iff there are none, the count is the cell's
//               weight; (3) the leaders leave row and column maxima and degrees with integer
//               LDS atomics: PURITY, COVER, CELLS, ISOLATED; (4) the cells that are alone in
//               their row and column are taken as they are, the others form the residual
//               graph, on which the assignment is solved exactly by shortest augmenting paths
//               with integer potentials (Kuhn-Munkres in Jonker-Volgenant's form), rows on
//               the smaller residual side.
// A step of a path is two barriers: the current row's cells drop their weights into cw (a
// thread holds its hunks' cells in registers); every unvisited column takes its reduced cost
// from the potentials and cw alone, keeps the smaller slack and the block takes the arg-min,
// ties to the lowest column; all threads then apply the same delta.
//
// Everything named ut_ is unionfind.h's, shared with the decoders.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "unionfind.h"

namespace {

using hdg::fail;

constexpr int MT_NT = 256;
constexpr int MT_WAVES = MT_NT / 64;
constexpr int MT_INF = 1 << 30;              // above every slack: potentials stay below 2^22
constexpr uint32_t MT_NONE = 0xffffu;        // no row / the path's start, in the u16 arrays

static_assert(HDG_MT_MAX_SETS == HDG_RL_MAX_RUNGS, "a ladder's rungs are one call's sets");
static_assert(UT_MAXN <= 2048, "a cell's key holds two 11-bit ids");

// the counters of a block, in LDS
enum { MC_GROUPS, MC_TGMAX, MC_MATCHED, MC_PURITY, MC_COVER, MC_CELLS, MC_ISOLATED, MC_RES_G,
       MC_RES_T, MC_BROKEN, MC_N };

__global__ __launch_bounds__(UT_CLOSE_NT) void k_mt_truth(const uint32_t* __restrict__ ybits,
                                                          int32_t* __restrict__ ws,
                                                          int32_t* __restrict__ tgroups,
                                                          const int nc) {
  __shared__ uint32_t par[UT_MAXN];
  __shared__ uint32_t rnk[UT_MAXN];
  __shared__ uint32_t t[UT_MAXN];
  __shared__ uint32_t wsum[UT_CLOSE_WAVES];
  const int b = blockIdx.x;
  ut_true_groups(par, rnk, t, wsum, ut_label_rows(ybits, b, nc), nc);
  for (int i = threadIdx.x; i < nc; i += UT_CLOSE_NT) {
    ws[(size_t)b * nc + i] = (int32_t)t[i];
    if (tgroups) tgroups[(size_t)b * nc + i] = (int32_t)t[i];
  }
}

// NMAX: the hunks the instance holds, nc <= NMAX
template <int NMAX>
__global__ __launch_bounds__(MT_NT) void k_mt_match(const int32_t* __restrict__ groups,
                                                    const int32_t* __restrict__ truth,
                                                    int32_t* __restrict__ mate,
                                                    unsigned long long* __restrict__ mt,
                                                    const int nc) {
  constexpr int PER = NMAX / MT_NT > 0 ? NMAX / MT_NT : 1;      // hunks (columns) per thread
  __shared__ uint32_t key[NMAX];      // g << 11 | t per hunk, g the group's smallest member
  __shared__ uint32_t low[NMAX];      // smallest member per input id
  __shared__ uint32_t rmax[NMAX];     // per predicted group / true group: largest cell ...
  __shared__ uint32_t cmax[NMAX];
  __shared__ uint32_t rdeg[NMAX];     // ... and number of cells
  __shared__ uint32_t cdeg[NMAX];
  __shared__ int32_t pu[NMAX];        // potentials of the rows and of the columns
  __shared__ int32_t pv[NMAX];
  __shared__ int32_t minv[NMAX];      // slack of a column on the current path
  __shared__ uint16_t way[NMAX];      // the column before it on the path (MT_NONE: the start)
  __shared__ uint16_t pcol[NMAX];     // the row assigned to a column
  __shared__ uint16_t rowmate[NMAX];  // the column assigned to a row
  __shared__ uint16_t cw[NMAX];       // the current row's cell weights by column, else 0
  __shared__ int16_t gm[NMAX];        // predicted group -> the true group it is assigned to
  __shared__ uint8_t resg[NMAX];      // residual predicted groups / true groups
  __shared__ uint8_t rest[NMAX];
  __shared__ uint8_t used[NMAX];
  __shared__ int32_t redv[MT_WAVES];
  __shared__ int32_t redj[MT_WAVES];
  __shared__ uint32_t cnt[MC_N];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int set = blockIdx.x, b = blockIdx.y;
  const size_t base = ((size_t)set * gridDim.y + b) * (size_t)nc;
  const int32_t* gin = groups + base;
  const int32_t* tin = truth + (size_t)b * nc;

  for (int i = tid; i < nc; i += MT_NT) {
    low[i] = (uint32_t)nc;
    rmax[i] = cmax[i] = rdeg[i] = cdeg[i] = 0u;
    pu[i] = pv[i] = 0;
    pcol[i] = rowmate[i] = (uint16_t)MT_NONE;
    cw[i] = 0;
    gm[i] = -1;
    resg[i] = rest[i] = 0;
  }
  if (tid < MC_N) cnt[tid] = 0u;
  __syncthreads();

  // ---- (1) predicted groups by smallest member; an id outside [0, nc) is alone ------------
  int32_t idq[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int q = tid + u * MT_NT;
    idq[u] = q < nc ? gin[q] : -1;
    if (q < nc && idq[u] >= 0 && idq[u] < nc) atomicMin(&low[idq[u]], (uint32_t)q);
  }
  __syncthreads();
  uint32_t kq[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int q = tid + u * MT_NT;
    kq[u] = 0xffffffffu;
    if (q < nc) {
      const uint32_t g = idq[u] >= 0 && idq[u] < nc ? low[idq[u]] : (uint32_t)q;
      const uint32_t t = (uint32_t)tin[q];
      kq[u] = g << 11 | t;
      key[q] = kq[u];
      if (g == (uint32_t)q) atomicAdd(&cnt[MC_GROUPS], 1u);
      atomicMax(&cnt[MC_TGMAX], t);
    }
  }
  __syncthreads();

  // ---- (2) cells: q leads its cell iff no p < q has its key; the weight counts the key ----
  uint32_t wq[PER], below[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) wq[u] = below[u] = 0u;
  for (int p = 0; p < nc; ++p) {
    const uint32_t kp = key[p];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const uint32_t e = kq[u] == kp;
      wq[u] += e;
      below[u] += e & (uint32_t)(p < tid + u * MT_NT);
    }
  }

  // ---- (3) row and column maxima and degrees ----------------------------------------------
  bool lead[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int q = tid + u * MT_NT;
    lead[u] = q < nc && below[u] == 0u;
    if (lead[u]) {
      const uint32_t g = kq[u] >> 11, t = kq[u] & 2047u;
      atomicMax(&rmax[g], wq[u]);
      atomicMax(&cmax[t], wq[u]);
      atomicAdd(&rdeg[g], 1u);
      atomicAdd(&cdeg[t], 1u);
      atomicAdd(&cnt[MC_CELLS], 1u);
    }
  }
  __syncthreads();
  // the isolated cells are in every optimum; the others are the residual graph
  bool res[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int q = tid + u * MT_NT;
    res[u] = false;
    if (q < nc) {
      atomicAdd(&cnt[MC_PURITY], rmax[q]);
      atomicAdd(&cnt[MC_COVER], cmax[q]);
    }
    if (lead[u]) {
      const uint32_t g = kq[u] >> 11, t = kq[u] & 2047u;
      if (rdeg[g] == 1u && cdeg[t] == 1u) {
        atomicAdd(&cnt[MC_ISOLATED], 1u);
        atomicAdd(&cnt[MC_MATCHED], wq[u]);
        gm[g] = (int16_t)t;
      } else {                      // every writer of a flag writes 1
        res[u] = true;
        resg[g] = 1;
        rest[t] = 1;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < nc; i += MT_NT) {
    if (resg[i]) atomicAdd(&cnt[MC_RES_G], 1u);
    if (rest[i]) atomicAdd(&cnt[MC_RES_T], 1u);
  }
  __syncthreads();

  // ---- (4) the assignment on the residual graph, rows on its smaller side -------------------
  const uint32_t kg = cnt[MC_RES_G], kt = cnt[MC_RES_T];
  if (kg > 0u) {
    const bool sw = kt < kg;                       // rows are the true groups
    const uint8_t* rmask = sw ? rest : resg;
    const uint8_t* cmask = sw ? resg : rest;
    int rowq[PER], colq[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int g = (int)(kq[u] >> 11), t = (int)(kq[u] & 2047u);
      rowq[u] = res[u] ? (sw ? t : g) : -1;
      colq[u] = sw ? g : t;
    }
    for (int i = 0; i < nc; ++i) {                 // at most K' = min(kg, kt) rows pass
      if (!rmask[i]) continue;
      for (int c = tid; c < nc; c += MT_NT) {
        minv[c] = MT_INF;
        used[c] = !cmask[c];
      }
      int i0 = i;
      uint32_t j0 = MT_NONE;
      bool found = false;
      __syncthreads();
      for (int step = 0; step <= nc; ++step) {     // at most K' + 1 columns join a path
#pragma unroll
        for (int u = 0; u < PER; ++u)
          if (rowq[u] == i0) cw[colq[u]] = (uint16_t)wq[u];
        __syncthreads();
        const int ui = pu[i0];
        int bv = INT32_MAX, bj = INT32_MAX;
        for (int c = tid; c < nc; c += MT_NT) {
          if (!used[c]) {
            const int cur = -(int)cw[c] - ui - pv[c];
            int m = minv[c];
            if (cur < m) {
              m = cur;
              minv[c] = m;
              way[c] = (uint16_t)j0;
            }
            if (m < bv) {
              bv = m;
              bj = c;
            }
          }
          cw[c] = 0;
        }
        // the block's smallest slack, ties to the lowest column
        int wv = bv;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const int x = __shfl_xor(wv, o, 64);
          wv = x < wv ? x : wv;
        }
        int wj = bv == wv ? bj : INT32_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const int x = __shfl_xor(wj, o, 64);
          wj = x < wj ? x : wj;
        }
        if (lane == 0) {
          redv[wave] = wv;
          redj[wave] = wj;
        }
        __syncthreads();
        int delta = redv[0], j1 = redj[0];
#pragma unroll
        for (int w = 1; w < MT_WAVES; ++w) {
          const int v = redv[w], j = redj[w];
          if (v < delta || (v == delta && j < j1)) {
            delta = v;
            j1 = j;
          }
        }
        if (j1 >= nc) {                            // no column left: cannot happen, rows <= columns;
          if (tid == 0) cnt[MC_BROKEN] = 1u;       // if it ever did, slot 7 of the row says so
          break;
        }
        for (int c = tid; c < nc; c += MT_NT) {
          if (used[c]) {
            if (cmask[c] && pcol[c] != MT_NONE) {  // on the path: assigned, to distinct rows
              pu[pcol[c]] += delta;
              pv[c] -= delta;
            }
          } else {
            minv[c] -= delta;
            if (c == j1) used[c] = 1;
          }
        }
        if (tid == 0) pu[i] += delta;              // the row of the path's start
        j0 = (uint32_t)j1;
        const uint32_t r = pcol[j1];
        if (r == MT_NONE) {
          found = true;
          break;
        }
        i0 = (int)r;
      }
      __syncthreads();
      if (tid == 0 && found) {                     // augment: at most K' + 1 columns
        uint32_t j = j0;
        for (int step = 0; step <= nc && j != MT_NONE; ++step) {
          const uint32_t jp = way[j];
          pcol[j] = jp == MT_NONE ? (uint16_t)i : pcol[jp];
          j = jp;
        }
      }
      __syncthreads();
    }
    for (int c = tid; c < nc; c += MT_NT)
      if (cmask[c] && pcol[c] != MT_NONE) rowmate[pcol[c]] = (uint16_t)c;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (rowq[u] >= 0 && rowmate[rowq[u]] == (uint32_t)colq[u]) {
        atomicAdd(&cnt[MC_MATCHED], wq[u]);
        gm[kq[u] >> 11] = (int16_t)(kq[u] & 2047u);
      }
    }
    __syncthreads();
  }

  // ---- outputs ---------------------------------------------------------------------------------
  if (mate) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int q = tid + u * MT_NT;
      if (q < nc) mate[base + q] = (int32_t)gm[kq[u] >> 11];
    }
  }
  if (tid == 0) {
    unsigned long long* row = mt + ((size_t)set * gridDim.y + b) * HDG_MT_SLOTS;
    row[HDG_MT_GROUPS] = cnt[MC_GROUPS];
    row[HDG_MT_TGROUPS] = cnt[MC_TGMAX] + 1u;
    row[HDG_MT_MATCHED] = cnt[MC_MATCHED];
    row[HDG_MT_PURITY] = cnt[MC_PURITY];
    row[HDG_MT_COVER] = cnt[MC_COVER];
    row[HDG_MT_CELLS] = cnt[MC_CELLS];
    row[HDG_MT_ISOLATED] = cnt[MC_ISOLATED];
    row[7] = cnt[MC_BROKEN];                       // 0: every path found its column
  }
}

inline int mt_check_sets(const int32_t n_sets, const char* who) {
  if (n_sets < 1 || n_sets > HDG_MT_MAX_SETS)
    return fail(HDG_EINVAL, "%s: n_sets must be in [1, %d] (got %d)", who, HDG_MT_MAX_SETS,
                (int)n_sets);
  return 0;
}

}  // namespace

extern "C" size_t hdg_match_workspace_bytes(const hdg_shape* s, int32_t n_sets) {
  if (ut_check_shape(s, "hdg_match_workspace_bytes")) return 0;
  if (mt_check_sets(n_sets, "hdg_match_workspace_bytes")) return 0;
  // the true ids, once for all sets; whole 8-byte words
  return (((size_t)s->batch * (size_t)s->nc * sizeof(int32_t)) + 7u) & ~(size_t)7u;
}

extern "C" int hdg_match(const hdg_shape* s, const hdg_batch* bt, const int32_t* groups,
                         int32_t n_sets, int32_t* mate, int32_t* tgroups, uint64_t* mt,
                         void* workspace, void* stream) {
  if (const int rc = ut_check_shape(s, "hdg_match")) return rc;
  if (const int rc = mt_check_sets(n_sets, "hdg_match")) return rc;
  if (!bt || !bt->ybits || !groups || !mt || !workspace)
    return fail(HDG_EINVAL, "hdg_match: NULL pointer (batch, batch->ybits, groups, mt or "
                            "workspace)");
  if (const int rc = ut_check_workspace(workspace, "hdg_match")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nc = s->nc;
  hipLaunchKernelGGL(k_mt_truth, dim3((unsigned)s->batch), dim3(UT_CLOSE_NT), 0, st, bt->ybits,
                     (int32_t*)workspace, tgroups, nc);
  if (const int rc = ut_launched("hdg_match", "truth")) return rc;
  const dim3 grid((unsigned)n_sets, (unsigned)s->batch);
  unsigned long long* row = (unsigned long long*)mt;
  const int32_t* truth = (const int32_t*)workspace;
  if (nc <= 128)
    hipLaunchKernelGGL(k_mt_match<128>, grid, dim3(MT_NT), 0, st, groups, truth, mate, row, nc);
  else if (nc <= 512)
    hipLaunchKernelGGL(k_mt_match<512>, grid, dim3(MT_NT), 0, st, groups, truth, mate, row, nc);
  else
    hipLaunchKernelGGL(k_mt_match<2048>, grid, dim3(MT_NT), 0, st, groups, truth, mate, row, nc);
  return ut_launched("hdg_match", "match");
}
