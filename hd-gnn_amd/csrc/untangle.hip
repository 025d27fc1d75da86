// untangle.hip -- on-device untangling of a commit's hunks (hdg_untangle, include/hdgnn.h).
//
// From the probabilities a forward or training launch left on the device ([B][2][Ncr]) and
// the batch's label bits, per commit: the predicted groups (connected components of the
// link graph the rule and threshold cut out of the pair scores), the true groups (connected
// components of the label graph), both as dense ids ordered by smallest member, and the
// pair-counting table of the two partitions (HDG_UT_*).  The definitions are the header's.
//
// Two launches, neither waits for another block:
//   k_ut_link   grid (nblk, B), 512 threads.  The hunk grid is cut into 64 x 64 tiles; block
//               blk takes the tile pairs k = blk, blk + nblk, ... (ut_tile_pair).  Per tile
//               pair it stages the I x J segment of s and its mirror in LDS (ut_stage),
//               visits every p < q of the tile once (ut_visit: s_pq by row from one tile,
//               s_qp transposed from the other), links the pairs whose weight (ut_weight) is
//               above the bound t' and unites them in a block-local union-find forest in LDS.
//               The flattened forest and the block's LINKS / NAN counts go to the workspace.
//   k_ut_close  grid B, 1024 threads.  Unites every node with its root in every block
//               forest of the commit (the roots are the blocks' partial components' minima,
//               so this merges them exactly), labels the components (ut_label), labels the
//               label graph (ut_true_groups), counts the pairs of the two labelings
//               (ut_pair_counts, ut_pair_table) and writes groups, tgroups and the ut row.
//
// Everything named ut_ is unionfind.h's, shared with linkage.hip, agglo.hip and refine.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn_internal.h"
#include "unionfind.h"

namespace {

using hdg::fail;

// workspace, in 4-byte words per commit: nblk forests of nc words, then nblk {LINKS, NAN}
__host__ __device__ inline size_t ut_commit_words(const int nc, const int nblk) {
  return (size_t)nblk * (size_t)(nc + 2);
}

__global__ __launch_bounds__(UT_LINK_NT) void k_ut_link(const float* __restrict__ probs,
                                                        uint32_t* __restrict__ ws, const int nc,
                                                        const int nblk, const int rule,
                                                        const float tp) {
  __shared__ float sa[UT_T * UT_LD];       // sa[a][c] = s(64 I + a, 64 J + c)
  __shared__ float sb[UT_T * UT_LD];       // sb[c][a] = s(64 J + c, 64 I + a)
  __shared__ uint32_t parent[UT_MAXN];
  __shared__ uint32_t red[UT_LINK_WAVES * 2];

  const int tid = threadIdx.x;
  const int blk = blockIdx.x, b = blockIdx.y;
  const float* s = ut_scores(probs, b, nc);
  const int tiles = ut_tiles(nc);

  for (int i = tid; i < nc; i += UT_LINK_NT) parent[i] = (uint32_t)i;

  uint32_t links = 0, nans = 0;
  for (int k = blk; k < tiles; k += nblk) {
    int p0, q0;
    ut_tile_pair(k, nc, p0, q0);
    __syncthreads();                       // parent initialised; the last visit is over
    ut_stage(s, nc, p0, q0, sa, sb);
    __syncthreads();
    ut_visit(nc, p0, q0, sa, sb,
             [&](int, int, int, const int p, const int q, const float spq, const float sqp) {
               float w;                    // NaN for +inf and -inf under MEAN: no link, and
               ut_weight(rule, spq, sqp, w);     // not a NaN score either
               if (spq != spq || sqp != sqp) {
                 ++nans;
               } else if (w > tp) {
                 ++links;
                 ut_union(parent, (uint32_t)p, (uint32_t)q);
               }
             });
  }
  __syncthreads();

  uint32_t* wb = ws + (size_t)b * ut_commit_words(nc, nblk);
  uint32_t* forest = wb + (size_t)blk * nc;
  for (int i = tid; i < nc; i += UT_LINK_NT) forest[i] = ut_find(parent, (uint32_t)i);
  ut_count_put(red, links, nans);
  __syncthreads();
  if (tid < 2)
    wb[(size_t)nblk * nc + 2 * blk + tid] = ut_count_sum<uint32_t, UT_LINK_WAVES, 2>(red, tid);
}

__global__ __launch_bounds__(UT_CLOSE_NT) void k_ut_close(const uint32_t* __restrict__ ws,
                                                          const uint32_t* __restrict__ ybits,
                                                          int32_t* __restrict__ groups,
                                                          int32_t* __restrict__ tgroups,
                                                          unsigned long long* __restrict__ ut,
                                                          const int nc, const int nblk) {
  __shared__ uint32_t par[UT_MAXN];
  __shared__ uint32_t rnk[UT_MAXN];
  __shared__ uint32_t g[UT_MAXN];
  __shared__ uint32_t t[UT_MAXN];
  __shared__ uint32_t wsum[UT_CLOSE_WAVES];
  __shared__ uint32_t red[UT_CLOSE_WAVES * 3];

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const uint32_t* wb = ws + (size_t)b * ut_commit_words(nc, nblk);

  // ---- predicted groups: the blocks' forests merged ------------------------------------
  for (int i = tid; i < nc; i += UT_CLOSE_NT) par[i] = (uint32_t)i;
  __syncthreads();
  for (int f = 0; f < nblk; ++f) {
    const uint32_t* forest = wb + (size_t)f * nc;
    for (int i = tid; i < nc; i += UT_CLOSE_NT) {
      const uint32_t r = forest[i];
      if (r < (uint32_t)i) ut_union(par, (uint32_t)i, r);
    }
  }
  __syncthreads();
  const uint32_t G = ut_label(par, rnk, g, wsum, nc);
  const uint32_t TG = ut_true_groups(par, rnk, t, wsum, ut_label_rows(ybits, b, nc), nc);
  ut_pair_counts(g, t, red, nc);

  // ---- outputs ------------------------------------------------------------------------------
  for (int i = tid; i < nc; i += UT_CLOSE_NT) {
    groups[(size_t)b * nc + i] = (int32_t)g[i];
    if (tgroups) tgroups[(size_t)b * nc + i] = (int32_t)t[i];
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long links = 0, nans = 0;
    const uint32_t* cnt = wb + (size_t)nblk * nc;
    for (int f = 0; f < nblk; ++f) {
      links += cnt[2 * f];
      nans += cnt[2 * f + 1];
    }
    unsigned long long* row = ut + (size_t)b * HDG_UT_SLOTS;
    ut_pair_table(red, G, TG, nc, row);
    row[HDG_UT_LINKS] = links;
    row[HDG_UT_NAN] = nans;
  }
}

}  // namespace

extern "C" size_t hdg_untangle_workspace_bytes(const hdg_shape* s) {
  if (ut_check_shape(s, "hdg_untangle_workspace_bytes")) return 0;
  return (size_t)s->batch * ut_commit_words(s->nc, ut_blocks(s->nc)) * sizeof(uint32_t);
}

extern "C" int hdg_untangle(const hdg_shape* s, const hdg_batch* bt, const float* probs,
                            float threshold, int32_t rule, int32_t* groups, int32_t* tgroups,
                            uint64_t* ut, void* workspace, void* stream) {
  if (const int rc = ut_check_shape(s, "hdg_untangle")) return rc;
  if (const int rc = ut_check_rule(rule, "hdg_untangle")) return rc;
  if (threshold != threshold) return fail(HDG_EINVAL, "hdg_untangle: threshold is NaN");
  if (!bt || !bt->ybits || !probs || !groups || !ut || !workspace)
    return fail(HDG_EINVAL, "hdg_untangle: NULL pointer (batch, batch->ybits, probs, groups, "
                            "ut or workspace)");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ut_blocks(s->nc);
  hipLaunchKernelGGL(k_ut_link, dim3((unsigned)nblk, (unsigned)s->batch), dim3(UT_LINK_NT), 0, st,
                     probs, (uint32_t*)workspace, s->nc, nblk, (int)rule,
                     ut_link_bound(rule, threshold));
  if (const int rc = ut_launched("hdg_untangle", "link")) return rc;
  hipLaunchKernelGGL(k_ut_close, dim3((unsigned)s->batch), dim3(UT_CLOSE_NT), 0, st,
                     (const uint32_t*)workspace, bt->ybits, groups, tgroups,
                     (unsigned long long*)ut, s->nc, nblk);
  return ut_launched("hdg_untangle", "close");
}
