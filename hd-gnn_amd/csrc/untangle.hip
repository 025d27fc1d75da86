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
//               blk takes the tile pairs k = blk, blk + nblk, ... (row-major over I <= J).
//               Per tile pair it stages the I x J segment of s and its mirror J x I segment
//               in LDS (row-coalesced loads; the [q > p] shift of r(p, q) moves inside a row
//               where the tile crosses the diagonal), visits every p < q of the tile once
//               (s_pq by row from one tile, s_qp transposed from the other: rows are 65
//               words apart, so the 32 lanes of a half-wave hit 32 banks both ways), applies
//               the rule and unites linked pairs in a block-local union-find forest in LDS.
//               The flattened forest and the block's LINKS / NAN counts go to the workspace.
//   k_ut_close  grid B, 1024 threads.  Unites every node with its root in every block
//               forest of the commit (the roots are the blocks' partial components' minima,
//               so this merges them exactly), labels the components, does the same for the
//               label graph from the set bits of ybits, counts the pairs of the two
//               labelings and writes groups, tgroups and the ut row.
//
// The union-find (lock-free, min-root hooking), the labelling and the tile geometry are
// unionfind.h's, shared with linkage.hip.
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
                                                        const float thr, const float thr2) {
  __shared__ float sa[UT_T * UT_LD];       // sa[a][c] = s(64 I + a, 64 J + c)
  __shared__ float sb[UT_T * UT_LD];       // sb[c][a] = s(64 J + c, 64 I + a)
  __shared__ uint32_t parent[UT_MAXN];
  __shared__ uint32_t red[UT_LINK_WAVES][2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, b = blockIdx.y;
  const int n1 = nc - 1;
  const size_t ncr = (size_t)nc * n1;
  const float* s = probs + (size_t)b * 2 * ncr + ncr;     // channel 1
  const int T = (nc + UT_T - 1) / UT_T, tiles = T * (T + 1) / 2;

  for (int i = tid; i < nc; i += UT_LINK_NT) parent[i] = (uint32_t)i;

  uint32_t links = 0, nans = 0;
  for (int k = blk; k < tiles; k += nblk) {
    int I = 0, rem = k;                    // tile pair k, row-major over I <= J
    while (rem >= T - I) {
      rem -= T - I;
      ++I;
    }
    const int p0 = I * UT_T, q0 = (I + rem) * UT_T;
    __syncthreads();                       // parent initialised; the last visit is over
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
    __syncthreads();
    for (int idx = tid; idx < UT_T * UT_T; idx += UT_LINK_NT) {
      const int a = idx >> 6, c = idx & 63;
      const int p = p0 + a, q = q0 + c;
      if (p < q && q < nc) {
        const float spq = sa[a * UT_LD + c], sqp = sb[c * UT_LD + a];
        if (spq != spq || sqp != sqp) {
          ++nans;
        } else {
          bool link;
          if (rule == HDG_UT_RULE_MEAN) link = spq + sqp > thr2;
          else if (rule == HDG_UT_RULE_ANY) link = spq > thr || sqp > thr;
          else link = spq > thr && sqp > thr;
          if (link) {
            ++links;
            ut_union(parent, (uint32_t)p, (uint32_t)q);
          }
        }
      }
    }
  }
  __syncthreads();

  uint32_t* wb = ws + (size_t)b * ut_commit_words(nc, nblk);
  uint32_t* forest = wb + (size_t)blk * nc;
  for (int i = tid; i < nc; i += UT_LINK_NT) forest[i] = ut_find(parent, (uint32_t)i);
  links = ut_wave_sum(links);
  nans = ut_wave_sum(nans);
  if (lane == 0) {
    red[wave][0] = links;
    red[wave][1] = nans;
  }
  __syncthreads();
  if (tid < 2) {
    uint32_t v = 0;
    for (int w = 0; w < UT_LINK_WAVES; ++w) v += red[w][tid];
    wb[(size_t)nblk * nc + 2 * blk + tid] = v;
  }
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
  __shared__ uint32_t red[UT_CLOSE_WAVES][3];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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

  // ---- true groups: the set bits of the commit's label rows ------------------------------
  for (int i = tid; i < nc; i += UT_CLOSE_NT) par[i] = (uint32_t)i;
  __syncthreads();
  ut_unite_labels(par, ybits + (size_t)b * nc * ((nc + 31) >> 5), nc);
  __syncthreads();
  const uint32_t TG = ut_label(par, rnk, t, wsum, nc);

  // ---- pair counts: this thread's q against every p < q -----------------------------------
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
  same_p = ut_wave_sum(same_p);
  same_t = ut_wave_sum(same_t);
  ss = ut_wave_sum(ss);
  if (lane == 0) {
    red[wave][0] = same_p;
    red[wave][1] = same_t;
    red[wave][2] = ss;
  }

  // ---- outputs ------------------------------------------------------------------------------
  for (int i = tid; i < nc; i += UT_CLOSE_NT) {
    groups[(size_t)b * nc + i] = (int32_t)g[i];
    if (tgroups) tgroups[(size_t)b * nc + i] = (int32_t)t[i];
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long sp = 0, st = 0, s2 = 0, links = 0, nans = 0;
    for (int w = 0; w < UT_CLOSE_WAVES; ++w) {
      sp += red[w][0];
      st += red[w][1];
      s2 += red[w][2];
    }
    const uint32_t* cnt = wb + (size_t)nblk * nc;
    for (int f = 0; f < nblk; ++f) {
      links += cnt[2 * f];
      nans += cnt[2 * f + 1];
    }
    const unsigned long long all = (unsigned long long)nc * (unsigned long long)(nc - 1) / 2ull;
    unsigned long long* row = ut + (size_t)b * HDG_UT_SLOTS;
    row[HDG_UT_GROUPS] = G;
    row[HDG_UT_TGROUPS] = TG;
    row[HDG_UT_SS] = s2;
    row[HDG_UT_SD] = sp - s2;
    row[HDG_UT_DS] = st - s2;
    row[HDG_UT_DD] = all - sp - st + s2;
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
  if (rule != HDG_UT_RULE_MEAN && rule != HDG_UT_RULE_ANY && rule != HDG_UT_RULE_BOTH)
    return fail(HDG_EINVAL, "hdg_untangle: unknown rule %d (HDG_UT_RULE_MEAN / _ANY / _BOTH)",
                (int)rule);
  if (threshold != threshold) return fail(HDG_EINVAL, "hdg_untangle: threshold is NaN");
  if (!bt || !bt->ybits || !probs || !groups || !ut || !workspace)
    return fail(HDG_EINVAL, "hdg_untangle: NULL pointer (batch, batch->ybits, probs, groups, "
                            "ut or workspace)");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ut_blocks(s->nc);
  volatile float two = threshold;          // fl32(threshold + threshold), once
  const float thr2 = two + two;
  hipLaunchKernelGGL(k_ut_link, dim3((unsigned)nblk, (unsigned)s->batch), dim3(UT_LINK_NT), 0, st,
                     probs, (uint32_t*)workspace, s->nc, nblk, (int)rule, threshold, thr2);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "hdg_untangle: launch (link): %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_ut_close, dim3((unsigned)s->batch), dim3(UT_CLOSE_NT), 0, st,
                     (const uint32_t*)workspace, bt->ybits, groups, tgroups,
                     (unsigned long long*)ut, s->nc, nblk);
  e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "hdg_untangle: launch (close): %s", hipGetErrorString(e));
  return 0;
}
