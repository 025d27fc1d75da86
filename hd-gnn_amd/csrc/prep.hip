// prep.hip -- batch preparation (hdg_prepare, hdg_pack_classes; include/hdgnn.h): the
// parameter-independent tables of an uploaded batch, built once per batch.
//
//   k_prep_sort     fused layout only: x sort order, distinct values + f64 prefix sums,
//                   CSR offsets and neighbour lists (PrepLayout, hdgnn_internal.h)
//   k_prep_counts   the cross-graph count matrices ks / kt and the class counts ncst, at
//   k_prep_ncst     the offsets either path's layout gives them (launch_prep_maps)
//   k_pack_classes  upload-time marshalling of a u8 class grid into label bits
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdgnn.h"
#include "hdgnn_internal.h"

namespace {

using namespace hdg;

// sort x (stable rank count), distinct values + f64 prefix sums, transposed class bits
__global__ __launch_bounds__(256) void k_prep_sort(const float* __restrict__ x,
                                                   const uint32_t* __restrict__ abits,
                                                   uint32_t* __restrict__ prep, int Ne, int Nc) {
  const PrepLayout L = prep_layout(Ne, Nc);
  const int b = blockIdx.x, t = threadIdx.x;
  const int WE = (Ne + 31) >> 5;
  __shared__ float xl[256], xsl[256];
  __shared__ uint32_t al[256 * 8];
  uint32_t* pb = prep + (size_t)b * L.words;
  float* xsrt = (float*)(pb + L.xsrt);
  int* perm = (int*)(pb + L.perm);
  float* xu = (float*)(pb + L.xu);
  int* cum = (int*)(pb + L.cum);
  double* pxd = (double*)(pb + L.pxd);
  if (t < Ne) xl[t] = x[(size_t)b * Ne + t];
  for (int w = t; w < Ne * WE; w += 256) al[w] = abits[(size_t)b * Ne * WE + w];
  __syncthreads();
  if (t < Ne) al[t * WE + (t >> 5)] &= ~(1u << (t & 31));      // a_ii is not a relation
  __syncthreads();
  if (t < Ne) {
    const float xi = xl[t];
    int r = 0;
    for (int j = 0; j < Ne; ++j) {
      const float xj = xl[j];
      r += (xj < xi || (xj == xi && j < t)) ? 1 : 0;
    }
    xsl[r] = xi;
    xsrt[r] = xi;
    perm[r] = t;
  }
  __shared__ uint32_t atl[256 * 8];
  __shared__ int offl[2][260];
  for (int e = t; e < Ne * WE; e += 256) {          // a^T bits
    const int j = e / WE, w = e - j * WE;
    uint32_t bits = 0;
    for (int l = 0; l < 32; ++l) {
      const int i = 32 * w + l;
      if (i < Ne) bits |= ((al[i * WE + (j >> 5)] >> (j & 31)) & 1u) << l;
    }
    atl[e] = bits;
  }
  __syncthreads();
  __shared__ int xof[2][260];
  if (t < Ne) {
    int dr = 0, dc = 0;
    for (int w = 0; w < WE; ++w) {
      dr += __builtin_popcount(al[t * WE + w]);
      dc += __builtin_popcount(atl[t * WE + w]);
    }
    offl[0][t] = dr;
    offl[1][t] = dc;
    xof[0][t] = (dr + 3) & ~3;
    xof[1][t] = (dc + 3) & ~3;
  }
  __syncthreads();
  if (t == 0) {            // serial scans of the padded x-list lengths, rows then columns
    int acc = 0;
    for (int s2 = 0; s2 < 2; ++s2) {
      int* dst = (int*)(pb + (s2 ? L.xoffc : L.xoffr));
      for (int i = 0; i < Ne; ++i) {
        const int d = xof[s2][i];
        xof[s2][i] = acc;
        dst[i] = acc;
        acc += d;
      }
      xof[s2][Ne] = acc;
      dst[Ne] = acc;
    }
  }
  if (t < 2) {                                       // serial exclusive scans, once per batch
    int acc = 0;
    for (int i = 0; i < Ne; ++i) {
      const int d = offl[t][i];
      offl[t][i] = acc;
      ((int*)(pb + (t ? L.offc : L.offr)))[i] = acc;
      acc += d;
    }
    offl[t][Ne] = acc;
    ((int*)(pb + (t ? L.offc : L.offr)))[Ne] = acc;
  }
  __syncthreads();
  const int cbase = (offl[0][Ne] + 3) & ~3;
  if (t == 0) {
    pb[L.meta + 1] = (uint32_t)offl[0][Ne];
    pb[L.meta + 2] = (uint32_t)offl[1][Ne];
    pb[L.meta + 3] = (uint32_t)cbase;
  }
  if (t < Ne) {
    uint8_t* lb = reinterpret_cast<uint8_t*>(pb + L.lists);
    float* xlp = reinterpret_cast<float*>(pb + L.xl);
    int xr = xof[0][t], xc = xof[1][t];
    for (int w = 0; w < WE; ++w) {
      uint32_t m = al[t * WE + w];
      while (m) {
        const int j = 32 * w + __builtin_ctz(m);
        lb[xr] = (uint8_t)j;
        xlp[xr++] = xl[j];
        m &= m - 1u;
      }
      m = atl[t * WE + w];
      while (m) {
        xlp[xc++] = xl[32 * w + __builtin_ctz(m)];
        m &= m - 1u;
      }
    }
    const float qnan = __builtin_nanf("");      // clamp_fma2(NaN) = 0: pads add nothing
    for (; xr < xof[0][t + 1]; ++xr) { xlp[xr] = qnan; lb[xr] = 0; }
    for (; xc < xof[1][t + 1]; ++xc) xlp[xc] = qnan;
  }
  __syncthreads();
  if (t == 0) {   // serial over <= 256 sorted values, once per batch
    int nd = 0;
    double s = 0.0;
    for (int m = 0; m < Ne; ++m) {
      const float v = xsl[m];
      if (m == 0 || v != xsl[m - 1]) {
        xu[nd] = v;
        cum[nd] = m;
        pxd[nd] = s;
        ++nd;
      }
      s += (double)v;
    }
    cum[nd] = Ne;
    pxd[nd] = s;
    pb[L.meta] = (uint32_t)nd;
  }
}

// Cross-graph aggregation counts.  marshalling_B2 (model_2.py:146-150, dense maps of
// utils2.py:111-137) is n_c = sum_r ([s_r = c] + [t_r = c]) B2_r with
// B2_r = [x'_I, x'_J, [a_IJ = 0], [a_IJ = 1]], (I, J) = relation r on the Ne-grid and
// s_r = hid[i'], t_r = hid[j'] with (i', j') = relation r on the n-grid (r < n(n-1)).
// Only x' changes between steps, so
//   n_c[0] = sum_I ks[c][I] x'_I,  n_c[1] = sum_J kt[c][J] x'_J,  n_c[2:4] = ncst[c]
// ks[c][I] = #{r in Ne-row I : s_r = c} + #{r in Ne-row I : t_r = c}, kt over Ne-columns.
//
// k_prep_counts grid (ceil(Ne / TI), B, 2): block (tile, b, z) owns TI Ne-rows (z = 0: ks,
// plus the class counts) or TI Ne-columns (z = 1: kt) of commit b and visits each of their
// relations once, counting into an LDS histogram [Nc][TI] (integer, order-independent).
// Lanes hold consecutive relations of a row (or column), whose hunk ids repeat in runs
// (s_r is constant over n-1 consecutive relations): each run of equal counter addresses in
// consecutive lanes is one LDS atomic by its first lane (ballot masks), not a same-address
// conflict per lane.  The tile's counters are written as coalesced u16 rows; the class
// counts are summed over tiles with global u32 atomics into ncst (zeroed, then converted to
// f32 in place by k_prep_ncst).  The count arrays live at word offsets (o_ks, o_kt, o_ncst)
// of each commit's prep block of `stride` words (fused layout: prep_layout; general path:
// its own layout).
// ------------------------------------------------------------------------------
__device__ __forceinline__ void divmod_exact(int r, int d, float inv, int& q, int& rem) {
  q = (int)((float)r * inv);
  rem = r - q * d;
  while (rem < 0) { --q; rem += d; }
  while (rem >= d) { ++q; rem -= d; }
}

// counter[key] += (number of consecutive valid lanes from this lane with the same key),
// issued by the first lane of each run; invalid lanes end runs.  All 64 lanes take part.
__device__ __forceinline__ void run_add(uint32_t* counter, int key, bool valid, int lane) {
  const int kp = __shfl_up(key, 1, 64);
  const unsigned long long V = __ballot(valid);
  const bool pv = lane > 0 && ((V >> (lane - 1)) & 1ull);   // previous lane in a run
  const bool lead = valid && (!pv || kp != key);
  const unsigned long long L = __ballot(lead);
  if (lead) {
    const unsigned long long stop =
        (L | ~V) & (lane == 63 ? 0ull : (~0ull << (lane + 1)));
    const int nxt = stop ? __builtin_ctzll(stop) : 64;
    atomicAdd(&counter[key], (uint32_t)(nxt - lane));
  }
}

__global__ __launch_bounds__(512) void k_prep_counts(const uint32_t* __restrict__ abits,
                                                     const int32_t* __restrict__ hidg,
                                                     const int32_t* __restrict__ nleng,
                                                     uint32_t* __restrict__ prep, int Ne, int Nc,
                                                     int TI, int stride, int o_ks, int o_kt,
                                                     int o_ncst) {
  extern __shared__ uint32_t hist[];   // [Nc][TI + 1] | class counts [Nc][2] | hid [Ne] |
                                       // the tile's a-rows [TI][WE] (z = 0)
  const int z = blockIdx.z, b = blockIdx.y, L0 = blockIdx.x * TI, t = threadIdx.x;
  const int lane = t & 63;
  const int WE = (Ne + 31) >> 5;
  uint32_t* pb = prep + (size_t)b * stride;
  const int TP = TI + 1;               // odd row stride: the hunks of one row / column of the
                                       // tile fall in different LDS banks
  uint32_t* ncl = hist + Nc * TP;
  int32_t* hid = reinterpret_cast<int32_t*>(ncl + 2 * Nc);   // LDS copies: the per-relation
  uint32_t* ab = ncl + 2 * Nc + Ne;                          // lookups stay on-chip
  int n = nleng[b];
  n = n < 0 ? 0 : (n > Ne ? Ne : n);
  const int nrel = n >= 2 ? n * (n - 1) : 0;
  const int n1 = n >= 2 ? n - 1 : 1, Ne1 = Ne - 1;
  const float invn = 1.f / (float)n1, invE = 1.f / (float)(Ne1 > 0 ? Ne1 : 1);
  const int nl = Ne - L0 < TI ? Ne - L0 : TI;
  for (int e = t; e < Ne; e += 512) hid[e] = hidg[(size_t)b * Ne + e];
  if (z == 0)
    for (int e = t; e < nl * WE; e += 512) ab[e] = abits[((size_t)b * Ne + L0) * WE + e];
  for (int e = t; e < Nc * TP + 2 * Nc; e += 512) hist[e] = 0;
  __syncthreads();
  const int items = nl * Ne1;
  for (int e0 = 0; e0 < items; e0 += 512) {   // block-uniform trips: every lane takes part
    const int e = e0 + t;
    int li = 0, k = 0, I = 0, jj = 0, J = 0;
    if (e < items) divmod_exact(e, Ne1, invE, li, k);
    if (z == 0) { I = L0 + li; jj = k; J = jj + (jj >= I ? 1 : 0); }
    else { J = L0 + li; I = k + (k >= J ? 1 : 0); jj = J - (J > I ? 1 : 0); }
    const int r = I * Ne1 + jj;
    const bool in = e < items && r < nrel;
    int hs = -1, ht = -1, a = 0;
    if (in) {
      int ip, jjp;
      divmod_exact(r, n1, invn, ip, jjp);
      const int jp = jjp + (jjp >= ip ? 1 : 0);
      hs = hid[ip];
      ht = hid[jp];
      if (z == 0) a = (int)((ab[li * WE + (J >> 5)] >> (J & 31)) & 1u);
    }
    const bool vs = hs >= 0 && hs < Nc, vt = ht >= 0 && ht < Nc;
    run_add(hist, vs ? hs * TP + li : 0, vs, lane);
    run_add(hist, vt ? ht * TP + li : 0, vt, lane);
    if (z == 0) {
      run_add(ncl, vs ? 2 * hs + a : 0, vs, lane);
      run_add(ncl, vt ? 2 * ht + a : 0, vt, lane);
    }
  }
  __syncthreads();
  uint16_t* out = (uint16_t*)(pb + (z ? o_kt : o_ks));
  for (int e = t; e < Nc * TI; e += 512) {
    const int c = e / TI, i = e - c * TI;
    if (i < nl) out[(size_t)c * Ne + L0 + i] = (uint16_t)hist[c * TP + i];
  }
  if (z == 0) {
    uint32_t* nc = pb + o_ncst;
    for (int e = t; e < 2 * Nc; e += 512)
      if (ncl[e]) atomicAdd(&nc[e], ncl[e]);
  }
}

// Upload-time marshalling (hdg_pack_classes): (B, N, N) u8 class grid -> (B, N, ceil(N/32))
// u32 rows, bit j of row i = (class(i, j) == 1), diagonal cleared -- the E_edge / C_edge
// one-hots of utils2.py:82, 105 as hdg_batch's abits / ybits.  One thread per word.
__global__ __launch_bounds__(256) void k_pack_classes(const uint8_t* __restrict__ cls, const int N,
                                                      const int W, const long long words,
                                                      uint32_t* __restrict__ bits) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= words) return;
  const long long row = w / W;
  const int wi = (int)(w - row * W), i = (int)(row % N), j0 = 32 * wi;
  const uint8_t* src = cls + row * N + j0;
  const int n = N - j0 < 32 ? N - j0 : 32;
  uint32_t b = 0u;
  for (int l = 0; l < n; ++l) b |= (src[l] == 1 ? 1u : 0u) << l;
  if (i >= j0 && i < j0 + 32) b &= ~(1u << (i - j0));   // a_ii is not a relation
  bits[w] = b;
}

// grid (B): mode 0 zeroes the class-count words of each commit, mode 1 turns the summed
// u32 counts into the f32 values the step kernels read (exact: counts < 2^24)
__global__ __launch_bounds__(256) void k_prep_ncst(uint32_t* __restrict__ prep, int Nc,
                                                   int stride, int o_ncst, int mode) {
  uint32_t* nc = prep + (size_t)blockIdx.x * stride + o_ncst;
  for (int e = threadIdx.x; e < 2 * Nc; e += 256) {
    if (mode == 0) nc[e] = 0u;
    else nc[e] = __float_as_uint((float)nc[e]);
  }
}

// k_prep_counts tile width: TI Ne-rows / -columns per block (<= 64 KiB of counters where
// possible, two blocks per CU), and the LDS words it needs
int prep_lds_words(int ne, int nc, int ti) {
  return (ti + 1) * nc + 2 * nc + ne + ti * ((ne + 31) / 32);
}
int prep_tile(int ne, int nc) {
  int ti = 64;
  while (ti > 16 && ti * nc > 16384) ti >>= 1;
  while (ti > 1 && prep_lds_words(ne, nc, ti) > 38 * 1024) ti >>= 1;
  return ti;
}

}  // namespace

namespace hdg {

hipError_t launch_prep_maps(const hdg_shape* s, const hdg_batch* bt, int stride, int o_ks,
                            int o_kt, int o_ncst, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_prep_counts,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const int ti = prep_tile(s->ne, s->nc);
  const size_t lds = (size_t)prep_lds_words(s->ne, s->nc, ti) * 4;
  uint32_t* prep = (uint32_t*)bt->prep;
  hipLaunchKernelGGL(k_prep_ncst, dim3(s->batch), dim3(256), 0, st, prep, s->nc, stride, o_ncst,
                     0);
  hipLaunchKernelGGL(k_prep_counts, dim3((s->ne + ti - 1) / ti, s->batch, 2), dim3(512), lds, st,
                     bt->abits, bt->hid, bt->nlen, prep, s->ne, s->nc, ti, stride, o_ks, o_kt,
                     o_ncst);
  hipLaunchKernelGGL(k_prep_ncst, dim3(s->batch), dim3(256), 0, st, prep, s->nc, stride, o_ncst,
                     1);
  return hipGetLastError();
}

int prep_fused(const hdg_shape* s, const hdg_batch* bt, hipStream_t st) {
  hipLaunchKernelGGL(k_prep_sort, dim3(s->batch), dim3(256), 0, st, bt->x, bt->abits,
                     (uint32_t*)bt->prep, s->ne, s->nc);
  HIP_TRY(hipGetLastError());
  const PrepLayout L = prep_layout(s->ne, s->nc);
  HIP_TRY(hdg::launch_prep_maps(s, bt, L.words, L.ks, L.kt, L.ncst, st));
  return 0;
}

}  // namespace hdg

extern "C" int hdg_pack_classes(const uint8_t* cls, int32_t batch, int32_t n, uint32_t* bits,
                                void* stream) {
  if (!cls || !bits || batch < 1 || n < 1)
    return fail(HDG_EINVAL, "hdg_pack_classes: NULL pointer or batch=%d n=%d", batch, n);
  const int W = (n + 31) / 32;
  const long long words = (long long)batch * n * W;
  hipLaunchKernelGGL(k_pack_classes, dim3((unsigned)((words + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, cls, n, W, words, bits);
  HIP_TRY(hipGetLastError());
  return 0;
}
