// fused_tail.h -- the fused path's gradient layout and the deterministic reduction of the
// step kernel's partial rows, shared by the kernels that end a fused step: k_grad_reduce /
// k_reduce_adam / k_adam_tf (hdgnn.hip) and the data-parallel tails (dp.hip).  What those
// kernels do with a reduced slot (TF1 ApplyAdam, the aux block, the loss stats) is in
// adam_tf.h, which the general path's tail (wide.hip) shares.
#ifndef HDGNN_FUSED_TAIL_H
#define HDGNN_FUSED_TAIL_H

#include "hdgnn_internal.h"
#include "adam_tf.h"

namespace hdg {

constexpr int NT_MID = 1024;        // k_commit_step block

// model_2 flat parameter offsets (tf.global_variables order)
namespace m2 {
constexpr int E1_W1 = 0, E1_B1 = 80, E1_W5 = 100, E1_B5 = 500;
constexpr int E3_W1 = 520, E3_B1 = 940, E3_W2 = 960, E3_B2 = 980;
constexpr int H1_W1 = 981, H1_B1 = 1181, H1_W2 = 1201, H1_B2 = 1601;
constexpr int H2_W1 = 1621, H2_B1 = 2061, H2_W2 = 2081, H2_B2 = 2121;
constexpr int TH1 = 2123, TH2 = 2125, NP = 2127;
constexpr Off O = param_offsets(2);
#define HDG_M2_SAME(f) static_assert(f == O.f, "m2::" #f " differs from param_offsets(2)")
HDG_M2_SAME(E1_W1); HDG_M2_SAME(E1_B1); HDG_M2_SAME(E1_W5); HDG_M2_SAME(E1_B5);
HDG_M2_SAME(E3_W1); HDG_M2_SAME(E3_B1); HDG_M2_SAME(E3_W2); HDG_M2_SAME(E3_B2);
HDG_M2_SAME(H1_W1); HDG_M2_SAME(H1_B1); HDG_M2_SAME(H1_W2); HDG_M2_SAME(H1_B2);
HDG_M2_SAME(H2_W1); HDG_M2_SAME(H2_B1); HDG_M2_SAME(H2_W2); HDG_M2_SAME(H2_B2);
HDG_M2_SAME(TH1); HDG_M2_SAME(TH2); HDG_M2_SAME(NP);
#undef HDG_M2_SAME
}  // namespace m2
constexpr int GRAD_LEN = m2::NP + HDG_TRAILER;
constexpr int NPART = (GRAD_LEN + 3) & ~3;   // per-block partial row: NP grads + trailer

// system-scope write-through store of one word (status words the host or a peer reads)
__device__ __forceinline__ void xstore1(uint32_t* p, const uint32_t w) {
  asm volatile("global_store_dword %0, %1, off sc0 sc1" ::"v"(p), "v"(w) : "memory");
}

// ------------------------------------------------------------------------------
// deterministic reduction of the partial rows (one per block of k_commit_step): a
// 1024-thread block takes RED_P = 16 parameters x 64 row phases (row r -> phase r % 64,
// fixed order); a thread's <= 4 rows per trip are loaded before they are added (one
// memory round trip up to 256 rows), the 4 phases of a wave close with two permlane
// swaps, the 16 waves in a fixed-order LDS sum.  Bitwise reproducible.  The correct-
// prediction count (slot NP + HDG_TR_COUNT, an exact integer per row) is summed as an
// integer alongside and returned in `count` (thread pl of that slot's block).
// ------------------------------------------------------------------------------
constexpr int RED_P = 16, RED_PH = NT_MID / RED_P;   // 16 parameters x 64 phases
constexpr int CNT_SLOT = m2::NP + HDG_TR_COUNT;

struct RedShared {
  float s[NT_MID / 64][RED_P];
  uint32_t c[NT_MID / 16];             // per (wave, phase lane group) count partials
};

// `used` keeps a reference besides the calls: the compiler inlines a function whose only use
// is one call (dp.hip) by another route than one with several callers (hdgnn.hip), and the
// count sum's 62 integer adds then come out with their operands swapped.  With it every
// translation unit gets the same instructions (and one unused copy of this function).
__attribute__((used))
__device__ __forceinline__ float reduce_commits(const float* __restrict__ part, int R, int p,
                                                bool valid, RedShared& sh, uint32_t& count) {
  const int pl = threadIdx.x & (RED_P - 1), ph = threadIdx.x / RED_P;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool isc = p == CNT_SLOT;
  float acc = 0.f;
  uint32_t accu = 0u;
  if (valid) {
    for (int b0 = ph; b0 < R; b0 += 4 * RED_PH) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = b0 + u * RED_PH;
        v[u] = b < R ? part[(size_t)b * NPART + p] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += v[u];
      if (isc) {
#pragma unroll
        for (int u = 0; u < 4; ++u) accu += (uint32_t)v[u];
      }
    }
  }
  acc = xrow_sum4(acc);                 // the wave's 4 phases (lanes pl, pl+16, +32, +48)
  if (lane < RED_P) sh.s[wv][pl] = acc;
  if (isc) sh.c[wv * 4 + (lane >> 4)] = accu;
  __syncthreads();
  float g = 0.f;
  count = 0u;
  if (threadIdx.x < RED_P) {
#pragma unroll
    for (int q = 0; q < NT_MID / 64; ++q) g += sh.s[q][pl];
    if (isc)
      for (int q = 0; q < NT_MID / 16; ++q) count += sh.c[q];
  }
  return g;
}

// the trailer's count slots from the integer total (each part < 2^16: exact under any
// float all-reduce of up to 256 ranks)
__device__ __forceinline__ void put_count(float* __restrict__ out, const uint32_t c) {
  out[0] = (float)(c & 0xFFFFu);
  out[1] = (float)(c >> 16);
  out[2] = 0.f;
}

}  // namespace hdg

#endif  // HDGNN_FUSED_TAIL_H
