// xlane.h -- wave64 cross-lane and packed-math device primitives shared by every engine
// path of libhdgnn.so (hdgnn.hip, dp.hip, wide.hip, eval.hip).  The inline-asm helpers carry
// their own wait states (the compiler's hazard recognizer does not look inside inline asm;
// tests/test_isa_hazards.py scans the result), so each exists here exactly once.
#ifndef HDGNN_XLANE_H
#define HDGNN_XLANE_H

#include <hip/hip_runtime.h>

namespace hdg {

template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                                               CTRL, 0xF, 0xF, false));
}

// Sum over a 16-lane DPP row; every lane of the row receives the total.  FIRST is the DPP
// control of the first step: the two paths pair lanes differently there (different fp32
// rounding), and each keeps its own bits.
constexpr int ROW_MIRROR = 0x140;   // lane i <- 15-i   (fused path)
constexpr int ROW_ROR8 = 0x128;     // lane i <- i ^ 8  (general path)
template <int FIRST>
__device__ __forceinline__ float row16_sum(float v) {
  v += dppf<FIRST>(v);
  v += dppf<0x141>(v);  // row_half_mirror   lane i <- 7-i (per 8)
  v += dppf<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dppf<0xB1>(v);   // quad_perm [1,0,3,2]
  return v;
}

// x <-> y exchange of DPP rows: swap32 trades x's lanes 32-63 for y's lanes 0-31, swap16
// x's rows 1, 3 for y's rows 0, 2.  v_permlane{32,16}_swap in the VALU (no LDS); inline asm
// because the ROCm 7.2 builtins mis-assign the two results, with the two wait states the
// swap needs after a VALU write of its operands inside the string.
__device__ __forceinline__ void swap32(float& x, float& y) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
}
__device__ __forceinline__ void swap16(float& x, float& y) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
}

// Sum over the 4 DPP rows of a wave for every lane column: lane l gets
// v[l] + v[l^16] + v[l^32] + v[l^48] (the swaps above, same hazard handling).
__device__ __forceinline__ float xrow_sum4(float v) {
  float x = v, y = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
  const float s = x + y;
  float p = s, q = s;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(p), "+v"(q));
  return p + q;
}

// whole-wave sum in the fused path's lane pairing, every lane receives it
__device__ __forceinline__ float wave_sum(float v) { return xrow_sum4(row16_sum<ROW_MIRROR>(v)); }

__device__ __forceinline__ float relu(float v) { return fmaxf(v, 0.f); }
// ln x for x in [1, 2] (the two-class CE's log(1 + e^-|d|) and log(e0 + e1)): v_log_f32
// (log2, ~1 ulp, no denormal range to guard) times ln 2 -- 2 VALU ops where logf expands to
// a denormal-scaled, split-constant sequence of ~11
__device__ __forceinline__ float ln_1to2(float x) { return __builtin_amdgcn_logf(x) * 0.693147182f; }

__device__ __forceinline__ int top_pow2(int n) {   // largest power of two <= n (n >= 1)
  return 1 << (31 - __builtin_clz((unsigned)n));
}

typedef float f2 __attribute__((ext_vector_type(2)));   // packed fp32 (v_pk_* ops)

// [z > 0] for two lanes of a packed pair in ONE VALU op: clamp(z * 2^126, 0, 1) on
// v_pk_mul_f32 (exact for every normal z; -0, NaN -> 0).  Used as step2(z) * w, which
// needs w finite wherever z <= 0 (padding rows / columns are kept finite).
__device__ __forceinline__ f2 step2(f2 z) {
  f2 r;
  asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(z), "v"((f2){0x1p126f, 0x1p126f}));
  return r;
}

// [x + c > 0] for a packed pair in ONE op where only the step of the sum is used (the
// backward passes' masks): clamp(fma(x, 2^64, c 2^64)).  The fma rounds the exact
// (x + c) 2^64 once: 0 for x + c <= 0 (-0, NaN: 0), 1 for every x + c >= 2^-64, so it
// differs from step2(fl(x + c)) only for 0 < x + c < 2^-64.  cs = c 2^64 (exact and finite
// for |c| < 2^63; -inf, as PADNEG 2^64 is, masks the pair).
#ifndef HDG_STEPF
#define HDG_STEPF 1
#endif
constexpr float STEP_S = 0x1p64f;
__device__ __forceinline__ f2 stepf2(f2 x, f2 cs) {
  f2 r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 clamp"
      : "=v"(r) : "v"(x), "s"((f2){STEP_S, STEP_S}), "v"(cs));
  return r;
}

// ------------------------------------------------------------------------------
// MFMA 16x16 fp32 tile (v_mfma_f32_16x16x4_f32) used by both paths
// ------------------------------------------------------------------------------
typedef float f4v __attribute__((ext_vector_type(4)));

// The tile with strided operands: lane l supplies row r = l & 15 of A as
// pa[k * sa] and column r of B as pb[k * sb], k < K.  A row / column outside the matrix
// passes a pointer to a 0.f word with stride 0 (a row of ones: a 1.f word, stride 0), so
// the K loop carries no bounds logic: one LDS read and one address add per operand.
// BATCH pins the 16-step body's schedule to its source order: the eight operand reads, then
// the four MFMAs (each behind the partial wait its own pair needs).  Without it the scheduler
// interleaves read, wait, MFMA under register pressure: one LDS round trip per k step.  Same
// operands in the same steps either way; the fused step kernel asks for it, the general
// path keeps the scheduler's choice.
template <bool BATCH = false>
__device__ __forceinline__ f4v mfma_tile16_p(const float* pa, const int sa, const float* pb,
                                             const int sb, const int K, const int lane) {
  const int q = lane >> 4;
  const float* a = pa + q * sa;
  const float* b = pb + q * sb;
  const int sa4 = 4 * sa, sb4 = 4 * sb;
  f4v c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
  int k = 0;
  for (; k + 16 <= K; k += 16) {
    float av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = a[u * sa4];
      bv[u] = b[u * sb4];
    }
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], c1, 0, 0, 0);
    if constexpr (BATCH) {
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);   // 8 DS reads
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // then 4 MFMAs
    }
    a += 4 * sa4;
    b += 4 * sb4;
  }
  for (; k + 4 <= K; k += 4) {
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c0, 0, 0, 0);
    a += sa4;
    b += sb4;
  }
  if (k < K) {                       // K % 4 tail: entries k + q >= K are selected to zero
    const bool ok = k + q < K;       // (callers' arrays are padded, the read stays in LDS)
    const float av = ok ? a[0] : 0.f, bv = ok ? b[0] : 0.f;
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c0, 0, 0, 0);
  }
  return c0 + c1;
}

}  // namespace hdg

#endif  // HDGNN_XLANE_H
