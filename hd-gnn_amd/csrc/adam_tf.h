// adam_tf.h -- the one statement of what ends a training step on every path: the loss
// terms and Adam factors of the pre-update parameters ("aux"), TF1 ApplyAdam of a parameter
// slot, and the step's loss stats.  Used by k_commit_step / k_reduce_adam / k_adam_tf
// (hdgnn.hip), the data-parallel tails and k_dp_aux (dp.hip), kw_derive / kw_ent_fwd /
// kw_reduce_adam (wide.hip).
//
// TF1 Adam (model_2.py:336-338): train_loss = 10 CE + 0.1 loss_map + loss_para.
//   g = dCE-part (from the reduction, already x10/(B Pc)) + 0.001 v
//       + [theta] 0.1*0.01*theta/|theta|
//   lr_t = lr sqrt(1-b2^t)/(1-b1^t);  m += (g-m)(1-b1); v += (g^2-v)(1-b2);
//   var -= lr_t m / (sqrt(v) + eps)     (tensorflow/core/kernels/training_ops.cc ApplyAdam)
#ifndef HDGNN_ADAM_TF_H
#define HDGNN_ADAM_TF_H

#include "hdgnn_internal.h"

namespace hdg {

constexpr float LOSS_CE_W = 10.f, LOSS_MAP_W = 0.1f;   // train_loss weights (model_2.py:336)
constexpr float LPARA_SCALE = 0.0005f;   // loss_para = 0.0005 sum w^2        (model_2.py:326-333)
constexpr float LMAP_SCALE = 0.01f;      // loss_map = 0.01 (|th2| + |th1|)   (model_2.py:123-130)
constexpr float LPARA_GRAD = 0.001f;     // d loss_para / dw = 2 x 0.0005 w
constexpr float LMAP_GRAD = 0.001f;      // 0.1 d loss_map / d theta = 0.1 x 0.01 theta / |theta|
// tf.train.AdamOptimizer's defaults (model_2.py:338; training_ops.cc ApplyAdam)
constexpr float ADAM_B1 = 0.9f, ADAM_B2 = 0.999f, ADAM_EPS = 1e-8f;

// aux: what a step's tail needs of the pre-update parameters and beta powers, written once
// per step (block 0 of k_commit_step, k_dp_aux, kw_derive / kw_ent_fwd at D_AUX) so that no
// block of the tail depends on another
enum AuxSlot : int {
  AUX_LPARA = 0,   // loss_para
  AUX_LMAP,        // loss_map
  AUX_N1,          // |map_theta1|
  AUX_N2,          // |map_theta2|
  AUX_LRF,         // sqrt(1 - b2^t) / (1 - b1^t): lr_t = lr x this
  AUX_B1P,         // b1^(t+1)
  AUX_B2P,         // b2^(t+1)
  AUX_LEN
};

__device__ __forceinline__ float loss_para(float l2_sum) { return LPARA_SCALE * l2_sum; }
__device__ __forceinline__ float loss_map(float n1, float n2) { return LMAP_SCALE * (n2 + n1); }

// one parameter's terms of the squared sums: all (loss_para), theta1, theta2 (the thetas
// close every variant's vector: np - 4 .. np - 1)
__device__ __forceinline__ void adam_sq_acc(int p, int np, float w, float& l2, float& t1,
                                            float& t2) {
  const int TH1 = np - 4, TH2 = np - 2;
  l2 = fmaf(w, w, l2);
  if (p >= TH1 && p < TH1 + 2) t1 = fmaf(w, w, t1);
  if (p >= TH2 && p < TH2 + 2) t2 = fmaf(w, w, t2);
}

// the norms come formed: each caller keeps its own summation
__device__ __forceinline__ void adam_aux_store(float* __restrict__ aux, float l2_sum, float n1,
                                               float n2, float b1p, float b2p) {
  aux[AUX_LPARA] = loss_para(l2_sum);
  aux[AUX_LMAP] = loss_map(n1, n2);
  aux[AUX_N1] = n1;
  aux[AUX_N2] = n2;
  aux[AUX_LRF] = sqrtf(1.f - b2p) / (1.f - b1p);
  aux[AUX_B1P] = b1p * ADAM_B1;
  aux[AUX_B2P] = b2p * ADAM_B2;
}

// The regularisation terms, moments and update of parameter slot p < np with reduced
// gradient g.  lr_t is the caller's: k_adam_tf forms lr * sqrtf(1 - b2p) / (1 - b1p) left to
// right, every other site lr * aux[AUX_LRF] with the quotient first.  The two differ in the
// last bit; both are kept as they are on purpose (each path's bits are pinned by its tests).
__device__ __forceinline__ void adam_tf_slot(int p, int np, float g, float w, float m0, float v0,
                                             float lr_t, float n1, float n2,
                                             float* __restrict__ params, float* __restrict__ mm,
                                             float* __restrict__ vv) {
  const int TH1 = np - 4, TH2 = np - 2;
  float gg = g + LPARA_GRAD * w;
  if (p >= TH1 && p < TH1 + 2) gg += LMAP_GRAD * w / n1;
  if (p >= TH2 && p < TH2 + 2) gg += LMAP_GRAD * w / n2;
  float m = m0, v = v0;
  m += (gg - m) * (1.f - ADAM_B1);
  v += (gg * gg - v) * (1.f - ADAM_B2);
  mm[p] = m;
  vv[p] = v;
  params[p] = w - lr_t * m / (sqrtf(v) + ADAM_EPS);
}

// stats[0..3]: CE, loss_map, loss_para, train_loss
__device__ __forceinline__ void step_stats_store(float* __restrict__ stats, float ce_sum,
                                                 float inv_pairs, float lmap, float lpara) {
  const float ce = ce_sum * inv_pairs;
  stats[0] = ce;
  stats[1] = lmap;
  stats[2] = lpara;
  stats[3] = LOSS_CE_W * ce + LOSS_MAP_W * lmap + lpara;
}

constexpr int ADAM_PT = 4;   // parameters per thread: 4 x 1024 >= every variant's count

// The squared sums of a whole parameter vector in one 1024-thread block (k_adam_tf,
// k_dp_aux): thread t holds w[u] = params[t + 1024 u] (0 past np); fmaf chain per thread,
// wave sums, then the 16 waves in a fixed order.  sh[0..2] = sum w^2, |theta1|^2, |theta2|^2,
// published to every thread.  red: [16 * 4] of LDS.
__device__ __forceinline__ void adam_sq_sums(const float (&w)[ADAM_PT], int np, float* red,
                                             float* sh) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float l2 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
  for (int u = 0; u < ADAM_PT; ++u) adam_sq_acc(t + u * 1024, np, w[u], l2, t1, t2);
  l2 = wave_sum(l2);
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
  if (lane == 0) { red[wv * 4] = l2; red[wv * 4 + 1] = t1; red[wv * 4 + 2] = t2; }
  __syncthreads();
  if (t < 3) {
    float s = 0.f;
    for (int q = 0; q < 16; ++q) s += red[q * 4 + t];
    sh[t] = s;
  }
  __syncthreads();
}

}  // namespace hdg

#endif  // HDGNN_ADAM_TF_H
