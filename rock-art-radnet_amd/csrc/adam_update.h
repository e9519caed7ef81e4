// The per-element update of keras.optimizers.Adam (Keras 2 rule, train.py:236-252): ONE routine for every kernel that applies it --
// the arena sweeps of adam.hip and the tile epilogue of the weight-gradient kernel (conv_wgrad_body.h) -- so that a weight comes out
// with the same bits whichever of them updates it.  The floating-point contraction is pinned: the two fused multiply-adds are written
// out (they are the ones the compiler formed in adam_kernel when the choice was its own) and nothing else may fuse.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)   (keras.optimizers.Adam.get_updates); host side, one expression for every entry point
static inline float radnet_adam_lr_t(float lr, float beta1, float beta2, int t) {
  return (float)((double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
}

__device__ __forceinline__ void adam_update1(float& p, const float g, float& m, float& v, const float lr_t, const float b1, const float b2,
                                             const float eps, const float gs) {
#pragma clang fp contract(off)
  const float gq = g * gs;
  const float m1 = (1.f - b1) * gq;
  const float v1 = ((1.f - b2) * gq) * gq;
  m = __builtin_fmaf(m, b1, m1);
  v = __builtin_fmaf(v, b2, v1);
  const float num = lr_t * m, den = sqrtf(v) + eps;
  const float q = num / den;
  p = p - q;
}
