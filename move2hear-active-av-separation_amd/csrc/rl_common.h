// Helpers shared by the RL units (rnn.hip, policy_heads.hip, ppo.hip, losses.hip, optim.hip, rollout_ops.hip, rollout_fused.hip): one
// definition each.  A helper that a single unit uses stays in that unit (sigmoidf_: rnn.hip; block_sum16: losses.hip).
#pragma once
#include "m2h_internal.h"

namespace m2h {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block-wide sum (blockDim = 256); result valid in every thread.
__device__ __forceinline__ float block_sum(float v, float* sh /* >= 4 floats */) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// Blocks of 256 threads over `total` elements, capped.  (layout.hip has a grid_for of its own, with a block size and another cap: it
// does not include this header, and the two stay two.)
static inline unsigned grid_for(size_t total, unsigned cap = 4096) {
  size_t g = (total + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

#define M2H_PARTS 1024   // block cap of the partial-sum launches (l1_loss, bin_l1_loss: losses.hip; grad_clip_coef: optim.hip)

}  // namespace m2h
