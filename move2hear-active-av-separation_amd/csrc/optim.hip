// Optimiser step of the RL path (gfx950), fp32, over a flat parameter buffer: gradient-norm clipping (torch clip_grad_norm_) and
// torch.optim.Adam.
#include "rl_common.h"

namespace m2h {

// sum of squares partials (grad-norm): part[blockIdx] = sum x^2 over the block's grid-stride share
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, size_t n, float* __restrict__ part) {
  __shared__ float sh[4];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += x[i] * x[i];
  const float t = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// clip_grad_norm_ coefficient (torch: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1): coef[0] = coefficient,
// coef[1] = total_norm.  part holds nparts sums of squares.  max_norm <= 0 -> coef 1.
__global__ void clip_coef_kernel(const float* __restrict__ part, int nparts, float max_norm, float* __restrict__ coef) {
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 64) s += part[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(s);
    float c = 1.f;
    if (max_norm > 0.f) c = fminf(max_norm / (norm + 1e-6f), 1.f);
    coef[0] = c;
    coef[1] = norm;
  }
}

// torch.optim.Adam step (no amsgrad, no weight decay) over a flat buffer; the gradient is scaled by coef[0] (clip) * gscale
// (1/world_size after a sum all-reduce) and written back scaled (as clip_grad_norm_ does in place).
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   size_t n, float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                   const float* __restrict__ coef, float gscale, const float* __restrict__ hyper) {
  const float c = (coef != nullptr ? coef[0] : 1.f) * gscale;
  if (hyper != nullptr) {   // m2h_adam_step_dev: the step-dependent scalars come from device memory (a replayed HIP graph holds no host scalars)
    lr = hyper[0];
    bc1 = hyper[1];
    bc2_sqrt = hyper[2];
  }
  const float step = lr / bc1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * c;
    g[i] = gi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] -= step * (mi / denom);
  }
}

__global__ void set3_kernel(float* __restrict__ dst, float a, float b, float c) {
  dst[0] = a;
  dst[1] = b;
  dst[2] = c;
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_grad_clip_coef(const float* g, size_t n, float max_norm, float* coef, float* scratch, m2h_stream stream) {
  M2H_REQUIRE(g && coef && scratch && n > 0, "grad_clip_coef: bad arguments");
  const unsigned gr = grid_for(n, M2H_PARTS);
  M2H_LAUNCH(sumsq_kernel, dim3(gr), dim3(256), 0, as_stream(stream), g, n, scratch);
  M2H_LAUNCH(clip_coef_kernel, dim3(1), dim3(64), 0, as_stream(stream), scratch, (int)gr, max_norm, coef);
  return launch_status("grad_clip_coef");
}

int m2h_adam_step(float* p, float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, int step,
                  const float* coef, float gscale, m2h_stream stream) {
  M2H_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adam_step: bad arguments");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2 = 1.f - powf(beta2, (float)step);
  M2H_LAUNCH(adam_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, as_stream(stream), p, g, m, v, n, lr, beta1, beta2, eps, bc1,
                     sqrtf(bc2), coef, gscale, (const float*)nullptr);
  return launch_status("adam_step");
}

int m2h_adam_hyper(float lr, float beta1, float beta2, int step, float* hyper, m2h_stream stream) {
  M2H_REQUIRE(hyper && step >= 1, "adam_hyper: bad arguments");
  // host arithmetic of m2h_adam_step (both entries take the same step); the values travel as kernel arguments: stream-ordered, no
  // host buffer to keep alive, no blocking copy
  M2H_LAUNCH(set3_kernel, dim3(1), dim3(1), 0, as_stream(stream), hyper, lr, 1.f - powf(beta1, (float)step),
                     sqrtf(1.f - powf(beta2, (float)step)));
  return launch_status("adam_hyper");
}

int m2h_adam_step_dev(float* p, float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2, float eps,
                      const float* coef, float gscale, m2h_stream stream) {
  M2H_REQUIRE(p && g && m && v && hyper && n > 0, "adam_step_dev: bad arguments");
  M2H_LAUNCH(adam_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, as_stream(stream), p, g, m, v, n, 0.f, beta1, beta2, eps, 1.f, 1.f, coef,
                     gscale, hyper);
  return launch_status("adam_step_dev");
}

}  // extern "C"
