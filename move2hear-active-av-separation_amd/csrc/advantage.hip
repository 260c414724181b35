// Returns and advantages of a finished rollout (gfx950), fp32.  (The PPO loss that consumes them is with the other losses, losses.hip.)
//   gae_returns        : GAE / discounted-return scan                (common/rollout_storage.py:155-180)
//   normalize_adv      : advantage normalisation                     (rl/ppo/ppo.py:75-80; ddppo_utils.py:168-190)
#include "rl_common.h"

namespace m2h {

// GAE / discounted-return scan: one thread per env, T steps backwards.  rewards [T,N], value_preds [T+1,N] (row T is
// overwritten with next_value when use_gae), masks [T+1,N], returns [T+1,N].
__global__ void gae_returns_kernel(const float* __restrict__ rewards, float* __restrict__ value_preds, const float* __restrict__ masks,
                                   const float* __restrict__ next_value, float* __restrict__ returns, int T, int N, int use_gae,
                                   float gamma, float tau) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  if (use_gae) {
    value_preds[T * N + e] = next_value[e];
    float gae = 0.f;
    for (int s = T - 1; s >= 0; --s) {
      const float m = masks[(s + 1) * N + e];
      const float delta = rewards[s * N + e] + gamma * value_preds[(s + 1) * N + e] * m - value_preds[s * N + e];
      gae = delta + gamma * tau * m * gae;
      returns[s * N + e] = gae + value_preds[s * N + e];
    }
  } else {
    returns[T * N + e] = next_value[e];
    for (int s = T - 1; s >= 0; --s)
      returns[s * N + e] = returns[(s + 1) * N + e] * gamma * masks[(s + 1) * N + e] + rewards[s * N + e];
  }
}

// adv = returns[:-1] - value_preds[:-1]; stats[0] = sum(adv), stats[1] = sum((adv-mean)^2) for the local n elements.
// mode 0: adv only.  mode 1 (local): (adv-mean)/(std_unbiased+eps).  mode 2 (distributed step A): write raw adv + local mean
// to stats[0];  the host all-reduces and calls normalize_apply.  Single block (n = T*N is small).
__global__ __launch_bounds__(256) void advantages_kernel(const float* __restrict__ returns, const float* __restrict__ value_preds,
                                                         float* __restrict__ adv, float* __restrict__ stats, int n, int mode, float eps) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float a = returns[i] - value_preds[i];
    adv[i] = a;
    s += a;
  }
  const float mean = block_sum(s, sh) / (float)n;
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = adv[i] - mean;
    q += d * d;
  }
  const float ss = block_sum(q, sh);
  if (threadIdx.x == 0 && stats != nullptr) {
    stats[0] = mean;
    stats[1] = ss / (float)n;  // biased variance around the LOCAL mean (mode 2 recomputes around the global mean)
  }
  if (mode == 1) {
    const float sd = sqrtf(ss / (float)(n - 1));
    for (int i = threadIdx.x; i < n; i += 256) adv[i] = (adv[i] - mean) / (sd + eps);
  }
}

// distributed step B: sqdiff[0] = mean((adv - gmean)^2) locally;  step C: adv = (adv - gmean)/(sqrt(gvar)+eps)
__global__ __launch_bounds__(256) void adv_sqdiff_kernel(const float* __restrict__ adv, const float* __restrict__ gmean,
                                                         float* __restrict__ out, int n) {
  __shared__ float sh[4];
  const float m = gmean[0];
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = adv[i] - m;
    q += d * d;
  }
  const float ss = block_sum(q, sh);
  if (threadIdx.x == 0) out[0] = ss / (float)n;
}

__global__ void adv_apply_kernel(float* __restrict__ adv, const float* __restrict__ gmean, const float* __restrict__ gvar, int n, float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) adv[i] = (adv[i] - gmean[0]) / (sqrtf(gvar[0]) + eps);
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_gae_returns(const float* rewards, float* value_preds, const float* masks, const float* next_value, float* returns, int T,
                    int N, int use_gae, float gamma, float tau, m2h_stream stream) {
  M2H_REQUIRE(rewards && value_preds && masks && next_value && returns && T > 0 && N > 0, "gae_returns: bad arguments");
  M2H_LAUNCH(gae_returns_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), rewards, value_preds, masks, next_value,
                     returns, T, N, use_gae, gamma, tau);
  return launch_status("gae_returns");
}

int m2h_advantages(const float* returns, const float* value_preds, float* adv, float* stats, int n, int mode, float eps,
                   m2h_stream stream) {
  M2H_REQUIRE(returns && value_preds && adv && n > 1 && mode >= 0 && mode <= 2, "advantages: bad arguments");
  M2H_LAUNCH(advantages_kernel, dim3(1), dim3(256), 0, as_stream(stream), returns, value_preds, adv, stats, n, mode, eps);
  return launch_status("advantages");
}

int m2h_adv_sqdiff(const float* adv, const float* gmean, float* out, int n, m2h_stream stream) {
  M2H_REQUIRE(adv && gmean && out && n > 0, "adv_sqdiff: bad arguments");
  M2H_LAUNCH(adv_sqdiff_kernel, dim3(1), dim3(256), 0, as_stream(stream), adv, gmean, out, n);
  return launch_status("adv_sqdiff");
}

int m2h_adv_apply(float* adv, const float* gmean, const float* gvar, int n, float eps, m2h_stream stream) {
  M2H_REQUIRE(adv && gmean && gvar && n > 0, "adv_apply: bad arguments");
  M2H_LAUNCH(adv_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), adv, gmean, gvar, n, eps);
  return launch_status("adv_apply");
}

}  // extern "C"
