// Losses and per-env distances of the RL path (gfx950), fp32: block reductions in a fixed order.
//   ppo_loss_fwd       : clipped surrogate + clipped value loss      (rl/ppo/ppo.py:125-157)
//   l1_loss / bin_l1   : the separators' L1 losses                   (rl/ppo/ppo.py:213-221)
//   sep_rewards        : -mse/mean(gt^2) per env (+variants)         (common/env_utils.py:690-713)
//   stft_l2            : STFT-L2 distance per env                    (common/eval_metrics.py:306-366)
#include "rl_common.h"

namespace m2h {

// block_sum for a 1024-thread block (16 waves), fixed summation order
__device__ __forceinline__ float block_sum16(float v, float* sh /* >= 16 floats */) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) t += sh[i];
  return t;
}

// PPO losses, forward + analytic gradients w.r.t. values, action_log_probs (and the entropy coefficient is applied by the
// caller).  out[0] = value_loss, out[1] = action_loss.  Single block.
__global__ __launch_bounds__(256) void ppo_loss_kernel(const float* __restrict__ values, const float* __restrict__ logp,
                                                       const float* __restrict__ old_values, const float* __restrict__ returns,
                                                       const float* __restrict__ adv, const float* __restrict__ old_logp,
                                                       float clip_host, const float* __restrict__ clip_dev, int use_clipped_value_loss,
                                                       float* __restrict__ out, float* __restrict__ g_values, float* __restrict__ g_logp,
                                                       float value_loss_coef, const float* __restrict__ entropy, float entropy_coef, int n) {
  __shared__ float sh[4];
  const float clip = clip_dev != nullptr ? clip_dev[0] : clip_host;  // device scalar: a replayed HIP graph follows the clip decay
  float sv = 0.f, sa = 0.f, se = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    if (entropy != nullptr) se += entropy[i];
    const float ratio = expf(logp[i] - old_logp[i]);
    const float a = adv[i];
    const float s1 = ratio * a;
    const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
    const float s2 = rc * a;
    sa += fminf(s1, s2);
    // d(-min(s1,s2))/dlogp: torch.min picks s1 when s1 <= s2 (ties -> first), clamp passes gradient inside [1-c, 1+c]
    float gl;
    if (s1 <= s2) gl = -a * ratio;
    else gl = (ratio >= 1.f - clip && ratio <= 1.f + clip) ? -a * ratio : 0.f;
    const float v = values[i], ov = old_values[i], R = returns[i];
    float vl, gv;
    if (use_clipped_value_loss) {
      const float dv = v - ov;
      const float vc = ov + fminf(fmaxf(dv, -clip), clip);
      const float l1 = (v - R) * (v - R), l2 = (vc - R) * (vc - R);
      if (l1 >= l2) {  // torch.max picks the first on ties
        vl = l1;
        gv = 2.f * (v - R);
      } else {
        vl = l2;
        gv = (dv >= -clip && dv <= clip) ? 2.f * (vc - R) : 0.f;
      }
    } else {
      vl = (R - v) * (R - v);
      gv = 2.f * (v - R);
    }
    sv += vl;
    if (g_logp != nullptr) g_logp[i] = gl / (float)n;
    if (g_values != nullptr) g_values[i] = 0.5f * gv / (float)n * value_loss_coef;
  }
  const float tv = block_sum(sv, sh);
  const float ta = block_sum(sa, sh);
  const float te = block_sum(se, sh);
  if (threadIdx.x == 0) {
    out[0] = 0.5f * tv / (float)n;
    out[1] = -ta / (float)n;
    out[2] = te / (float)n;                                                      // dist_entropy (mean over rows)
    out[3] = out[0] * value_loss_coef + out[1] - out[2] * entropy_coef;          // total_loss (ppo.py:150-154)
  }
}

// Per-env reductions over L = F*T*C elements (one 1024-thread block per env, four independent loads in flight per thread: the
// 256-thread serial loop was latency-bound at 24 us for 64 KB of input):
//   stats[e][0] = sum (p-g)^2, stats[e][1] = sum g^2  -> reward_util = -(s0/L)/(s1/L)
__global__ __launch_bounds__(1024) void sq_stats_kernel(const float* __restrict__ pred, const float* __restrict__ gt_comps, int gt_stride,
                                                        int gt_off, float* __restrict__ stats, int L) {
  __shared__ float sh[16];
  const int e = blockIdx.x;
  const float* p = pred + (size_t)e * L;
  const float* g = gt_comps + (size_t)e * L * gt_stride + gt_off;
  float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i0 = threadIdx.x; i0 < L; i0 += 4096) {
    float pv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 1024 * u;
      const bool ok = i < L;
      pv[u] = ok ? p[i] : 0.f;
      gv[u] = ok ? g[(size_t)i * gt_stride] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float d = pv[u] - gv[u];
      s0[u] += d * d;
      s1[u] += gv[u] * gv[u];
    }
  }
  const float t0 = block_sum16((s0[0] + s0[1]) + (s0[2] + s0[3]), sh);
  const float t1 = block_sum16((s1[0] + s1[1]) + (s1[2] + s1[3]), sh);
  if (threadIdx.x == 0) {
    stats[e * 2 + 0] = t0;
    stats[e * 2 + 1] = t1;
  }
}

// rewards[e] per override_rewards:  done -> 0;  else r = -(next0/L)/(next1/L);  quality_improvement: r -= -(cur0/L)/(cur1/L);
// otherwise r *= mult.
__global__ void rewards_from_stats_kernel(const float* __restrict__ next_stats, const float* __restrict__ cur_stats,
                                          const float* __restrict__ not_done, float* __restrict__ rewards, int N, int L, int quality,
                                          float mult) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  float r = 0.f;
  if (not_done[e] != 0.f) {
    r = -(next_stats[2 * e] / (float)L) / (next_stats[2 * e + 1] / (float)L);
    if (quality) r -= -(cur_stats[2 * e] / (float)L) / (cur_stats[2 * e + 1] / (float)L);
    else r *= mult;
  }
  rewards[e] = r;
}

// STFT-L2 per env (one 1024-thread block per env).  Both sides use the GT phase (common/eval_metrics.py STFT_L2_distance), so
// with m_g, m_p the magnitudes the reference's mean over (re, im, F, T) of (m_g cos - m_p cos)^2 and (m_g sin - m_p sin)^2 is
// (m_g - m_p)^2 (cos^2 + sin^2); the kernel evaluates (m_g - m_p)^2 directly -- equal to the term-by-term form to fp32 rounding
// (|cos^2 + sin^2 - 1| <= 2^-23), without 2 transcendental calls per element.  The phase plane is not read.
// pred magnitude p = (exp(mix)-1)*mask for the binaural channels (use_mix=1) or the tensor itself (mono).
__global__ __launch_bounds__(1024) void stft_l2_kernel(const float* __restrict__ mix, const float* __restrict__ pred, int Cp,
                                                       const float* __restrict__ gt_comps, int Cg, int nch, int use_mix,
                                                       float* __restrict__ out, int L /* F*T */) {
  __shared__ float sh[16];
  const int e = blockIdx.x;
  float tot = 0.f;
  for (int ch = 0; ch < nch; ++ch) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = threadIdx.x; i0 < L; i0 += 4096) {
      float gm[4], pm[4], mx[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 1024 * u;
        const bool ok = i < L;
        const size_t pix = (size_t)e * L + (ok ? i : 0);
        gm[u] = ok ? gt_comps[pix * Cg + 2 * ch] : 0.f;
        pm[u] = ok ? pred[pix * Cp + ch] : 0.f;
        mx[u] = (ok && use_mix) ? mix[pix * Cp + ch] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float p = use_mix ? (expf(mx[u]) - 1.f) * pm[u] : pm[u];
        const float d = gm[u] - p;
        s[u] += d * d;
      }
    }
    tot += block_sum16((s[0] + s[1]) + (s[2] + s[3]), sh) / (float)(2 * L);
  }
  if (threadIdx.x == 0) out[e] = tot;
}

// L1 loss against a strided ground truth (F.l1_loss(pred, gt_comps[..., off], reduction=mean); ppo.py:213,216,221):
// partial sums per block into part[blockIdx], grad[i] = sign(p - g) / n  (sign(0) = 0 like torch).
__global__ __launch_bounds__(256) void l1_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int gt_stride, int gt_off,
                                                      float* __restrict__ part, float* __restrict__ grad, size_t n) {
  __shared__ float sh[4];
  float s = 0.f;
  const float inv = 1.f / (float)n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = pred[i] - gt[i * gt_stride + gt_off];
    s += fabsf(d);
    if (grad != nullptr) grad[i] = d > 0.f ? inv : (d < 0.f ? -inv : 0.f);
  }
  const float t = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// The same loss for a prediction that is still in the convolution's NHWC layout [B][32 rows][T][16 bands] (AcousticMem's last conv before its
// de-slice, memory_nets.py:62-67): pred_BHWC[b][band * 32 + row][t] = y[b][row][t][band].  One block per (b, row): the 16 band rows of the
// ground truth (T x gt_stride floats each, contiguous) and the T x 16 tile of y are read coalesced, |y - g| is summed and the gradient
// sign(y - g) / n leaves in the SAME NHWC layout -- the layout the conv's weight / input gradient kernels read.  Replaces the conv's
// de-sliced store + m2h_l1_loss + the gradient's re-slice (m2h_slice_concat_input): one pass over y instead of three tensors' round trips.
__global__ __launch_bounds__(256) void l1_nhwc16_kernel(const float* __restrict__ y, const float* __restrict__ gt, int gt_stride, int gt_off, int T,
                                                        float* __restrict__ part, float* __restrict__ dy, float inv, int nrows) {
  extern __shared__ float gts[];                       // [16 bands][T] (+1 pad per band row)
  __shared__ float sh[4];
  const int TP = T + 1;
  float s = 0.f;
  for (int br = blockIdx.x; br < nrows; br += gridDim.x) {   // (b, row) pairs of this block: at most 2048 partial sums whatever B
    const int b = br >> 5, row = br & 31;
    __syncthreads();                                   // (the previous pair's tile is consumed)
    for (int i = threadIdx.x; i < 16 * T; i += 256) {  // band-major, coalesced over t
      const int band = i / T, t = i - band * T;
      gts[band * TP + t] = gt[(((size_t)b * 512 + band * 32 + row) * T + t) * gt_stride + gt_off];
    }
    __syncthreads();
    const size_t base = ((size_t)b * 32 + row) * T * 16;
    for (int i = threadIdx.x; i < 16 * T; i += 256) {  // NHWC order: band fastest
      const int t = i >> 4, band = i & 15;
      const float d = y[base + i] - gts[band * TP + t];
      s += fabsf(d);
      if (dy != nullptr) dy[base + i] = d > 0.f ? inv : (d < 0.f ? -inv : 0.f);
    }
  }
  const float tot = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// partial sums of a long list (one block per 1024 entries is overkill here: a few tens of thousands of floats) -> out[0] = scale * sum, fixed order
__global__ __launch_bounds__(1024) void sum_partials_wide_kernel(const float* __restrict__ part, int n, float scale, float* __restrict__ out) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) s += part[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += sh[w];
    out[0] = t * scale;
  }
}

// bin loss for logging (ppo.py:219-221; passive_trainer.py:270-272): mean | (exp(mix)-1)*mask - gt_bin_comps[..., 2c] | over [.., c<2]
__global__ __launch_bounds__(256) void bin_l1_kernel(const float* __restrict__ mix, const float* __restrict__ masks, const float* __restrict__ gt,
                                                     int Cg, int cstep, float* __restrict__ part, float* __restrict__ grad_masks, size_t npix) {
  __shared__ float sh[4];
  float s = 0.f;
  const float inv = 1.f / (float)(2 * npix);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * npix; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i >> 1;
    const int c = (int)(i & 1);
    const float e = expf(mix[i]) - 1.f;
    const float d = e * masks[i] - gt[pix * Cg + cstep * c];
    s += fabsf(d);
    if (grad_masks != nullptr) grad_masks[i] = (d > 0.f ? inv : (d < 0.f ? -inv : 0.f)) * e;
  }
  const float t = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// out[0] = scale * sum(part[0..n))   (one wave, fixed lane-strided order + butterfly: deterministic)
__global__ void sum_partials_kernel(const float* __restrict__ part, int n, float scale, float* __restrict__ out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += part[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[0] = s * scale;
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_ppo_loss(const float* values, const float* logp, const float* old_values, const float* returns, const float* adv,
                 const float* old_logp, const float* entropy, float clip, const float* clip_dev, int use_clipped_value_loss,
                 float value_loss_coef, float entropy_coef, float* out, float* g_values, float* g_logp, int n, m2h_stream stream) {
  M2H_REQUIRE(values && logp && old_values && returns && adv && old_logp && out && n > 0, "ppo_loss: bad arguments");
  M2H_LAUNCH(ppo_loss_kernel, dim3(1), dim3(256), 0, as_stream(stream), values, logp, old_values, returns, adv, old_logp, clip,
                     clip_dev, use_clipped_value_loss, out, g_values, g_logp, value_loss_coef, entropy, entropy_coef, n);
  return launch_status("ppo_loss");
}

int m2h_l1_loss(const float* pred, const float* gt, int gt_stride, int gt_off, float* loss, float* grad, float* scratch, size_t n,
                m2h_stream stream) {
  M2H_REQUIRE(pred && gt && loss && scratch && n > 0 && gt_stride > 0 && gt_off >= 0 && gt_off < gt_stride, "l1_loss: bad arguments");
  const unsigned g = grid_for(n, M2H_PARTS);
  M2H_LAUNCH(l1_loss_kernel, dim3(g), dim3(256), 0, as_stream(stream), pred, gt, gt_stride, gt_off, scratch, grad, n);
  M2H_LAUNCH(sum_partials_kernel, dim3(1), dim3(64), 0, as_stream(stream), scratch, (int)g, 1.f / (float)n, loss);
  return launch_status("l1_loss");
}

int m2h_l1_loss_nhwc16(const float* y, const float* gt, int gt_stride, int gt_off, float* loss, float* dy, float* scratch, int B, int T,
                       m2h_stream stream) {
  M2H_REQUIRE(y && gt && loss && scratch && B > 0 && T > 0 && T <= 256 && gt_stride > 0 && gt_off >= 0 && gt_off < gt_stride, "l1_loss_nhwc16: bad arguments");
  const size_t n = (size_t)B * 512 * T;
  const int nrows = B * 32, blocks = nrows < 2048 ? nrows : 2048;
  M2H_LAUNCH(l1_nhwc16_kernel, dim3((unsigned)blocks), dim3(256), 16 * (T + 1) * sizeof(float), as_stream(stream), y, gt, gt_stride, gt_off, T,
                     scratch, dy, 1.f / (float)n, nrows);
  M2H_LAUNCH(sum_partials_wide_kernel, dim3(1), dim3(1024), 0, as_stream(stream), scratch, blocks, 1.f / (float)n, loss);
  return launch_status("l1_loss_nhwc16");
}

int m2h_bin_l1_loss(const float* mix, const float* masks, const float* gt_bin_comps, int Cg, int cstep, float* loss, float* grad_masks,
                    float* scratch, size_t npix, m2h_stream stream) {
  M2H_REQUIRE(mix && masks && gt_bin_comps && loss && scratch && npix > 0 && cstep >= 1 && Cg >= cstep + 1, "bin_l1_loss: bad arguments");
  const unsigned g = grid_for(2 * npix, M2H_PARTS);
  M2H_LAUNCH(bin_l1_kernel, dim3(g), dim3(256), 0, as_stream(stream), mix, masks, gt_bin_comps, Cg, cstep, scratch, grad_masks, npix);
  M2H_LAUNCH(sum_partials_kernel, dim3(1), dim3(64), 0, as_stream(stream), scratch, (int)g, 1.f / (float)(2 * npix), loss);
  return launch_status("bin_l1_loss");
}

int m2h_sq_stats(const float* pred, const float* gt_comps, int gt_stride, int gt_off, float* stats, int N, int L, m2h_stream stream) {
  M2H_REQUIRE(pred && gt_comps && stats && N > 0 && L > 0 && gt_stride > 0 && gt_off >= 0 && gt_off < gt_stride, "sq_stats: bad arguments");
  M2H_LAUNCH(sq_stats_kernel, dim3(N), dim3(1024), 0, as_stream(stream), pred, gt_comps, gt_stride, gt_off, stats, L);
  return launch_status("sq_stats");
}

int m2h_rewards_from_stats(const float* next_stats, const float* cur_stats, const float* not_done, float* rewards, int N, int L,
                           int quality_improvement, float mult, m2h_stream stream) {
  M2H_REQUIRE(next_stats && not_done && rewards && N > 0 && L > 0 && (!quality_improvement || cur_stats), "rewards_from_stats: bad arguments");
  M2H_LAUNCH(rewards_from_stats_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), next_stats, cur_stats, not_done,
                     rewards, N, L, quality_improvement, mult);
  return launch_status("rewards_from_stats");
}

int m2h_stft_l2(const float* mix, const float* pred, int Cp, const float* gt_comps, int Cg, int nch, int use_mix, float* out, int N,
                int L, m2h_stream stream) {
  M2H_REQUIRE(pred && gt_comps && out && N > 0 && L > 0 && nch > 0 && Cp >= nch && Cg >= 2 * nch && (!use_mix || mix), "stft_l2: bad arguments");
  M2H_LAUNCH(stft_l2_kernel, dim3(N), dim3(1024), 0, as_stream(stream), mix, pred, Cp, gt_comps, Cg, nch, use_mix, out, L);
  return launch_status("stft_l2");
}

}  // extern "C"
