// Policy heads of the RL path (gfx950), fp32: forward with the action draw, backward, parameter gradient.
//   policy_heads       : actor/critic linear heads + categorical     (common/utils.py:16-50, rl/ppo/policy.py:15-23)
#include "rl_common.h"

namespace m2h {

// Philox4x32-10 (Salmon et al., SC'11: the counter-based generator torch's device generator is built on), one 32-bit word of the
// block at `counter` under `seed`, as Exp(1) noise: -log(u), u = (23 random bits + 0.5) / 2^23 in (0, 1) -- 23 bits, so that the sum
// is exact in fp32 (with 24 bits 0xFFFFFF + 0.5 rounds to 2^24: u = 1, noise 0, probs / noise = inf and that action wins whatever its
// probability): u in [2^-24, 1 - 2^-24], noise in [6.0e-8, 16.7].
__device__ __forceinline__ float philox_exp1(unsigned long long seed, unsigned long long counter) {
  unsigned c0 = (unsigned)counter, c1 = (unsigned)(counter >> 32), c2 = 0x6d32685fu, c3 = 0u;   // (c2: a stream tag)
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const float u = ((float)(c0 >> 9) + 0.5f) * (1.0f / 8388608.0f);
  return -logf(u);
}

// One wave per row: logits = feats Wa^T + ba (A <= 8 actions), value = feats Wc^T + bc; log-softmax, softmax, entropy,
// optional log-prob of a given action.  H multiple of 64.
__global__ __launch_bounds__(256) void policy_heads_kernel(const float* __restrict__ feats, const float* __restrict__ Wa,
                                                           const float* __restrict__ ba, const float* __restrict__ Wc,
                                                           const float* __restrict__ bc, const long long* __restrict__ actions,
                                                           float* __restrict__ value, float* __restrict__ logp_all,
                                                           float* __restrict__ probs, float* __restrict__ entropy,
                                                           float* __restrict__ logp_act, int M, int H, int A,
                                                           const float* __restrict__ noise = nullptr, long long* __restrict__ act_out = nullptr,
                                                           const unsigned long long* __restrict__ rng = nullptr,
                                                           float* __restrict__ noise_out = nullptr) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float acc[9];
#pragma unroll
  for (int a = 0; a < 9; ++a) acc[a] = 0.f;
  const float* f = feats + (size_t)row * H;
  if ((H & 255) == 0) {
    // (The heads' weights live back to back in FlatAdam's buffer -- the critic's row starts 12 bytes past a 16-byte boundary behind the
    // 3-float action bias: the 16-byte loads below are then dword-aligned only, which global loads accept on gfx950, as the GRU / skinny
    // kernels' loads of flat-buffer rows rely on too.  ONE path whatever the alignment: a second one would round differently, and the
    // same weights before and after they move into the flat buffer would give losses that differ in the last bit.)
    // 16 bytes per lane and load, every load of a pass issued before the first use (the scalar loop below is a chain of H / 64 dependent
    // load rounds: 10 us of a 14-row launch)
    typedef float f4 __attribute__((ext_vector_type(4)));
    for (int k = lane * 4; k < H; k += 256) {
      const f4 x = *reinterpret_cast<const f4*>(f + k);
      const f4 wc = *reinterpret_cast<const f4*>(Wc + k);
      f4 w[8];
#pragma unroll
      for (int a = 0; a < 8; ++a) w[a] = *reinterpret_cast<const f4*>(Wa + (size_t)(a < A ? a : 0) * H + k);
#pragma unroll
      for (int a = 0; a < 8; ++a)
        if (a < A) acc[a] += (x[0] * w[a][0] + x[1] * w[a][1]) + (x[2] * w[a][2] + x[3] * w[a][3]);
      acc[8] += (x[0] * wc[0] + x[1] * wc[1]) + (x[2] * wc[2] + x[3] * wc[3]);
    }
  } else {
    for (int k = lane; k < H; k += 64) {
      const float x = f[k];
#pragma unroll
      for (int a = 0; a < 8; ++a)
        if (a < A) acc[a] += x * Wa[a * H + k];
      acc[8] += x * Wc[k];
    }
  }
#pragma unroll
  for (int a = 0; a < 9; ++a) acc[a] = wave_sum(acc[a]);
  if (lane == 0) {
    float mx = -INFINITY;
    for (int a = 0; a < A; ++a) {
      acc[a] += ba[a];
      mx = fmaxf(mx, acc[a]);
    }
    float se = 0.f;
    for (int a = 0; a < A; ++a) se += expf(acc[a] - mx);
    const float lse = mx + logf(se);
    float ent = 0.f;
    for (int a = 0; a < A; ++a) {
      const float lp = acc[a] - lse;
      const float p = expf(lp);
      logp_all[row * A + a] = lp;
      probs[row * A + a] = p;
      ent -= lp * p;
    }
    value[row] = acc[8] + bc[0];
    entropy[row] = ent;
    if (actions != nullptr && logp_act != nullptr) logp_act[row] = logp_all[row * A + (int)actions[row]];
    if (act_out != nullptr) {
      // Policy.act in the same launch (rl/ppo/policy.py:217-225): the action -- with noise the single draw of torch.multinomial,
      // argmax(probs / Exp(1) noise), exactly as sample_actions_kernel takes it (correctly rounded division, NaN is the maximum,
      // ties keep the lowest index); without noise the mode, argmax(probs) -- and its log-probability
      // rng = {seed, counter} on the device ("fused" sampling): the Exp(1) noise of element (row, a) is -log(u), u from Philox4x32-10
      // keyed by the seed at counter + row A + a -- no generator launch in the step; the counter is advanced by step_index_advance
      // noise_out (optional, with rng): the noise drawn, [M][A] -- what the parity tests hand the CPU oracle in place of its generator's draw
      const bool draw = noise != nullptr || rng != nullptr;
      auto nz = [&](int a) {
        if (rng == nullptr) return noise[row * A + a];
        const float q = philox_exp1(rng[0], rng[1] + (unsigned long long)(row * A + a));
        if (noise_out != nullptr) noise_out[row * A + a] = q;
        return q;
      };
      int arg = 0;
      float best = draw ? expf(acc[0] - lse) / nz(0) : expf(acc[0] - lse);
      for (int a = 1; a < A; ++a) {
        const float p = expf(acc[a] - lse);
        const float q = draw ? p / nz(a) : p;
        if (!(best != best) && (q > best || q != q)) { best = q; arg = a; }
      }
      act_out[row] = arg;
      if (logp_act != nullptr) logp_act[row] = acc[arg] - lse;
    }
  }
}

__global__ void gather_logp_kernel(const float* __restrict__ logp_all, const long long* __restrict__ actions,
                                   float* __restrict__ out, int M, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) out[i] = logp_all[i * A + (int)actions[i]];
}

// argmax(probs / noise) per row: the single-draw path of torch.multinomial with caller-supplied Exp(1) noise (m2h_sample_actions).
// Correctly rounded fp32 division (hipcc's default), NaN counts as the maximum and ties keep the lowest index, as ATen's argmax.
// (The same loop closes policy_heads_kernel's fused draw.  The two stay two: written as one function -- the loop over a callable, or the
// comparison alone -- each compiles to other instructions than this text does, profiles/rl_split_isa.txt.)
__global__ void sample_actions_kernel(const float* __restrict__ probs, const float* __restrict__ noise, long long* __restrict__ actions,
                                      int M, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  float best = probs[i * A] / noise[i * A];
  int arg = 0;
  for (int j = 1; j < A; ++j) {
    const float q = probs[i * A + j] / noise[i * A + j];
    if (!(best != best) && (q > best || q != q)) { best = q; arg = j; }
  }
  actions[i] = arg;
}

// Parameter gradients of the two heads from dz [M][ZS] (policy_heads_bwd_kernel) and the features: dw[z][h] = sum_m dz[m][z] feats[m][h],
// db[z] = sum_m dz[m][z].  ZS x H = 8 x 512 outputs over a few hundred rows: the tiled weight-gradient engine spent 19 us + a 5 us reduce +
// a 4.5 us bias launch on it at the head of every policy epoch's backward.  A block owns 64 columns; its four waves take every fourth row
// (each lane: one column, ZS running sums; dz rows come through LDS), and meet in LDS in wave order (bit-reproducible).
template <int ZS>
__global__ __launch_bounds__(256) void policy_heads_wgrad_kernel(const float* __restrict__ feats, const float* __restrict__ dz,
                                                                 float* __restrict__ dw, float* __restrict__ db, int M, int H) {
  constexpr int RB = 64;                         // rows of dz staged per round
  __shared__ float zs[RB][ZS];
  __shared__ float part[4][ZS][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x * 64 + lane;
  float acc[ZS], bsum[ZS];
#pragma unroll
  for (int z = 0; z < ZS; ++z) acc[z] = bsum[z] = 0.f;
  for (int m0 = 0; m0 < M; m0 += RB) {
    __syncthreads();
    for (int i = tid; i < RB * ZS; i += 256) {
      const int r = i / ZS;
      zs[r][i - r * ZS] = m0 + r < M ? dz[(size_t)(m0 + r) * ZS + (i - r * ZS)] : 0.f;
    }
    __syncthreads();
    const int rn = min(RB, M - m0);
    float f[RB / 4];
#pragma unroll
    for (int j = 0; j < RB / 4; ++j) f[j] = feats[(size_t)min(m0 + wave + 4 * j, M - 1) * H + h];   // (all in flight; rows past the end are read clamped and not used)
#pragma unroll
    for (int j = 0; j < RB / 4; ++j) {
      const int r = wave + 4 * j;
      if (r < rn) {
#pragma unroll
        for (int z = 0; z < ZS; ++z) {
          acc[z] += zs[r][z] * f[j];
          bsum[z] += zs[r][z];
        }
      }
    }
  }
#pragma unroll
  for (int z = 0; z < ZS; ++z) part[wave][z][lane] = acc[z];
  __syncthreads();
  for (int i = tid; i < ZS * 64; i += 256) {
    const int z = i >> 6, l = i & 63;
    dw[(size_t)z * H + blockIdx.x * 64 + l] = (part[0][z][l] + part[1][z][l]) + (part[2][z][l] + part[3][z][l]);
  }
  if (blockIdx.x == 0) {       // the bias gradient: every lane of a wave holds the same row sums
    __syncthreads();
#pragma unroll
    for (int z = 0; z < ZS; ++z) part[wave][z][lane] = bsum[z];
    __syncthreads();
    if (tid < ZS) db[tid] = (part[0][tid][0] + part[1][tid][0]) + (part[2][tid][0] + part[3][tid][0]);
  }
}

// Backward of policy_heads_kernel: one wave per row.  g_value, g_logp, g_ent_rows = dL/d(value | logp_act | entropy) per row.
//   dz [M][ZS]: columns 0..A-1 = dL/dlogits, column A = dL/dvalue, rest 0   (ZS = A+1 rounded up to 4)
//   dfeats [M][H] = sum_a dlogit_a * Wa[a] + dvalue * Wc
__global__ __launch_bounds__(256) void policy_heads_bwd_kernel(const float* __restrict__ logp_all, const float* __restrict__ probs,
                                                               const long long* __restrict__ actions, const float* __restrict__ g_value,
                                                               const float* __restrict__ g_logp, const float* __restrict__ g_ent_rows, const float* __restrict__ Wa,
                                                               const float* __restrict__ Wc, float* __restrict__ dz,
                                                               float* __restrict__ dfeats, int M, int H, int A, int ZS) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float ent = 0.f;
  for (int a = 0; a < A; ++a) ent -= probs[row * A + a] * logp_all[row * A + a];
  const int act = actions != nullptr ? (int)actions[row] : -1;
  const float gl = g_logp != nullptr ? g_logp[row] : 0.f;
  const float gv = g_value != nullptr ? g_value[row] : 0.f;
  const float g_ent = g_ent_rows != nullptr ? g_ent_rows[row] : 0.f;
  float dl[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    dl[a] = 0.f;
    if (a < A) {
      const float p = probs[row * A + a], lp = logp_all[row * A + a];
      dl[a] = gl * ((a == act ? 1.f : 0.f) - p) + g_ent * (-p * (lp + ent));
    }
  }
  if (lane == 0) {
    for (int a = 0; a < ZS; ++a) dz[row * ZS + a] = a < A ? dl[a] : (a == A ? gv : 0.f);
  }
  for (int k = lane; k < H; k += 64) {
    float s = gv * Wc[k];
#pragma unroll
    for (int a = 0; a < 8; ++a)
      if (a < A) s += dl[a] * Wa[a * H + k];
    dfeats[(size_t)row * H + k] = s;
  }
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_policy_heads(const float* feats, const float* Wa, const float* ba, const float* Wc, const float* bc,
                     const long long* actions, float* value, float* logp_all, float* probs, float* entropy, float* logp_act,
                     int M, int H, int A, m2h_stream stream) {
  M2H_REQUIRE(feats && Wa && ba && Wc && bc && value && logp_all && probs && entropy, "policy_heads: null pointer");
  M2H_REQUIRE(M > 0 && H > 0 && H % 64 == 0 && A > 0 && A <= 8, "policy_heads: bad sizes (H %% 64, A <= 8)");
  M2H_LAUNCH(policy_heads_kernel, dim3((M + 3) / 4), dim3(256), 0, as_stream(stream), feats, Wa, ba, Wc, bc, actions, value,
                     logp_all, probs, entropy, logp_act, M, H, A);
  return launch_status("policy_heads");
}

int m2h_policy_heads_act(const float* feats, const float* Wa, const float* ba, const float* Wc, const float* bc, const float* noise,
                         float* value, float* logp_all, float* probs, float* entropy, long long* actions, float* logp_act, int M, int H,
                         int A, m2h_stream stream) {
  M2H_REQUIRE(feats && Wa && ba && Wc && bc && value && logp_all && probs && entropy && actions && logp_act, "policy_heads_act: null pointer");
  M2H_REQUIRE(M > 0 && H > 0 && H % 64 == 0 && A > 0 && A <= 8, "policy_heads_act: bad sizes (H %% 64, A <= 8)");
  M2H_LAUNCH(policy_heads_kernel, dim3((M + 3) / 4), dim3(256), 0, as_stream(stream), feats, Wa, ba, Wc, bc,
                     static_cast<const long long*>(nullptr), value, logp_all, probs, entropy, logp_act, M, H, A, noise, actions);
  return launch_status("policy_heads_act");
}

int m2h_policy_heads_act_rng(const float* feats, const float* Wa, const float* ba, const float* Wc, const float* bc, const unsigned long long* rng_state,
                             float* value, float* logp_all, float* probs, float* entropy, long long* actions, float* logp_act, float* noise_out,
                             int M, int H, int A, m2h_stream stream) {
  M2H_REQUIRE(feats && Wa && ba && Wc && bc && rng_state && value && logp_all && probs && entropy && actions && logp_act, "policy_heads_act_rng: null pointer");
  M2H_REQUIRE(M > 0 && H > 0 && H % 64 == 0 && A > 0 && A <= 8, "policy_heads_act_rng: bad sizes (H %% 64, A <= 8)");
  M2H_LAUNCH(policy_heads_kernel, dim3((M + 3) / 4), dim3(256), 0, as_stream(stream), feats, Wa, ba, Wc, bc,
             static_cast<const long long*>(nullptr), value, logp_all, probs, entropy, logp_act, M, H, A, static_cast<const float*>(nullptr), actions, rng_state,
             noise_out);
  return launch_status("policy_heads_act (fused draw)");
}

int m2h_sample_actions(const float* probs, const float* noise, long long* actions, int M, int A, m2h_stream stream) {
  M2H_REQUIRE(probs && noise && actions && M > 0 && A > 0 && A <= 64, "sample_actions: bad arguments");
  M2H_LAUNCH(sample_actions_kernel, dim3((M + 255) / 256), dim3(256), 0, as_stream(stream), probs, noise, actions, M, A);
  return launch_status("sample_actions");
}

int m2h_gather_logp(const float* logp_all, const long long* actions, float* out, int M, int A, m2h_stream stream) {
  M2H_REQUIRE(logp_all && actions && out && M > 0 && A > 0, "gather_logp: bad arguments");
  M2H_LAUNCH(gather_logp_kernel, dim3((M + 255) / 256), dim3(256), 0, as_stream(stream), logp_all, actions, out, M, A);
  return launch_status("gather_logp");
}

int m2h_policy_heads_bwd(const float* logp_all, const float* probs, const long long* actions, const float* g_value, const float* g_logp,
                         const float* g_ent, const float* Wa, const float* Wc, float* dz, float* dfeats, int M, int H, int A, int ZS,
                         m2h_stream stream) {
  M2H_REQUIRE(logp_all && probs && Wa && Wc && dz && dfeats && M > 0 && H > 0 && A > 0 && A <= 8 && ZS >= A + 1 && ZS % 4 == 0,
              "policy_heads_bwd: bad arguments");
  M2H_LAUNCH(policy_heads_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, as_stream(stream), logp_all, probs, actions, g_value, g_logp,
                     g_ent, Wa, Wc, dz, dfeats, M, H, A, ZS);
  return launch_status("policy_heads_bwd");
}

int m2h_policy_heads_wgrad(const float* feats, const float* dz, float* dw, float* db, int M, int H, int ZS, m2h_stream stream) {
  M2H_REQUIRE(feats && dz && dw && db && M > 0 && H > 0 && H % 64 == 0 && (ZS == 4 || ZS == 8), "policy_heads_wgrad: bad arguments (H %% 64, ZS 4 | 8)");
  if (ZS == 8) M2H_LAUNCH(policy_heads_wgrad_kernel<8>, dim3(H / 64), dim3(256), 0, as_stream(stream), feats, dz, dw, db, M, H);
  else M2H_LAUNCH(policy_heads_wgrad_kernel<4>, dim3(H / 64), dim3(256), 0, as_stream(stream), feats, dz, dw, db, M, H);
  return launch_status("policy_heads_wgrad");
}

}  // extern "C"
