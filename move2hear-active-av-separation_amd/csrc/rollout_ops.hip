// HBM-bound glue of the rollout (gfx950): network input layouts, the storages' row copies, the synthetic environment's step.
//   slice_concat_input : AcousticMem / AudioCNN input glue          (memory_nets.py:40-59, audio_cnn.py:117-133)
//   visual_input       : rgb/255 (+depth) -> NHWC padded to 4 ch     (visual_cnn.py:135-150)
#include "rl_common.h"

namespace m2h {

// out[b][h][t][c*16+s] = f(virtual[b][s*Hs+h][t][c]),  virtual channel c < Ca -> a[..][c] (times mul[..][c] inside op 1),
// else b[..][c-Ca] * bscale[batch].   op: 0 none | 1 log1p(max(0, mul*(exp(a)-1))) | 2 log1p(max(0, x))
__global__ __launch_bounds__(256) void slice_concat_kernel(const float* __restrict__ a, int Ca, const float* __restrict__ bsrc, int Cb,
                                                           const float* __restrict__ mul, const float* __restrict__ bscale, int op,
                                                           float* __restrict__ out, int B, int F, int T) {
  const int C = Ca + Cb;
  const int Hs = F >> 4;
  const int CG = (16 * C) >> 2;
  const size_t total = (size_t)B * Hs * T * CG;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int cg = (int)(i % CG);
    size_t r = i / CG;
    const int t = (int)(r % T);
    r /= T;
    const int h = (int)(r % Hs);
    const int b = (int)(r / Hs);
    const int n0 = cg * 4;
    const int c = n0 >> 4, s0 = n0 & 15;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t pix = ((size_t)b * F + (size_t)(s0 + j) * Hs + h) * T + t;
      float x;
      if (c < Ca) {
        x = a[pix * Ca + c];
        if (op == 1) x = log1pf(fmaxf(mul[pix * Ca + c] * (expf(x) - 1.f), 0.f));
      } else {
        x = bsrc[pix * Cb + (c - Ca)];
        if (bscale != nullptr) x *= bscale[b];
      }
      if (op == 2) x = log1pf(fmaxf(x, 0.f));
      v[j] = x;
    }
    *reinterpret_cast<f32x4*>(out + i * 4) = v;
  }
}

// rgb [B,H,W,3] (0..255) (+ depth [B,H,W,1]) -> out [B,H,W,4] = (r/255, g/255, b/255, depth or 0)
__global__ __launch_bounds__(256) void visual_input_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                           float* __restrict__ out, size_t npix) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 v;
    v[0] = rgb[i * 3 + 0] / 255.0f;
    v[1] = rgb[i * 3 + 1] / 255.0f;
    v[2] = rgb[i * 3 + 2] / 255.0f;
    v[3] = depth != nullptr ? depth[i] : 0.f;
    *reinterpret_cast<f32x4*>(out + i * 4) = v;
  }
}

// Per-episode statistics of the rollout step (ppo_trainer.py:407-478: the reference keeps them as python floats / numpy and
// pays a host sync per value): one thread per env does what the reference does after every env step -- accumulate the
// running sums of the current episode, fold them into the finished-episode totals where the env is done (nd = 1 - not_done),
// reset the running sums there.  Arithmetic order and rounding are those of the elementwise formulation
// (cur += x; total += nd * (cur / steps); cur *= not_done), without fused multiply-adds.
__global__ void episode_stats_kernel(m2h_episode_stats st, const float* __restrict__ rewards, const float* __restrict__ dist_probs,
                                     const float* __restrict__ bin_losses, const float* __restrict__ mono_losses,
                                     const float* __restrict__ mem_losses, const float* __restrict__ not_done,
                                     const float* __restrict__ ndgs, const float* __restrict__ dgs, int N, int A) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const float m = not_done[e];
  const float nd = 1.f - m;
  if (ndgs) st.episode_ndgs[e] = __fadd_rn(st.episode_ndgs[e], __fmul_rn(nd, ndgs[e]));
  if (dgs) st.episode_dgs[e] = __fadd_rn(st.episode_dgs[e], __fmul_rn(nd, dgs[e]));
  const float cr = __fadd_rn(st.current_episode_reward[e], rewards[e]);
  const float cs = __fadd_rn(st.current_episode_step[e], 1.f);
  const float cb = __fadd_rn(st.current_episode_bin_losses[e], bin_losses[e]);
  const float cm = __fadd_rn(st.current_episode_mono_losses[e], mono_losses[e]);
  const float cf = __fadd_rn(st.current_episode_monoFromMem_losses[e], mem_losses[e]);
  st.episode_rewards[e] = __fadd_rn(st.episode_rewards[e], __fmul_rn(nd, cr));
  st.episode_steps[e] = __fadd_rn(st.episode_steps[e], __fmul_rn(nd, cs));
  st.episode_counts[e] = __fadd_rn(st.episode_counts[e], nd);
  for (int a = 0; a < A; ++a) {
    const float cp = __fadd_rn(st.current_episode_dist_probs[e * A + a], dist_probs[e * A + a]);
    st.episode_dist_probs[e * A + a] = __fadd_rn(st.episode_dist_probs[e * A + a], __fmul_rn(nd, __fdiv_rn(cp, cs)));
    st.current_episode_dist_probs[e * A + a] = __fmul_rn(cp, m);
  }
  st.episode_bin_losses_allSteps[e] = __fadd_rn(st.episode_bin_losses_allSteps[e], __fmul_rn(nd, __fdiv_rn(cb, cs)));
  st.episode_mono_losses_lastStep[e] = __fadd_rn(st.episode_mono_losses_lastStep[e], __fmul_rn(nd, mono_losses[e]));
  st.episode_mono_losses_allSteps[e] = __fadd_rn(st.episode_mono_losses_allSteps[e], __fmul_rn(nd, __fdiv_rn(cm, cs)));
  st.episode_monoFromMem_losses_lastStep[e] = __fadd_rn(st.episode_monoFromMem_losses_lastStep[e], __fmul_rn(nd, mem_losses[e]));
  st.episode_monoFromMem_losses_allSteps[e] = __fadd_rn(st.episode_monoFromMem_losses_allSteps[e], __fmul_rn(nd, __fdiv_rn(cf, cs)));
  st.current_episode_reward[e] = __fmul_rn(cr, m);
  st.current_episode_step[e] = __fmul_rn(cs, m);
  st.current_episode_bin_losses[e] = __fmul_rn(cb, m);
  st.current_episode_mono_losses[e] = __fmul_rn(cm, m);
  st.current_episode_monoFromMem_losses[e] = __fmul_rn(cf, m);
}

// Batched row copies with device-resident row indices (RolloutStoragePol/Sep.insert and the per-step row reads of the rollout,
// common/rollout_storage.py:68-96, 372-390, when the step is replayed from a HIP graph): item i copies `bytes` bytes from
// src + idx[src_slot] * bytes to dst + idx[dst_slot] * bytes (slot < 0: no offset).  grid.y = item, grid.x strides over it.
struct RowsCopyArgs {
  m2h_row_copy item[M2H_ROWS_COPY_MAX];
};
__global__ __launch_bounds__(256) void rows_copy_kernel(RowsCopyArgs a, const long long* __restrict__ idx) {
  const m2h_row_copy it = a.item[blockIdx.y];
  const char* src = static_cast<const char*>(it.src) + (it.src_slot >= 0 ? (size_t)idx[it.src_slot] * it.bytes : 0);
  char* dst = static_cast<char*>(it.dst) + (it.dst_slot >= 0 ? (size_t)idx[it.dst_slot] * it.bytes : 0);
  const size_t start = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (((reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst) | it.bytes) & 15) == 0) {  // block-uniform
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (size_t i = start; i < it.bytes / 16; i += stride) d4[i] = s4[i];
  } else {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d1 = reinterpret_cast<uint32_t*>(dst);
    for (size_t i = start; i < it.bytes / 4; i += stride) d1[i] = s1[i];
  }
}

// Device-resident step counters of the two rollout storages, idx = (pol_step, pol_step + 1, sep_step + 1), advanced at the end
// of a replayed rollout step (RolloutStoragePol/Sep.insert: step = (step + 1) % num_steps, common/rollout_storage.py:96,390).
__global__ void step_index_advance_kernel(long long* __restrict__ idx, int T_pol, int T_sep, unsigned long long* __restrict__ rng = nullptr,
                                          unsigned long long rng_inc = 0) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (rng != nullptr) rng[1] += rng_inc;   // the fused sampler's counter: past the step's draws
    const long long p = (idx[0] + 1) % T_pol;
    const long long s = idx[2] % T_sep;   // idx[2] holds sep_step + 1
    idx[0] = p;
    idx[1] = p + 1;
    idx[2] = s + 1;
  }
}

// Synthetic vector env (m2h/envs/synthetic_env.py; stands in for the simulator's pose update, habitat_audio/simulator_train.py):
// action 0 = MOVE_FORWARD (node + 1), 1 = TURN_LEFT (angle + 1), 2 = TURN_RIGHT (angle + 3), all modulo; one thread per env.
__global__ void synth_env_step_kernel(const long long* __restrict__ actions, long long* __restrict__ node, long long* __restrict__ angle,
                                      int n_nodes, int N) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const long long a = actions[e];
  node[e] = (node[e] + (a == 0 ? 1 : 0)) % n_nodes;
  angle[e] = (angle[e] + (a == 1 ? 1 : 0) + (a == 2 ? 3 : 0)) % 4;
}

// Batched row gathers: item i copies, for every env e < N, row index[sel_i][e] * mul_i + add[e] * ... of src_i to row e of dst_i.
// Serves the synthetic env's observation lookup (cached frames indexed by node * 4 + angle, audio pool indexed per env): six
// index_select launches as one.  index: [2][N] int64 = (frame index parts, audio index); frame row = node * 4 + angle.
struct RowsGatherArgs {
  m2h_row_copy item[M2H_ROWS_COPY_MAX];   // src_slot: 0 = frame index (node * 4 + angle), 1 = audio index; dst_slot unused
};
__global__ __launch_bounds__(256) void rows_gather_kernel(RowsGatherArgs a, const long long* __restrict__ node,
                                                          const long long* __restrict__ angle, const long long* __restrict__ audio_idx) {
  const m2h_row_copy it = a.item[blockIdx.z];
  const int e = blockIdx.y;
  const long long row = it.src_slot == 0 ? node[e] * 4 + angle[e] : audio_idx[e];
  const char* src = static_cast<const char*>(it.src) + (size_t)row * it.bytes;
  char* dst = static_cast<char*>(it.dst) + (size_t)e * it.bytes;
  const size_t start = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (((reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst) | it.bytes) & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (size_t i = start; i < it.bytes / 16; i += stride) d4[i] = s4[i];
  } else {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d1 = reinterpret_cast<uint32_t*>(dst);
    for (size_t i = start; i < it.bytes / 4; i += stride) d1[i] = s1[i];
  }
}

// Minibatch gather of the recurrent generators (common/rollout_storage.py:182-298,392-457):
// dst[t][j][:] = src[t][perm[j]][:]  for t < T, j < Nsel; rows of L elements (bytes, copied as 16-byte or 4-byte words).
__global__ __launch_bounds__(256) void gather_envs_kernel(const uint32_t* __restrict__ src, const long long* __restrict__ perm,
                                                          uint32_t* __restrict__ dst, int T, int N, int Nsel, size_t Lw) {
  const size_t total = (size_t)T * Nsel * Lw;
  if ((Lw & 3) == 0) {
    const size_t L4 = Lw >> 2;
    const size_t tot4 = (size_t)T * Nsel * L4;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot4; i += (size_t)gridDim.x * blockDim.x) {
      const size_t l = i % L4;
      const size_t r = i / L4;
      const int j = (int)(r % Nsel);
      const int t = (int)(r / Nsel);
      d4[i] = s4[((size_t)t * N + (size_t)perm[j]) * L4 + l];
    }
    return;
  }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t l = i % Lw;
    const size_t r = i / Lw;
    const int j = (int)(r % Nsel);
    const int t = (int)(r / Nsel);
    dst[i] = src[((size_t)t * N + (size_t)perm[j]) * Lw + l];
  }
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_slice_concat_input(const float* a, int Ca, const float* b, int Cb, const float* mul, const float* bscale, int op,
                           float* out, int B, int F, int T, m2h_stream stream) {
  M2H_REQUIRE(a != nullptr && out != nullptr && Ca > 0 && Cb >= 0, "slice_concat_input: bad arguments");
  M2H_REQUIRE((Cb == 0) == (b == nullptr), "slice_concat_input: b/Cb mismatch");
  M2H_REQUIRE(op >= 0 && op <= 2 && (op != 1 || mul != nullptr), "slice_concat_input: bad op");
  M2H_REQUIRE(B > 0 && F > 0 && T > 0 && F % 16 == 0, "slice_concat_input: bad sizes (F %% 16)");
  const size_t total = (size_t)B * (F / 16) * T * (16 * (Ca + Cb) / 4);
  M2H_LAUNCH(slice_concat_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), a, Ca, b, Cb, mul, bscale, op, out, B, F, T);
  return launch_status("slice_concat_input");
}

int m2h_visual_input(const float* rgb, const float* depth, float* out, int B, int H, int W, m2h_stream stream) {
  M2H_REQUIRE(rgb != nullptr && out != nullptr && B > 0 && H > 0 && W > 0, "visual_input: bad arguments");
  const size_t npix = (size_t)B * H * W;
  M2H_LAUNCH(visual_input_kernel, dim3(grid_for(npix)), dim3(256), 0, as_stream(stream), rgb, depth, out, npix);
  return launch_status("visual_input");
}

int m2h_gather_envs(const void* src, const long long* perm, void* dst, int T, int N, int Nsel, size_t row_bytes, m2h_stream stream) {
  M2H_REQUIRE(src && perm && dst && T > 0 && N > 0 && Nsel > 0 && row_bytes > 0 && row_bytes % 4 == 0, "gather_envs: bad arguments (row_bytes %% 4)");
  const size_t Lw = row_bytes / 4;
  M2H_LAUNCH(gather_envs_kernel, dim3(grid_for((size_t)T * Nsel * ((Lw & 3) ? Lw : Lw / 4), 8192)), dim3(256), 0, as_stream(stream),
                     static_cast<const uint32_t*>(src), perm, static_cast<uint32_t*>(dst), T, N, Nsel, Lw);
  return launch_status("gather_envs");
}

int m2h_episode_stats_update(const m2h_episode_stats* st, const float* rewards, const float* dist_probs, const float* bin_losses,
                             const float* mono_losses, const float* monoFromMem_losses, const float* not_done, const float* ndgs,
                             const float* dgs, int N, int A, m2h_stream stream) {
  M2H_REQUIRE(st && rewards && dist_probs && bin_losses && mono_losses && monoFromMem_losses && not_done && N > 0 && A > 0,
              "episode_stats_update: bad arguments");
  const float* const* fields = reinterpret_cast<const float* const*>(st);
  for (size_t i = 0; i < sizeof(m2h_episode_stats) / sizeof(float*); ++i) M2H_REQUIRE(fields[i], "episode_stats_update: null statistics tensor");
  M2H_LAUNCH(episode_stats_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), *st, rewards, dist_probs, bin_losses,
                     mono_losses, monoFromMem_losses, not_done, ndgs, dgs, N, A);
  return launch_status("episode_stats_update");
}

int m2h_rows_copy(const m2h_row_copy* items, int n_items, const long long* idx, m2h_stream stream) {
  M2H_REQUIRE(items && n_items > 0 && n_items <= M2H_ROWS_COPY_MAX, "rows_copy: 1..%d items", M2H_ROWS_COPY_MAX);
  RowsCopyArgs a;
  size_t big = 0;
  for (int i = 0; i < n_items; ++i) {
    const m2h_row_copy& it = items[i];
    M2H_REQUIRE(it.src && it.dst && it.bytes > 0 && it.bytes % 4 == 0, "rows_copy: item %d: null pointer or size not a multiple of 4", i);
    M2H_REQUIRE((it.src_slot < 0 && it.dst_slot < 0) || idx, "rows_copy: item %d uses a row index but idx is NULL", i);
    a.item[i] = it;
    big = it.bytes > big ? it.bytes : big;
  }
  const int gx = (int)((big / 16 + 255) / 256 > 256 ? 256 : ((big / 16 + 255) / 256 < 1 ? 1 : (big / 16 + 255) / 256));
  M2H_LAUNCH(rows_copy_kernel, dim3(gx, n_items), dim3(256), 0, as_stream(stream), a, idx);
  return launch_status("rows_copy");
}

int m2h_step_index_advance(long long* idx, int T_pol, int T_sep, m2h_stream stream) {
  M2H_REQUIRE(idx && T_pol > 0 && T_sep > 0, "step_index_advance: bad arguments");
  M2H_LAUNCH(step_index_advance_kernel, dim3(1), dim3(64), 0, as_stream(stream), idx, T_pol, T_sep);
  return launch_status("step_index_advance");
}

int m2h_step_index_advance_rng(long long* idx, int T_pol, int T_sep, unsigned long long* rng_state, unsigned long long rng_inc, m2h_stream stream) {
  M2H_REQUIRE(idx && T_pol > 0 && T_sep > 0 && rng_state, "step_index_advance_rng: bad arguments");
  M2H_LAUNCH(step_index_advance_kernel, dim3(1), dim3(64), 0, as_stream(stream), idx, T_pol, T_sep, rng_state, rng_inc);
  return launch_status("step_index_advance");
}

int m2h_synth_env_step(const long long* actions, long long* node, long long* angle, int n_nodes, int N, m2h_stream stream) {
  M2H_REQUIRE(actions && node && angle && n_nodes > 0 && N > 0, "synth_env_step: bad arguments");
  M2H_LAUNCH(synth_env_step_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), actions, node, angle, n_nodes, N);
  return launch_status("synth_env_step");
}

int m2h_synth_env_observe(const m2h_row_copy* items, int n_items, const long long* node, const long long* angle, const long long* audio_idx,
                          int N, m2h_stream stream) {
  M2H_REQUIRE(items && n_items > 0 && n_items <= M2H_ROWS_COPY_MAX && node && angle && audio_idx && N > 0, "synth_env_observe: bad arguments");
  RowsGatherArgs a;
  size_t big = 0;
  for (int i = 0; i < n_items; ++i) {
    M2H_REQUIRE(items[i].src && items[i].dst && items[i].bytes > 0 && items[i].bytes % 4 == 0 && (items[i].src_slot == 0 || items[i].src_slot == 1),
                "synth_env_observe: item %d: null pointer, size not a multiple of 4, or index selector not in {0, 1}", i);
    a.item[i] = items[i];
    big = items[i].bytes > big ? items[i].bytes : big;
  }
  size_t gx = (big / 16 + 255) / 256;
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  M2H_LAUNCH(rows_gather_kernel, dim3((unsigned)gx, (unsigned)N, (unsigned)n_items), dim3(256), 0, as_stream(stream), a, node, angle, audio_idx);
  return launch_status("synth_env_observe");
}

}  // extern "C"
