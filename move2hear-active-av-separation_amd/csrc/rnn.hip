// Recurrent cells of the RL path (gfx950), fp32: the GRU cell forward and backward, the LSTM cell forward and backward.
//   gru_gates / gru_step / gru_cell          : GRU cell pointwise part, hidden mask fused  (rnn_state_encoder.py:74-84)
//   gru_gates_bwd / gru_bwd_rec / _combine   : its backward, one BPTT step
//   lstm_cell / lstm_cell_bwd                : the rnn_type = "LSTM" variant               (rnn_state_encoder.py:10-34,49-69)
// The GRU gate arithmetic is written ONCE, as gru_gate / gru_gate_fwd / gru_gate_bwd below: the three forward kernels and the two
// backward kernels must agree to the bit (the backward recomputes the forward's gates), so none of them spells it out itself.
#include "rl_common.h"

namespace m2h {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// One hidden unit's GRU gates (order r, z, n).  gi = x W_ih^T + b_ih;  gh = h W_hh^T of the UNMASKED state, no bias;  b = b_hh;
// m = the row's hidden mask in {0,1}: (h*m) W^T = m * (h W^T), so the mask is applied here, to gh and to the carried state, never to gi,
// and b_hn stays INSIDE the r (...) product.
// The operands come by ADDRESS, gate by gate (GruIn): an operand that lives in memory is then loaded where the expression uses it, in
// the order the expressions use them, as a kernel that spells the gates out itself does.  By value or by reference the compiler
// hoists the loads of gru_gates_kernel and contracts m * gh_n + b_hn differently (a last-bit change, profiles/rl_split_isa.txt); for
// operands in registers (&local) the three forms compile alike.
struct GruIn {
  const float *gi_r, *gh_r, *b_r, *gi_z, *gh_z, *b_z, *gi_n, *gh_n, *b_n, *m, *hprev;   // hprev: the UNMASKED previous state
};
struct GruGate {
  float r, z, hn, n, hp;   // hn = m * gh_n + b_hn (the factor of r), hp = m * hprev (the masked previous state)
};
__device__ __forceinline__ GruGate gru_gate(const GruIn& in) {
  GruGate g;
  g.r = sigmoidf_(*in.gi_r + (*in.m * *in.gh_r + *in.b_r));
  g.z = sigmoidf_(*in.gi_z + (*in.m * *in.gh_z + *in.b_z));
  g.hn = *in.m * *in.gh_n + *in.b_n;
  g.n = tanhf(*in.gi_n + g.r * g.hn);
  g.hp = *in.m * *in.hprev;
  return g;
}

// -> the new state h' = (1 - z) n + z (m hprev)
__device__ __forceinline__ float gru_gate_fwd(const GruIn& in) {
  const GruGate g = gru_gate(in);
  return (1.f - g.z) * g.n + g.z * g.hp;
}

// Its backward for dh = dL/dh':  dar, daz, dan = dL/d(gi) per gate (= dL/d(m * gh + b_hh) for r and z);  hp = m * hprev (the A operand of the
// W_hh weight gradient).  r and z go back with them: the caller forms dan * r = dL/d(m * gh_n + b_hn) and dh * z (the direct path to the
// masked previous state) in the statements that store them, where the kernels always formed them (gru_bwd_rec_kernel's epilogue keeps its
// instruction order that way).
struct GruGateGrad {
  float dar, daz, dan, r, z, hp;
};
__device__ __forceinline__ GruGateGrad gru_gate_bwd(const GruIn& in, const float* dh) {
  const GruGate g = gru_gate(in);
  const float gd = *dh;
  const float dn = gd * (1.f - g.z);
  const float dz = gd * (g.hp - g.n);
  GruGateGrad d;
  d.dan = dn * (1.f - g.n * g.n);
  const float dr = d.dan * g.hn;
  d.daz = dz * g.z * (1.f - g.z);
  d.dar = dr * g.r * (1.f - g.r);
  d.r = g.r;
  d.z = g.z;
  d.hp = g.hp;
  return d;
}

// GRU cell pointwise part.  gi = x W_ih^T + b_ih  [M,3H];  gh_raw = h W_hh^T (no bias, UNMASKED h)  [M,3H];  mask m[row] in {0,1}.
__global__ __launch_bounds__(256) void gru_gates_kernel(const float* __restrict__ gi, const float* __restrict__ gh_raw,
                                                        const float* __restrict__ bhh, const float* __restrict__ hprev,
                                                        const float* __restrict__ mask, float* __restrict__ hout, int M, int H) {
  const int total = M * H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int row = i / H, j = i - row * H;
    const float m = mask != nullptr ? mask[row] : 1.f;
    const float* gir = gi + (size_t)row * 3 * H;
    const float* ghr = gh_raw + (size_t)row * 3 * H;
    hout[i] = gru_gate_fwd({&gir[j], &ghr[j], &bhh[j], &gir[H + j], &ghr[H + j], &bhh[H + j], &gir[2 * H + j], &ghr[2 * H + j], &bhh[2 * H + j], &m, &hprev[i]});
  }
}

// Skinny dot products on the matrix pipe: D[m][r] = sum_k X[m][k] * Wr[k] for 16 rows m of X and 16 weight rows r, both operands
// straight from global memory into v_mfma_f32_16x16x4_f32 registers (lane (row i, k-quarter kq) loads 16 bytes of its row = four
// consecutive MFMAs' worth; no LDS staging, no barrier in the k-loop).  The block's NW waves split the K/16 steps (a block's latency is
// its longest wave's chain of dependent loads: 16 waves quarter it against 4 for the long-K products); the caller
// sums their partial tiles through LDS in a fixed order (wave_tile_sum).  Returns acc[e] = D[m = kq*4 + e][r = i] over this wave's steps.
template <int NW = 4>
__device__ __forceinline__ f32x4 skinny_dot16(const float* __restrict__ xrow, const float* __restrict__ wrow, int steps, int wave) {
  const int s0 = (steps * wave) / NW, s1 = (steps * (wave + 1)) / NW;   // the block's NW waves split the K / 16 steps
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = s0; s < s1; ++s) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(xrow + 16 * s);
    const f32x4 b = *reinterpret_cast<const f32x4*>(wrow + 16 * s);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
  }
  return acc;
}

// sum over the NW waves' partial tiles, pairwise in a fixed tree (bit-reproducible)
template <int NW>
__device__ __forceinline__ float wave_tile_sum(const float (*R)[16][17], int m, int r) {
  float t[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) t[w] = R[w][m][r];
#pragma unroll
  for (int n = NW; n > 1; n >>= 1)
#pragma unroll
    for (int w = 0; w < n / 2; ++w) t[w] = t[2 * w] + t[2 * w + 1];
  return t[0];
}

// One GRU time step for a handful of rows (M <= 16: the rollout's 14 envs, one step of the update's sequence pass) in ONE
// launch: recurrent product gh_raw = h W_hh^T and the gate math of gru_gates_kernel.  At this size the product is a weight
// stream (3H x H floats, 3 MB at H = 512) against 14 rows: a tiled-GEMM launch + its split-K reduce + the gate kernel spend
// ~29 us on it, almost all launch and pipeline latency.  A block owns GRU_U hidden units = 3*GRU_U weight rows (r, z, n) and
// runs their dot products with the 16 state rows through skinny_dot16; the three gates of a unit meet through LDS.  gh_raw is
// written too (the backward pass reads it).  (First version: weights and state staged in LDS, one thread per (row, env) dot
// product with broadcast LDS reads -- 12 us, bound by LDS bandwidth.)
constexpr int GRU_U = 4;     // hidden units per block
constexpr int GRU_E = 16;    // env slots per block (M <= 16)
constexpr int GS_NW = 8;     // waves per block: the 32 steps of the H-long products are 4 per wave
__global__ __launch_bounds__(64 * GS_NW) void gru_step_kernel(const float* __restrict__ gi, const float* __restrict__ whh,
                                                       const float* __restrict__ bhh, const float* __restrict__ hprev,
                                                       const float* __restrict__ mask, float* __restrict__ gh_raw,
                                                       float* __restrict__ hout, int M, int H) {
  __shared__ float R[GS_NW][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int j0 = blockIdx.x * GRU_U;
  const int r = min(i, 3 * GRU_U - 1);                         // weight row of this lane: gate r / GRU_U, unit r % GRU_U
  const float* wrow = whh + ((size_t)(r / GRU_U) * H + j0 + (r % GRU_U)) * H + 4 * kq;
  const float* xrow = hprev + (size_t)min(i, M - 1) * H + 4 * kq;
  // gate inputs of this thread's (unit, env) pair, fetched before the dot products
  const int gu = (tid >> 4) & (GRU_U - 1), ge = min(tid & 15, M - 1), gj = j0 + gu;
  const float gmask = mask != nullptr ? mask[ge] : 1.f;
  const float gi_r = gi[(size_t)ge * 3 * H + gj], gi_z = gi[(size_t)ge * 3 * H + H + gj], gi_n = gi[(size_t)ge * 3 * H + 2 * H + gj];
  const float b_r = bhh[gj], b_z = bhh[H + gj], b_n = bhh[2 * H + gj];
  const float hp_raw = hprev[(size_t)ge * H + gj];
  const f32x4 acc = skinny_dot16<GS_NW>(xrow, wrow, H >> 4, wave);
#pragma unroll
  for (int e = 0; e < 4; ++e) R[wave][kq * 4 + e][i] = acc[e];   // [m][weight row]
  __syncthreads();
  if (tid < 3 * GRU_U * GRU_E) {                                  // gh_raw: thread (weight row rr, env m)
    const int rr = tid >> 4, m = tid & 15;
    if (m < M) gh_raw[(size_t)m * 3 * H + (size_t)(rr / GRU_U) * H + j0 + (rr % GRU_U)] = wave_tile_sum<GS_NW>(R, m, rr);
  }
  if (tid < GRU_U * GRU_E && (tid & 15) < M) {
    const int u = tid >> 4, m = tid & 15;
    auto tot = [&](int rr) { return wave_tile_sum<GS_NW>(R, m, rr); };
    const float gr = tot(u), gz = tot(GRU_U + u), gn = tot(2 * GRU_U + u);
    hout[(size_t)m * H + j0 + u] = gru_gate_fwd({&gi_r, &gr, &b_r, &gi_z, &gz, &b_z, &gi_n, &gn, &b_n, &gmask, &hp_raw});
  }
}

// The whole GRU cell of a no-grad single step (rnn_state_encoder.py:74-84 at the rollout width, M <= 16 rows) in ONE launch: the input
// projection gi = x W_ih^T + b_ih is the same kind of weight stream as the recurrent product (3H x I floats, 9.4 MB at I = 1536),
// so the block that owns GRU_U hidden units runs the dot products of its 3*GRU_U rows of BOTH matrices through skinny_dot16 and
// applies the gates; nothing but the new state is written (no backward pass follows a no-grad step).  Replaces the projection GEMM +
// gru_step_kernel of the rollout step.
constexpr int GC_NW = 16;    // waves per block of gru_cell_kernel: the 96 + 32 steps of the two products are 8 per wave
__global__ __launch_bounds__(64 * GC_NW) void gru_cell_kernel(const float* __restrict__ x, const float* __restrict__ wih, const float* __restrict__ bih,
                                                       const float* __restrict__ whh, const float* __restrict__ bhh,
                                                       const float* __restrict__ hprev, const float* __restrict__ mask,
                                                       float* __restrict__ hout, int M, int I, int H) {
  __shared__ float R[2][GC_NW][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int j0 = blockIdx.x * GRU_U;
  const int r = min(i, 3 * GRU_U - 1);                         // weight row of this lane: gate r / GRU_U, unit r % GRU_U
  const size_t wr = (size_t)(r / GRU_U) * H + j0 + (r % GRU_U);
  const int row = min(i, M - 1);
  const int gu = (tid >> 4) & (GRU_U - 1), ge = min(tid & 15, M - 1), gj = j0 + gu;
  const float gmask = mask != nullptr ? mask[ge] : 1.f;
  const float bi_r = bih[gj], bi_z = bih[H + gj], bi_n = bih[2 * H + gj];
  const float b_r = bhh[gj], b_z = bhh[H + gj], b_n = bhh[2 * H + gj];
  const float hp_raw = hprev[(size_t)ge * H + gj];
  const f32x4 ai = skinny_dot16<GC_NW>(x + (size_t)row * I + 4 * kq, wih + wr * I + 4 * kq, I >> 4, wave);
  const f32x4 ah = skinny_dot16<GC_NW>(hprev + (size_t)row * H + 4 * kq, whh + wr * H + 4 * kq, H >> 4, wave);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    R[0][wave][kq * 4 + e][i] = ai[e];   // [m][weight row]
    R[1][wave][kq * 4 + e][i] = ah[e];
  }
  __syncthreads();
  if (tid < GRU_U * GRU_E && (tid & 15) < M) {
    const int u = tid >> 4, m = tid & 15;
    auto tot = [&](int w, int rr) { return wave_tile_sum<GC_NW>(R[w], m, rr); };
    const float gi_r = tot(0, u) + bi_r, gi_z = tot(0, GRU_U + u) + bi_z, gi_n = tot(0, 2 * GRU_U + u) + bi_n;
    const float gr = tot(1, u), gz = tot(1, GRU_U + u), gn = tot(1, 2 * GRU_U + u);
    hout[(size_t)m * H + j0 + u] = gru_gate_fwd({&gi_r, &gr, &b_r, &gi_z, &gz, &b_z, &gi_n, &gn, &b_n, &gmask, &hp_raw});
  }
}

// LSTM cell, pointwise part (the class's rnn_type = "LSTM" variant, rnn_state_encoder.py:10-34,49-69; nn.LSTM's gate order i, f, g, o):
// pre = gi + gh  [M][4H] (gi = x W_ih^T + b_ih, gh = (h m) W_hh^T + b_hh);  c' = sigma(f) (c m) + sigma(i) tanh(g);  h' = sigma(o) tanh(c').
// The reset mask m[row] multiplies the carried cell state here (the hidden state's mask is applied before its product: _mask_hidden, :63-69).
// gates_out [M][4H] keeps the ACTIVATED gates for the backward.  One thread per (row, unit).
__global__ __launch_bounds__(256) void lstm_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ cprev,
                                                        const float* __restrict__ mask, float* __restrict__ hout, float* __restrict__ cout,
                                                        float* __restrict__ gates_out, int M, int H) {
  const size_t total = (size_t)M * H;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(idx / H), j = (int)(idx - (size_t)row * H);
    const size_t b = (size_t)row * 4 * H;
    const float ig = sigmoidf_(gi[b + j] + gh[b + j]);
    const float fg = sigmoidf_(gi[b + H + j] + gh[b + H + j]);
    const float gg = tanhf(gi[b + 2 * H + j] + gh[b + 2 * H + j]);
    const float og = sigmoidf_(gi[b + 3 * H + j] + gh[b + 3 * H + j]);
    const float cm = cprev[idx] * mask[row];
    const float c = fg * cm + ig * gg;
    cout[idx] = c;
    hout[idx] = og * tanhf(c);
    if (gates_out != nullptr) {
      gates_out[b + j] = ig;
      gates_out[b + H + j] = fg;
      gates_out[b + 2 * H + j] = gg;
      gates_out[b + 3 * H + j] = og;
    }
  }
}

// Its backward: dh, dc = gradients of (h', c'); dpre [M][4H] = gradient of the pre-activations (of gi and gh alike), dcprev = gradient of the
// carried cell state (through the mask).  dh or dc may be NULL (zero).
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ dc, const float* __restrict__ gates,
                                                            const float* __restrict__ cprev, const float* __restrict__ mask, const float* __restrict__ c,
                                                            float* __restrict__ dpre, float* __restrict__ dcprev, int M, int H) {
  const size_t total = (size_t)M * H;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(idx / H), j = (int)(idx - (size_t)row * H);
    const size_t b = (size_t)row * 4 * H;
    const float ig = gates[b + j], fg = gates[b + H + j], gg = gates[b + 2 * H + j], og = gates[b + 3 * H + j];
    const float m = mask[row];
    const float tc = tanhf(c[idx]);
    const float gh_ = dh != nullptr ? dh[idx] : 0.f;
    const float dct = (dc != nullptr ? dc[idx] : 0.f) + gh_ * og * (1.f - tc * tc);
    dpre[b + j] = dct * gg * ig * (1.f - ig);
    dpre[b + H + j] = dct * (cprev[idx] * m) * fg * (1.f - fg);
    dpre[b + 2 * H + j] = dct * ig * (1.f - gg * gg);
    dpre[b + 3 * H + j] = gh_ * tc * og * (1.f - og);
    dcprev[idx] = dct * fg * m;
  }
}

// Backward of gru_gates_kernel for one time step.  Inputs as the forward plus dh = dL/dh_out.  Outputs:
//   dgi  [M,3H] = dL/d(x W_ih^T + b_ih)           dpre [M,3H] = dL/d(m * gh_raw + b_hh)  (so dL/dgh_raw = m * dpre)
//   dhp  [M,H]  = dh * z  (direct path to the masked previous hidden state; caller applies the mask)
//   hpm  [M,H]  = m * hprev  (masked previous hidden state, the A operand of the W_hh weight gradient)
__global__ __launch_bounds__(256) void gru_gates_bwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh_raw,
                                                            const float* __restrict__ bhh, const float* __restrict__ hprev,
                                                            const float* __restrict__ mask, const float* __restrict__ dh,
                                                            float* __restrict__ dgi, float* __restrict__ dpre, float* __restrict__ dhp,
                                                            float* __restrict__ hpm, int M, int H) {
  const int total = M * H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int row = i / H, j = i - row * H;
    const float m = mask != nullptr ? mask[row] : 1.f;
    const size_t o = (size_t)row * 3 * H;
    const GruGateGrad d = gru_gate_bwd({&gi[o + j], &gh_raw[o + j], &bhh[j], &gi[o + H + j], &gh_raw[o + H + j], &bhh[H + j], &gi[o + 2 * H + j],
                                        &gh_raw[o + 2 * H + j], &bhh[2 * H + j], &m, &hprev[i]}, &dh[i]);
    dgi[o + j] = d.dar;
    dgi[o + H + j] = d.daz;
    dgi[o + 2 * H + j] = d.dan;
    dpre[o + j] = d.dar;
    dpre[o + H + j] = d.daz;
    dpre[o + 2 * H + j] = d.dan * d.r;
    dhp[i] = dh[i] * d.z;
    hpm[i] = d.hp;
  }
}

// out = a + mask_row * (b + c): total gradient of h_{t-1} = output-path gradient + masked recurrent-path gradient
__global__ void gru_bwd_combine_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                       const float* __restrict__ mask, float* __restrict__ out, int M, int H) {
  const int total = M * H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const float m = mask != nullptr ? mask[i / H] : 1.f;
    out[i] = (a != nullptr ? a[i] : 0.f) + m * (b[i] + c[i]);
  }
}

// Recurrent part of one GRU backward step for M <= 16 rows in one launch: out = a + mask * (dpre W_hh + dhp), i.e. the
// [M,3H] x [3H,H] product (a 3 MB weight stream against 14 rows) and m2h_gru_bwd_combine.  A block owns GB_U hidden units = GB_U rows
// of W_hh^T and runs their 3H-long dot products with the 16 rows of dpre through skinny_dot16 (the 16-wide tile's other columns
// repeat the last row); the four waves' partial tiles meet through LDS in wave order.
constexpr int GB_U = 4, GB_E = 16;
// With the *_p arguments (gi_p != nullptr) the gate backward of the PREVIOUS time step (gru_gates_bwd_kernel over this block's
// columns: it is elementwise in (row, hidden unit), and its dh is exactly the out element the thread has just produced) runs as this
// kernel's epilogue: one launch per BPTT step instead of two.  dhp is read (this step's) and rewritten (the previous step's) by the
// same thread at the same element.
constexpr int GB_NW = 16;    // waves per block: the 96 steps of the 3H-long products are 6 per wave (four waves: 24 -- 9.7 us per BPTT step)
__global__ __launch_bounds__(64 * GB_NW) void gru_bwd_rec_kernel(const float* __restrict__ dpre, const float* __restrict__ whh_t,
                                                          const float* __restrict__ a, float* __restrict__ dhp,
                                                          const float* __restrict__ mask, float* __restrict__ out, int M, int H,
                                                          const float* __restrict__ gi_p = nullptr, const float* __restrict__ gh_p = nullptr,
                                                          const float* __restrict__ bhh = nullptr, const float* __restrict__ hprev_p = nullptr,
                                                          const float* __restrict__ mask_p = nullptr, float* __restrict__ dgi_p = nullptr,
                                                          float* __restrict__ dpre_p = nullptr, float* __restrict__ hpm_p = nullptr) {
  __shared__ float R[GB_NW][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int j0 = blockIdx.x * GB_U, K = 3 * H;
  const float* wrow = whh_t + (size_t)(j0 + min(i, GB_U - 1)) * K + 4 * kq;
  const float* xrow = dpre + (size_t)min(i, M - 1) * K + 4 * kq;
  // the epilogue's operands of this thread's (unit, row) pair, fetched before the dot products (as gru_step_kernel does): behind the
  // barrier they were a second dependent round trip in every one of the 20 BPTT steps
  const bool epi = tid < GB_U * GB_E && (tid & 15) < M;
  const int eu = (tid >> 4) & (GB_U - 1), em = min(tid & 15, M - 1), ej = j0 + eu;
  const size_t eo = (size_t)em * H + ej, eo3 = (size_t)em * 3 * H;
  const float e_mk = mask != nullptr ? mask[em] : 1.f;
  const float e_a = (epi && a != nullptr) ? a[eo] : 0.f;
  const float e_dhp = epi ? dhp[eo] : 0.f;
  float e_mp = 1.f, e_gir = 0.f, e_giz = 0.f, e_gin = 0.f, e_ghr = 0.f, e_ghz = 0.f, e_ghn = 0.f, e_br = 0.f, e_bz = 0.f, e_bn = 0.f, e_hp = 0.f;
  if (gi_p != nullptr && epi) {
    e_mp = mask_p != nullptr ? mask_p[em] : 1.f;
    e_gir = gi_p[eo3 + ej]; e_giz = gi_p[eo3 + H + ej]; e_gin = gi_p[eo3 + 2 * H + ej];
    e_ghr = gh_p[eo3 + ej]; e_ghz = gh_p[eo3 + H + ej]; e_ghn = gh_p[eo3 + 2 * H + ej];
    e_br = bhh[ej]; e_bz = bhh[H + ej]; e_bn = bhh[2 * H + ej];
    e_hp = hprev_p[eo];
  }
  const f32x4 acc = skinny_dot16<GB_NW>(xrow, wrow, K >> 4, wave);
#pragma unroll
  for (int e = 0; e < 4; ++e) R[wave][kq * 4 + e][i] = acc[e];
  __syncthreads();
  if (epi) {
    const int u = tid >> 4, m = tid & 15;
    const float rec = wave_tile_sum<GB_NW>(R, m, u);
    const size_t o = (size_t)m * H + j0 + u;
    const float g = e_a + e_mk * (rec + e_dhp);
    out[o] = g;
    if (gi_p != nullptr) {                 // gru_gates_bwd_kernel of the previous step at (row m, unit j), dh = g
      const int j = j0 + u;
      const size_t o3 = (size_t)m * 3 * H;
      const GruGateGrad d = gru_gate_bwd({&e_gir, &e_ghr, &e_br, &e_giz, &e_ghz, &e_bz, &e_gin, &e_ghn, &e_bn, &e_mp, &e_hp}, &g);
      dgi_p[o3 + j] = d.dar;
      dgi_p[o3 + H + j] = d.daz;
      dgi_p[o3 + 2 * H + j] = d.dan;
      dpre_p[o3 + j] = d.dar;
      dpre_p[o3 + H + j] = d.daz;
      dpre_p[o3 + 2 * H + j] = d.dan * d.r;
      dhp[o] = g * d.z;
      hpm_p[o] = d.hp;
    }
  }
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_gru_gates(const float* gi, const float* gh_raw, const float* bhh, const float* hprev, const float* mask, float* hout,
                  int M, int H, m2h_stream stream) {
  M2H_REQUIRE(gi && gh_raw && bhh && hprev && hout && M > 0 && H > 0, "gru_gates: bad arguments");
  M2H_LAUNCH(gru_gates_kernel, dim3(grid_for((size_t)M * H)), dim3(256), 0, as_stream(stream), gi, gh_raw, bhh, hprev, mask, hout, M, H);
  return launch_status("gru_gates");
}

int m2h_gru_step(const float* gi, const float* whh, const float* bhh, const float* hprev, const float* mask, float* gh_raw, float* hout,
                 int M, int H, m2h_stream stream) {
  M2H_REQUIRE(gi && whh && bhh && hprev && gh_raw && hout, "gru_step: null pointer");
  M2H_REQUIRE(M > 0 && M <= GRU_E && H > 0 && H % 16 == 0, "gru_step: needs 1 <= M <= %d rows and H %% 16 == 0 (got M=%d, H=%d)",
              GRU_E, M, H);
  M2H_LAUNCH(gru_step_kernel, dim3(H / GRU_U), dim3(64 * GS_NW), 0, as_stream(stream), gi, whh, bhh, hprev, mask, gh_raw, hout, M, H);
  return launch_status("gru_step");
}

int m2h_gru_cell(const float* x, const float* wih, const float* bih, const float* whh, const float* bhh, const float* hprev,
                 const float* mask, float* hout, int M, int I, int H, m2h_stream stream) {
  M2H_REQUIRE(x && wih && bih && whh && bhh && hprev && hout, "gru_cell: null pointer");
  M2H_REQUIRE(M > 0 && M <= GRU_E && H > 0 && H % 16 == 0 && I > 0 && I % 16 == 0,
              "gru_cell: needs 1 <= M <= %d rows, H %% 16 == 0 and I %% 16 == 0 (got M=%d, I=%d, H=%d)", GRU_E, M, I, H);
  M2H_LAUNCH(gru_cell_kernel, dim3(H / GRU_U), dim3(64 * GC_NW), 0, as_stream(stream), x, wih, bih, whh, bhh, hprev, mask, hout, M, I, H);
  return launch_status("gru_cell");
}

int m2h_lstm_cell(const float* gi, const float* gh, const float* c_prev, const float* mask, float* h_out, float* c_out, float* gates_out, int M, int H,
                  m2h_stream stream) {
  M2H_REQUIRE(gi && gh && c_prev && mask && h_out && c_out && M > 0 && H > 0, "lstm_cell: bad arguments");
  M2H_LAUNCH(lstm_cell_kernel, dim3(grid_for((size_t)M * H)), dim3(256), 0, as_stream(stream), gi, gh, c_prev, mask, h_out, c_out, gates_out, M, H);
  return launch_status("lstm_cell");
}

int m2h_lstm_cell_bwd(const float* dh, const float* dc, const float* gates, const float* c_prev, const float* mask, const float* c, float* dpre,
                      float* dc_prev, int M, int H, m2h_stream stream) {
  M2H_REQUIRE(gates && c_prev && mask && c && dpre && dc_prev && M > 0 && H > 0, "lstm_cell_bwd: bad arguments");
  M2H_LAUNCH(lstm_cell_bwd_kernel, dim3(grid_for((size_t)M * H)), dim3(256), 0, as_stream(stream), dh, dc, gates, c_prev, mask, c, dpre, dc_prev, M, H);
  return launch_status("lstm_cell_bwd");
}

int m2h_gru_gates_bwd(const float* gi, const float* gh_raw, const float* bhh, const float* hprev, const float* mask, const float* dh,
                      float* dgi, float* dpre, float* dhp, float* hpm, int M, int H, m2h_stream stream) {
  M2H_REQUIRE(gi && gh_raw && bhh && hprev && dh && dgi && dpre && dhp && hpm && M > 0 && H > 0, "gru_gates_bwd: bad arguments");
  M2H_LAUNCH(gru_gates_bwd_kernel, dim3(grid_for((size_t)M * H)), dim3(256), 0, as_stream(stream), gi, gh_raw, bhh, hprev, mask, dh,
                     dgi, dpre, dhp, hpm, M, H);
  return launch_status("gru_gates_bwd");
}

int m2h_gru_bwd_combine(const float* a, const float* b, const float* c, const float* mask, float* out, int M, int H, m2h_stream stream) {
  M2H_REQUIRE(b && c && out && M > 0 && H > 0, "gru_bwd_combine: bad arguments");
  M2H_LAUNCH(gru_bwd_combine_kernel, dim3(grid_for((size_t)M * H)), dim3(256), 0, as_stream(stream), a, b, c, mask, out, M, H);
  return launch_status("gru_bwd_combine");
}

int m2h_gru_bwd_rec(const float* dpre, const float* whh_t, const float* a, const float* dhp, const float* mask, float* out, int M, int H,
                    m2h_stream stream) {
  M2H_REQUIRE(dpre && whh_t && dhp && out, "gru_bwd_rec: null pointer");
  M2H_REQUIRE(M > 0 && M <= GB_E && H > 0 && H % 16 == 0, "gru_bwd_rec: needs 1 <= M <= %d rows and H %% 16 == 0 (got M=%d, H=%d)",
              GB_E, M, H);
  M2H_LAUNCH(gru_bwd_rec_kernel, dim3(H / GB_U), dim3(64 * GB_NW), 0, as_stream(stream), dpre, whh_t, a, const_cast<float*>(dhp), mask, out, M, H,
                     static_cast<const float*>(nullptr), static_cast<const float*>(nullptr), static_cast<const float*>(nullptr),
                     static_cast<const float*>(nullptr), static_cast<const float*>(nullptr), static_cast<float*>(nullptr),
                     static_cast<float*>(nullptr), static_cast<float*>(nullptr));
  return launch_status("gru_bwd_rec");
}

int m2h_gru_bwd_step(const float* dpre, const float* whh_t, const float* a, float* dhp, const float* mask, float* out, const float* gi_prev,
                     const float* gh_prev, const float* bhh, const float* hprev_prev, const float* mask_prev, float* dgi_prev, float* dpre_prev,
                     float* hpm_prev, int M, int H, m2h_stream stream) {
  M2H_REQUIRE(dpre && whh_t && dhp && out && gi_prev && gh_prev && bhh && hprev_prev && dgi_prev && dpre_prev && hpm_prev, "gru_bwd_step: null pointer");
  M2H_REQUIRE(M > 0 && M <= GB_E && H > 0 && H % 16 == 0, "gru_bwd_step: needs 1 <= M <= %d rows and H %% 16 == 0 (got M=%d, H=%d)",
              GB_E, M, H);
  M2H_REQUIRE(dpre_prev != dpre, "gru_bwd_step: the previous step's dpre must not alias this step's (every block reads all of it)");
  M2H_LAUNCH(gru_bwd_rec_kernel, dim3(H / GB_U), dim3(64 * GB_NW), 0, as_stream(stream), dpre, whh_t, a, dhp, mask, out, M, H, gi_prev, gh_prev, bhh,
                     hprev_prev, mask_prev, dgi_prev, dpre_prev, hpm_prev);
  return launch_status("gru_bwd_step");
}

}  // extern "C"
