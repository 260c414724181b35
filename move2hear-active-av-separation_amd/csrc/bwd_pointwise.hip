// Pointwise backward pieces beside the weight gradient (gfx950):
//   pack_dgrad_weight   the input gradient of a stride-s conv runs on the FORWARD engines (conv_dispatch.hip) as s*s sub-pixel phase
//                       convolutions of dY with the (ci <-> co)-transposed, tap-strided weights; m2h_pack_dgrad_weight lays those out
//   unpack_convT_wgrad  per-phase packed gradients of a transposed conv -> its torch layout
//   act_bwd             dY * (y > 0 ? 1 : slope)  for the fused ReLU / LeakyReLU epilogues;  bias_grad = column sums of dY
#include "m2h_internal.h"

namespace m2h {

// w [Co][Ci][KH][KW] -> per phase (ph,pw) of the stride: wp[phase][ci][th][tw][co] = w[co][ci][kh0(ph)+s*th][kw0(pw)+s*tw],
// kh0(ph) = (ph + pad) % s.  Requires KH % s == 0, KW % s == 0.  The matching launch: N = Ci, taps (KH/s, KW/s), mul = -1,
// off = (ph + pad - kh0)/s, stride 1, output step s, phase (ph,pw).
__global__ void pack_dgrad_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, int Co, int Ci, int KH, int KW, int s, int pad) {
  const int th_n = KH / s, tw_n = KW / s;
  const size_t per_phase = (size_t)Ci * th_n * tw_n * Co;
  const size_t total = per_phase * s * s;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Co);
    size_t r = i / Co;
    const int tw = (int)(r % tw_n);
    r /= tw_n;
    const int th = (int)(r % th_n);
    r /= th_n;
    const int ci = (int)(r % Ci);
    const int phase = (int)(r / Ci);
    const int ph = phase / s, pw = phase % s;
    const int kh = (ph + pad) % s + s * th, kw = (pw + pad) % s + s * tw;
    wp[i] = w[(((size_t)co * Ci + ci) * KH + kh) * KW + kw];
  }
}

// inverse of pack_convT_weight for gradients: dw[ci][co][kh][kw] = dwp[phase][co][th][tw][ci], kh = (ph ? 2 : 1) + th*(ph ? -2 : 2)
__global__ void unpack_convT_wgrad_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int Ci, int Co) {
  const size_t total = (size_t)16 * Co * Ci;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Ci);
    size_t r = i / Ci;
    const int tw = (int)(r & 1);
    const int th = (int)((r >> 1) & 1);
    r >>= 2;
    const int co = (int)(r % Co);
    const int phase = (int)(r / Co);
    const int ph = phase >> 1, pw = phase & 1;
    const int kh = (ph ? 2 : 1) + th * (ph ? -2 : 2);
    const int kw = (pw ? 2 : 1) + tw * (pw ? -2 : 2);
    dw[(((size_t)ci * Co + co) * 4 + kh) * 4 + kw] = dwp[i];
  }
}

__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float slope, float* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = y[i] > 0.f ? dy[i] : dy[i] * slope;
}

// db[n] = sum_m dy[m][n].  Two ordered stages (deterministic): grid (column blocks of 64, row splits) -> part[split][n],
// then one thread per column sums the splits.  Lanes walk columns (coalesced 256-byte rows), the 4 waves stride the rows.
// GATE: m2h_act_bwd_bias -- the element is first passed through the activation's backward (y > 0 ? dy : dy * slope) and written to `out`: the
// same partition and summation order, so db has the bits of m2h_act_bwd followed by m2h_bias_grad, from one pass over dy instead of two.
// NW = waves per block = row lanes: 16 for the one-stage form (a few hundred rows on N / 64 blocks: with 4 waves a wave walked 70 of the update
// batch's 280 rows, nine dependent batches of loads -- 24-37 us for the encoders' 512-wide Linear layers on 8 blocks)
template <bool GATE, int NW = 4>
__global__ __launch_bounds__(64 * NW) void bias_grad_partial_kernel(const float* __restrict__ dy, float* __restrict__ part, int M, int N, int rows_per_split,
                                                                const float* __restrict__ y = nullptr, float slope = 1.f, float* __restrict__ out = nullptr) {
  __shared__ float sh[NW][64];
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  const int w = threadIdx.x >> 6;
  const int m0 = blockIdx.y * rows_per_split;
  const int m1 = min(M, m0 + rows_per_split);
  float s = 0.f;
  if (n < N) {
    // U rows' loads in flight before the first add (the sum keeps its order, row by row: same bits as the one-load-at-a-time loop, which
    // was a chain of dependent memory round trips -- 47-51 us for the update batch's 280 rows x 512 columns on 8 blocks)
    constexpr int U = 8;
    for (int m = m0 + w; m < m1; m += NW * U) {
      float v[U], g[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int mm = m + NW * u;
        v[u] = mm < m1 ? dy[(size_t)mm * N + n] : 0.f;
        if constexpr (GATE) g[u] = mm < m1 ? y[(size_t)mm * N + n] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int mm = m + NW * u;
        if (mm < m1) {
          float x = v[u];
          if constexpr (GATE) {
            x = g[u] > 0.f ? x : x * slope;
            out[(size_t)mm * N + n] = x;
          }
          s += x;
        }
      }
    }
  }
  sh[w][threadIdx.x & 63] = s;
  __syncthreads();
  if (w == 0 && n < N) {
    float r = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
#pragma unroll
    for (int k = 4; k < NW; ++k) r += sh[k][threadIdx.x];
    part[(size_t)blockIdx.y * N + n] = r;
  }
}

// The same partial sums for NARROW gradients (N in {1, 2, 4, 8, 16, 32}: the U-Net heads' 2 channels over a million pixels, the encoders'
// 32-channel convs): with lanes walking columns only N of 64 lanes work and a wave's load is an N-float run (the head's bias gradient
// took 82 us for 8 MB).  Here a wave reads 64 consecutive floats = 64 / N whole rows per step (lane l: row l / N, column l % N), four
// steps in flight, and the lanes of one column meet in a fixed xor butterfly; then the waves in order.
template <bool GATE>
__global__ __launch_bounds__(256) void bias_grad_partial_narrow_kernel(const float* __restrict__ dy, float* __restrict__ part, int M, int N,
                                                                       int rows_per_split, const float* __restrict__ y = nullptr, float slope = 1.f,
                                                                       float* __restrict__ out = nullptr) {
  __shared__ float sh[4][32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int RW = 64 / N;                                   // rows per wave step
  const int m0 = blockIdx.y * rows_per_split;
  const int m1 = min(M, m0 + rows_per_split);
  const size_t end = (size_t)m1 * N;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  size_t i = ((size_t)m0 + (size_t)w * RW) * N + lane;      // this lane's element; a block step is 4 waves x 64 floats
  auto gated = [&](size_t j, float v) {
    if constexpr (GATE) {
      v = y[j] > 0.f ? v : v * slope;
      out[j] = v;
    }
    return v;
  };
  for (; i + 3 * 256 < end; i += 4 * 256) {
    float a = dy[i], b = dy[i + 256], c = dy[i + 512], d = dy[i + 768];
    a = gated(i, a); b = gated(i + 256, b); c = gated(i + 512, c); d = gated(i + 768, d);
    s0 += a; s1 += b; s2 += c; s3 += d;
  }
  for (; i < end; i += 256) s0 += gated(i, dy[i]);
  float s = (s0 + s1) + (s2 + s3);
  for (int o = 32; o >= N; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane < N) sh[w][lane] = s;
  __syncthreads();
  if (w == 0 && lane < N) part[(size_t)blockIdx.y * N + lane] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

// one wave per column: lanes sum the splits strided by 64, then a fixed butterfly (deterministic)
__global__ __launch_bounds__(256) void bias_grad_final_kernel(const float* __restrict__ part, float* __restrict__ db, int N, int splits) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  float s = 0.f;
  for (int z = threadIdx.x & 63; z < splits; z += 64) s += part[(size_t)z * N + n];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) db[n] = s;
}

static int bias_grad_splits(int M, int N) {
  const int colblocks = (N + 63) / 64;
  int splits = (1024 + colblocks - 1) / colblocks;  // ~4 blocks per CU
  if (splits > (M + 63) / 64) splits = (M + 63) / 64;  // at least 64 rows per split
  if (splits < 1) splits = 1;
  if (M <= 1024) splits = 1;   // a few hundred rows (the update batch's Linear / GRU layers): one stage, straight into db -- no second launch
  return splits;
}

template <bool GATE>
static int bias_grad_launch(const float* dy, const float* y, float slope, float* out, float* db, int M, int N, float* workspace, hipStream_t st) {
  const int splits = bias_grad_splits(M, N);
  const int rps = (M + splits - 1) / splits;
  if (splits == 1) {   // the one split's "partial" IS the column sum
    if (M > 64) M2H_LAUNCH((bias_grad_partial_kernel<GATE, 16>), dim3((N + 63) / 64, 1), dim3(1024), 0, st, dy, db, M, N, rps, y, slope, out);
    else M2H_LAUNCH((bias_grad_partial_kernel<GATE, 4>), dim3((N + 63) / 64, 1), dim3(256), 0, st, dy, db, M, N, rps, y, slope, out);
    return launch_status(GATE ? "act_bwd_bias" : "bias_grad");
  }
  if (N <= 32 && 64 % N == 0) {   // narrow: splits of whole wave steps (64 / N rows); trailing splits may be empty (their partial is 0)
    const int rw = 64 / N, rps_n = (rps + rw - 1) / rw * rw;
    M2H_LAUNCH(bias_grad_partial_narrow_kernel<GATE>, dim3(1, splits), dim3(256), 0, st, dy, workspace, M, N, rps_n, y, slope, out);
  } else
    M2H_LAUNCH((bias_grad_partial_kernel<GATE, 4>), dim3((N + 63) / 64, splits), dim3(256), 0, st, dy, workspace, M, N, rps, y, slope, out);
  M2H_LAUNCH(bias_grad_final_kernel, dim3((N + 3) / 4), dim3(256), 0, st, workspace, db, N, splits);
  return launch_status(GATE ? "act_bwd_bias" : "bias_grad");
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_pack_dgrad_weight(const float* w, float* wp, int Co, int Ci, int KH, int KW, int stride, int pad, m2h_stream stream) {
  M2H_REQUIRE(w && wp && Co > 0 && Ci > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0, "pack_dgrad_weight: bad arguments");
  M2H_REQUIRE(KH % stride == 0 && KW % stride == 0, "pack_dgrad_weight: kernel size must be a multiple of the stride");
  const size_t total = (size_t)Co * Ci * KH * KW;
  size_t g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  M2H_LAUNCH(pack_dgrad_weight_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), w, wp, Co, Ci, KH, KW, stride, pad);
  return launch_status("pack_dgrad_weight");
}

int m2h_unpack_convT_wgrad(const float* dwp, float* dw, int Ci, int Co, m2h_stream stream) {
  M2H_REQUIRE(dwp && dw && Ci > 0 && Co > 0, "unpack_convT_wgrad: bad arguments");
  size_t g = ((size_t)16 * Co * Ci + 255) / 256;
  if (g > 2048) g = 2048;
  M2H_LAUNCH(unpack_convT_wgrad_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), dwp, dw, Ci, Co);
  return launch_status("unpack_convT_wgrad");
}

int m2h_act_bwd(const float* dy, const float* y, float slope, float* out, size_t n, m2h_stream stream) {
  M2H_REQUIRE(dy && y && out && n > 0, "act_bwd: bad arguments");
  size_t g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  M2H_LAUNCH(act_bwd_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), dy, y, slope, out, n);
  return launch_status("act_bwd");
}

size_t m2h_bias_grad_workspace_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)bias_grad_splits(M, N) * N * sizeof(float);
}

int m2h_bias_grad(const float* dy, float* db, int M, int N, float* workspace, m2h_stream stream) {
  M2H_REQUIRE(dy && db && workspace && M > 0 && N > 0, "bias_grad: bad arguments");
  return bias_grad_launch<false>(dy, nullptr, 1.f, nullptr, db, M, N, workspace, as_stream(stream));
}

int m2h_act_bwd_bias(const float* dy, const float* y, float slope, float* out, float* db, int M, int N, float* workspace, m2h_stream stream) {
  M2H_REQUIRE(dy && y && out && db && workspace && M > 0 && N > 0, "act_bwd_bias: bad arguments");
  M2H_REQUIRE((size_t)M * N < ((size_t)1 << 40), "act_bwd_bias: tensor too large");
  return bias_grad_launch<true>(dy, y, slope, out, db, M, N, workspace, as_stream(stream));
}

}  // extern "C"
