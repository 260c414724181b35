// Weight gradient, the ordered split sums (gfx950): slabs [split][N][Kpad] -> the gradient in the layout the caller asked for.
#include "wgrad_common.h"

namespace m2h {

// Sum of one slab element over the splits [z0, z1): eight running sums (eight loads in flight per lane), combined pairwise -- the ONE
// order of every many-split reduce below (wgrad_reduce_kernel and the fused re-layout kernels give the same bits).
__device__ __forceinline__ float wgrad_quarter_sum(const float* __restrict__ src, int z0, int z1, size_t zs) {
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int z = z0;
  for (; z + 7 < z1; z += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(z + j) * zs];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += v[j];
  }
  for (; z < z1; ++z) a[0] += src[(size_t)z * zs];
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// dw[n][k] = sum over splits, fixed order (packed layout; a quad launch ends in convT_wgrad_reduce_unpack_kernel instead).  A block owns 64 consecutive k of one row n; its four waves each sum a quarter of
// the splits (eight loads in flight per lane: wgrad_quarter_sum), then the quarters are combined in wave order.  (One thread per element walking
// all splits serially took 39 us for a 32 x 384 gradient with 512 splits: 36 blocks, one dependent load at a time.)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WGradP p) {
  __shared__ float sh[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int kb = (p.K + 63) / 64;
  const int n = blockIdx.x / kb;
  const int k = (blockIdx.x - n * kb) * 64 + lane;
  const int z0 = (int)(((long)p.S * w) / 4), z1 = (int)(((long)p.S * (w + 1)) / 4);
  const size_t zs = (size_t)p.N * p.Kpad;
  const float* src = k < p.K ? p.ws + (size_t)n * p.Kpad + k : nullptr;   // (nullptr: outside the tensor, as in wgrad_tile_sum)
  sh[w][lane] = src != nullptr ? wgrad_quarter_sum(src, z0, z1, zs) : 0.f;
  __syncthreads();
  if (w == 0 && k < p.K) p.dw[(size_t)n * p.K + k] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

// few splits: one thread per element (the block-per-64-k form above would be tens of thousands of near-empty blocks)
__global__ __launch_bounds__(256) void wgrad_reduce_small_kernel(const WGradP p) {
  const size_t total = (size_t)p.N * p.K, zs = (size_t)p.N * p.Kpad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / p.K);
    const int k = (int)(i - (size_t)n * p.K);
    const float* src = p.ws + (size_t)n * p.Kpad + k;
    float s = 0.f;
    for (int z = 0; z < p.S; ++z) s += src[(size_t)z * zs];
    p.dw[i] = s;
  }
}

// The split sum of a 16 x 16 tile of gradient elements, in the order (and so with the bits) of the reduce kernel the launch would
// otherwise take: S < 16 -> 256 threads, one running sum per element (wgrad_reduce_small_kernel); S >= 16 -> 1024 threads, thread
// (quarter, element) sums its quarter of the splits, the quarters meet in LDS as (q0 + q1) + (q2 + q3) (wgrad_reduce_kernel).
// src = this thread's element in split 0 (nullptr: outside the tensor).  Returns the sum in the threads of quarter 0.
template <bool Q4>
__device__ __forceinline__ float wgrad_tile_sum(const float* __restrict__ src, int S, size_t zs, float (*qs)[256]) {
  const int el = threadIdx.x & 255, w = threadIdx.x >> 8;
  if constexpr (!Q4) {
    float s = 0.f;
    if (src != nullptr)
      for (int z = 0; z < S; ++z) s += src[(size_t)z * zs];
    return s;
  } else {
    qs[w][el] = src != nullptr ? wgrad_quarter_sum(src, (int)(((long)S * w) / 4), (int)(((long)S * (w + 1)) / 4), zs) : 0.f;
    __syncthreads();
    return w == 0 ? (qs[0][el] + qs[1][el]) + (qs[2][el] + qs[3][el]) : 0.f;
  }
}

// Transposed-conv weight gradient: split sum AND the scatter to the torch layout dw[ci][co][kh][kw] in one launch (round 4: one node
// less per decoder layer on the training step's chain).  A block owns (co, 16 ci): element (e = kh * 4 + kw, ci) of phase (ph, pw),
// tap (th, tw) is summed over the splits straight from the slabs (16 consecutive ci = 64-byte runs), the tile is transposed through
// LDS and leaves as 16 runs of 64 bytes.
template <bool Q4>
__global__ __launch_bounds__(Q4 ? 1024 : 256) void convT_wgrad_reduce_unpack_kernel(const WGradP p) {
  __shared__ float tile[16][17];
  __shared__ float qs[Q4 ? 4 : 1][256];
  const int cb = (p.Ctot + 15) / 16;
  const int n = blockIdx.x / cb, ci0 = (blockIdx.x - n * cb) * 16;
  const int el = threadIdx.x & 255;
  {
    const int e = el >> 4, ci = ci0 + (el & 15);
    const int kh = e >> 2, kw = e & 3;
    const int ph = (kh & 1) ^ 1, th = (kh == 0 || kh == 3) ? 1 : 0, pw = (kw & 1) ^ 1, tw = (kw == 0 || kw == 3) ? 1 : 0;
    const size_t zs = (size_t)p.N * p.Kpad;
    const float* src = ci < p.Ctot ? p.ws + (size_t)(ph * 2 + pw) * p.S * zs + (size_t)n * p.Kpad + (size_t)(th * 2 + tw) * p.Ctot + ci : nullptr;
    const float v = wgrad_tile_sum<Q4>(src, p.S, zs, qs);
    if (threadIdx.x < 256) tile[el & 15][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < 256) {
    const int cl = el >> 4, e = el & 15;
    if (ci0 + cl < p.Ctot) p.dw[((size_t)(ci0 + cl) * p.N + n) * 16 + e] = tile[cl][e];
  }
}

// Conv2d weight gradient: split sum AND the re-layout packed [n][(tap, c)] -> torch [n][c][tap] in one launch (m2h_conv_wgrad_torch_f32: the
// permute(0, 3, 1, 2).contiguous() copy of the packed gradient was a launch per conv layer of every backward pass).  A block owns
// (n, 16 channels): its output is ONE run of 16 x ntap floats; taps go through the LDS tile sixteen at a time.
template <bool Q4>
__global__ __launch_bounds__(Q4 ? 1024 : 256) void conv_wgrad_reduce_torch_kernel(const WGradP p) {
  __shared__ float tile[16][17];
  __shared__ float qs[Q4 ? 4 : 1][256];
  const int Ci = p.torch_ci;
  const int cb = (Ci + 15) / 16;
  const int n = blockIdx.x / cb, ci0 = (blockIdx.x - n * cb) * 16;
  const size_t zs = (size_t)p.N * p.Kpad;
  const int el = threadIdx.x & 255;
  // gridDim.y > 1: a block takes every gridDim.y-th group of 16 taps (layers with few (n, 16-channel) blocks and many taps and splits --
  // VisualCNN's first conv: 32 blocks summing 64 taps x 500 splits took 37-41 us at the end of the policy epoch's longest branch)
  for (int t0 = 16 * blockIdx.y; t0 < p.ntap; t0 += 16 * gridDim.y) {
    {
      const int t = t0 + (el >> 4), ci = ci0 + (el & 15);
      const float* src = (t < p.ntap && ci < Ci) ? p.ws + (size_t)n * p.Kpad + (size_t)t * p.Ctot + ci : nullptr;
      const float v = wgrad_tile_sum<Q4>(src, p.S, zs, qs);
      if (threadIdx.x < 256) tile[el & 15][el >> 4] = v;
    }
    __syncthreads();
    if (threadIdx.x < 256) {
      const int cl = el >> 4, t = t0 + (el & 15);
      if (ci0 + cl < Ci && t < p.ntap) p.dw[((size_t)n * Ci + ci0 + cl) * p.ntap + t] = tile[cl][el & 15];
    }
    __syncthreads();
  }
}

int wgrad_finish(const WGradP& p, hipStream_t st) {
  if (p.quad) {   // split sum + scatter to the torch layout in one launch
    const long gu = (long)p.N * ((p.Ctot + 15) / 16);
    M2H_REQUIRE(gu < 0x7fffffffL, "convT_wgrad: unpack grid too large");
    if (p.S >= 16) M2H_LAUNCH(convT_wgrad_reduce_unpack_kernel<true>, dim3((unsigned)gu), dim3(1024), 0, st, p);
    else M2H_LAUNCH(convT_wgrad_reduce_unpack_kernel<false>, dim3((unsigned)gu), dim3(256), 0, st, p);
    return launch_status("convT_wgrad reduce + unpack");
  }
  if (p.torch_ci > 0) {   // split sum + re-layout to [N][Ci][KH][KW] in one launch
    const long gt = (long)p.N * ((p.torch_ci + 15) / 16);
    M2H_REQUIRE(gt < 0x7fffffffL, "conv_wgrad: reduce grid too large");
    const int tgroups = (p.ntap + 15) / 16;
    const unsigned gy = (unsigned)(gt >= 512 || tgroups == 1 ? 1 : (tgroups < 8 ? tgroups : 8));   // enough blocks for the chip before the taps are spread
    if (p.S >= 16) M2H_LAUNCH(conv_wgrad_reduce_torch_kernel<true>, dim3((unsigned)gt, gy), dim3(1024), 0, st, p);
    else M2H_LAUNCH(conv_wgrad_reduce_torch_kernel<false>, dim3((unsigned)gt, gy), dim3(256), 0, st, p);
    return launch_status("conv_wgrad reduce (torch layout)");
  }
  if (p.S >= 16) {
    const long g = (long)p.N * ((p.K + 63) / 64);
    M2H_REQUIRE(g < 0x7fffffffL, "conv_wgrad: reduce grid too large");
    M2H_LAUNCH(wgrad_reduce_kernel, dim3((unsigned)g), dim3(256), 0, st, p);
  } else {
    size_t g = ((size_t)p.N * p.K + 255) / 256;
    if (g > 4096) g = 4096;
    M2H_LAUNCH(wgrad_reduce_small_kernel, dim3((unsigned)g), dim3(256), 0, st, p);
  }
  return launch_status("conv_wgrad reduce");
}

}  // namespace m2h
