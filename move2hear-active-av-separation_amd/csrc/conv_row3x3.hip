// Image-row 3x3 engine: Conv2d(3x3, stride 1, pad 1) over 32-pixel-wide images with N <= 32 output channels in fp32 and in bf16x3
// math, the fused L1 loss of the 16-channel instantiations, the shape rule of both kernels and the C entry points of the fused op.
#include "igemm_common.h"

namespace m2h {

// Fused L1 epilogue of the image-row kernels' 16-channel instantiations (IGemmP::l1_gt): lane (band n = lane & 15, pixel group lane >> 4)
// holds four consecutive time frames of band n per 16-pixel fragment -- 16 contiguous bytes of the target plane -- so the loss costs one
// 16-byte load per fragment; the gradient sign(y - g) / n leaves in the conv's own NHWC layout, y itself is never stored (update_sep,
// ppo.py:206-216 with memory_nets.py:16,62-67: 110 MB written and read back per epoch otherwise, and one launch).  Returns the lane's |y - g| sum.
template <int FM, typename AccT>
__device__ __forceinline__ float l1_row_epilogue(const IGemmP& p, const AccT (&acc)[FM], int b, int q, int lane, float sh) {
  const int n = lane & 15;
  float s = 0.f;
#pragma unroll
  for (int mi = 0; mi < FM; ++mi) {
    const int x0 = mi * 16 + (lane >> 4) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(p.l1_gt + ((size_t)(b * 16 + n) * p.Ho + q) * p.Wo + x0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = (acc[mi][e] + sh) - g[e];
      s += fabsf(d);
      p.dst[((size_t)(b * p.Ho + q) * p.Wo + x0 + e) * p.ldc + n] = d > 0.f ? p.l1_inv : (d < 0.f ? -p.l1_inv : 0.f);
    }
  }
  return s;
}

// the block's partial sum of the fused loss: lanes -> wave (shuffles) -> the four waves in wave order, one float per block
__device__ __forceinline__ void l1_block_partial(const IGemmP& p, float s, float* scratch4, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();                                   // (scratch4 aliases the main loop's LDS: every wave is done with it)
  if ((tid & 63) == 0) scratch4[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) p.l1_part[blockIdx.x] = (scratch4[0] + scratch4[1]) + (scratch4[2] + scratch4[3]);
}

// loss = inv * sum of the blocks' partials, fixed order (one block of 256 threads; n <= 1024)
__global__ __launch_bounds__(256) void l1_partials_sum_kernel(const float* __restrict__ part, int n, float inv, float* __restrict__ loss) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = ((sh[0] + sh[1]) + (sh[2] + sh[3])) * inv;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Image-row 3x3 convolution (fp32 MFMA): Conv2d(3x3, stride 1, pad 1) over 16- or 32-channel, 32-pixel-wide images with N <= 32
// output channels -- AcousticMem's two convs (rl/models/memory_nets.py:11-16) and the input gradient of the second one, at the
// 1.7 M pixels of an update_sep epoch.  The register engine (conv_igemm.hip) fetches each pixel's nine taps separately (and its scalar loader
// needs C % 32 == 0, so the 16-channel input gradient ran on the per-lane decode); here a block keeps the whole weight matrix
// in LDS and walks chunks of FOUR image rows: the six input rows they touch are staged once as a zero-padded 6 x 34-pixel
// patch, every tap is a row / column shift of it, each wave owns one image row (32 pixels) x all output channels, and N <= 16
// runs on v_mfma_f32_16x16x4_f32.  Fragment reads are the 16-byte reads of the register engine (rows padded to C + 4 floats).
// Tap t = (th, tw) reads the input at (q + offh + th*mulh, r + offw + tw*mulw): forward (mul 1, off -1) and input gradient
// (mul -1, off 1) alike.  Epilogue: optional bias, ReLU / LeakyReLU, NHWC or de-sliced store.
template <int FR, int C>
__global__ __launch_bounds__(256, 2) void conv3x3_row_kernel(const IGemmP p) {
  constexpr int W = 32, PW = W + 2, ROWS = 4, PR = ROWS + 2;
  constexpr int CP = C + 4;                         // patch pixel stride (floats)
  constexpr int K = 9 * C, KP = K + 4;              // weight row stride: an odd multiple of 4 floats mod 64, like CP (conflict-free 16-byte reads)
  constexpr int GK = FR == 32 ? 8 : 16;             // k per fragment group (one 16-byte read per lane)
  constexpr int NG = C / GK;                        // groups per tap
  constexpr int FM = 32 / FR;                       // pixel fragments per wave (one image row)
  constexpr int NE = FR == 32 ? 16 : 4;
  constexpr int SEG = C / 4;                        // 16-byte segments per pixel
  constexpr int NPL = (PR * PW * SEG + 255) / 256;  // patch loads per thread
  using AccT = typename std::conditional<FR == 32, f32x16, f32x4>::type;
  static_assert(NG >= 1 && (KP % 64) % 8 == 4 && (CP % 64) % 8 == 4, "tile shape");
  __shared__ __attribute__((aligned(16))) float Wl[FR * KP];
  __shared__ __attribute__((aligned(16))) float Pl[PR * PW * CP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & (FR - 1), fk = (lane / FR) * 4;
  const int chunks = p.B * (p.Hq / ROWS);

  // weights [N][K] -> LDS rows (rows past N: zeros), once per block
  for (int i = tid; i < FR * (K / 4); i += 256) {
    const int n = i / (K / 4), s4 = i - n * (K / 4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < p.N) v = *reinterpret_cast<const f32x4*>(p.w + (size_t)n * K + s4 * 4);
    *reinterpret_cast<f32x4*>(&Wl[n * KP + s4 * 4]) = v;
  }
  int shift[9];                                     // patch offset of tap t relative to the output pixel's own patch position
#pragma unroll
  for (int t = 0; t < 9; ++t) shift[t] = (p.offh + (t / 3) * p.mulh) * PW + (p.offw + (t % 3) * p.mulw);

  f32x4 rp[NPL];
  unsigned okm = 0;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_chunk = [&](int c) {
    const int b = c / (p.Hq / ROWS), q0 = (c - b * (p.Hq / ROWS)) * ROWS;
    okm = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int i = tid + 256 * j;
      const int l = i / SEG, seg = i - l * SEG;
      const int pr = l / PW, pc = l - pr * PW;
      const int ih = q0 + pr - 1, iw = pc - 1;
      const bool ok = i < PR * PW * SEG && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)W;
      const size_t off = ok ? ((size_t)(b * p.Hi + ih) * W + iw) * C + seg * 4 : (size_t)0;
      rp[j] = *reinterpret_cast<const f32x4*>(p.src0 + off);
      okm |= ok ? (1u << j) : 0u;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int i = tid + 256 * j;
      if (i < PR * PW * SEG) *reinterpret_cast<f32x4*>(&Pl[(i / SEG) * CP + (i % SEG) * 4]) = (okm & (1u << j)) ? rp[j] : zero4;
    }
  };
  const size_t plane = (size_t)p.Ho * p.Wo;
  const int Cc = p.N >> 4;
  float l1_sum = 0.f;
  for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
    if (c == (int)blockIdx.x) load_chunk(c);
    __syncthreads();              // the previous chunk's fragment reads (and the weight stores) are done
    store_chunk();
    __syncthreads();
    if (c + (int)gridDim.x < chunks) load_chunk(c + gridDim.x);   // next chunk's loads fly under this chunk's MFMAs
    AccT acc[FM];
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[mi][e] = 0.f;
    const int prow0 = (wave + 1) * PW + 1;          // this wave's image row inside the patch, column 0
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f32x4 bw = *reinterpret_cast<const f32x4*>(&Wl[frow * KP + t * C + g * GK + fk]);
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(&Pl[(prow0 + mi * FR + frow + shift[t]) * CP + g * GK + fk]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if constexpr (FR == 32)
              acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bw[j], acc[mi], 0, 0, 0);
            else
              acc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bw[j], acc[mi], 0, 0, 0);
          }
        }
      }
    }
    // epilogue: rows = pixels of image row (q0 + wave), columns = output channels
    const int b = c / (p.Hq / ROWS), q = (c - b * (p.Hq / ROWS)) * ROWS + wave;
    const int n = lane & (FR - 1);
    const float sh = (p.shift != nullptr && n < p.N) ? p.shift[n] : 0.f;
    if constexpr (FR == 16) {
      if (p.l1_gt != nullptr) {       // (N == 16, NHWC, slope 1: host rule) the loss instead of the store
        l1_sum += l1_row_epilogue<FM>(p, acc, b, q, lane, sh);
        continue;
      }
    }
    if (n < p.N) {
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const int x = mi * FR + (FR == 32 ? (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) : (lane >> 4) * 4 + e);
          float v = acc[mi][e] + sh;
          v = v > 0.f ? v : v * p.slope;
          if (p.out_mode == M2H_OUT_NHWC) {
            p.dst[((size_t)(b * p.Ho + q) * p.Wo + x) * p.ldc + n] = v;
          } else {
            const size_t out = (size_t)b * 16 * plane + (size_t)q * p.Wo + x;
            p.dst[(out + (size_t)(n & 15) * plane) * Cc + (n >> 4)] = v;
          }
        }
    }
  }
  if constexpr (FR == 16) {
    if (p.l1_gt != nullptr) l1_block_partial(p, l1_sum, Pl, tid);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The image-row 3x3 convolution in bf16x3 arithmetic (three bf16 MFMAs per fp32 product: lo*hi + hi*lo + hi*hi, fp32 accumulate --
// the engine's split-product mode, M2H_MATH_BF16X3).  Same walk as conv3x3_row_kernel: a block keeps the weight matrix in LDS and
// stages four image rows + halo as a zero-padded 6 x 34-pixel patch; here both are SPLIT on the way into LDS -- a pixel's (a
// weight row's) k-values as [hi bf16 x K | lo bf16 x K] -- so a 16-byte fragment read is eight consecutive channels of one pixel:
// one operand of v_mfma_f32_32x32x16_bf16 (N <= 32) / v_mfma_f32_16x16x32_bf16 (N <= 16).  At the 1.7 M pixels of an update_sep
// epoch the fp32-MFMA kernel is matrix-bound (31.7 GFLOP of 16-pass fp32 MFMAs: 285 us at 71 % of the 157 TFLOP/s peak); the
// three bf16 MFMAs cost 3/16 of that, which leaves the layer to its HBM stream (220 MB in + 220 MB out).
// De-sliced store with N = 16: a lane's four accumulator values are four consecutive time frames of one band: one 16-byte store.
// blocks per CU by LDS: 32 -> 32 channels 66.8 KB (2), 32 -> 16 48.1 KB (3), 16 -> 32 35.3 KB (4, held at 3: the register budget of three)
template <int FR, int C>
__global__ __launch_bounds__(256, (FR == 32 && C == 32) ? 2 : 3) void conv3x3_row_bf16x3_kernel(const IGemmP p) {
  constexpr int W = 32, PW = W + 2, ROWS = 4, PR = ROWS + 2;
  constexpr int K = 9 * C;
  constexpr int PS = 4 * C + 16;                    // patch pixel stride, bytes ([hi C | lo C] + 16: an odd count of 16-byte units)
  constexpr int WS = 4 * K + 16;                    // weight row stride, bytes
  constexpr int KI = FR == 32 ? 16 : 32;            // k per MFMA
  constexpr int NG = C / KI;                        // MFMAs (x3) per tap
  constexpr int FM = 32 / FR;                       // pixel fragments per wave (one image row)
  constexpr int NE = FR == 32 ? 16 : 4;
  constexpr int SEG = C / 4;                        // 16-byte fp32 segments per pixel
  constexpr int NPL = (PR * PW * SEG + 255) / 256;  // patch loads per thread
  using AccT = typename std::conditional<FR == 32, f32x16, f32x4>::type;
  static_assert(NG >= 1 && C % KI == 0 && (PS / 16) % 2 == 1 && (WS / 16) % 2 == 1, "tile shape");
  __shared__ __attribute__((aligned(16))) char Wl[FR * WS];
  __shared__ __attribute__((aligned(16))) char Pl[PR * PW * PS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & (FR - 1), kq = lane / FR;
  const int chunks = p.B * (p.Hq / ROWS);

  auto split_store = [&](char* dst_hi, int lo_off, f32x4 v) {
    const bf16x4 hi = __builtin_convertvector(v, bf16x4);
    const f32x4 hf = __builtin_convertvector(hi, f32x4);
    const bf16x4 lo = __builtin_convertvector(v - hf, bf16x4);
    *reinterpret_cast<bf16x4*>(dst_hi) = hi;
    *reinterpret_cast<bf16x4*>(dst_hi + lo_off) = lo;
  };
  // weights [N][K] fp32 -> split LDS rows (rows past N: zeros), once per block
  for (int i = tid; i < FR * (K / 4); i += 256) {
    const int n = i / (K / 4), s4 = i - n * (K / 4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < p.N) v = *reinterpret_cast<const f32x4*>(p.w + (size_t)n * K + s4 * 4);
    split_store(Wl + n * WS + s4 * 8, 2 * K, v);
  }
  int shift[9];                                     // patch offset of tap t relative to the output pixel's own patch position
#pragma unroll
  for (int t = 0; t < 9; ++t) shift[t] = (p.offh + (t / 3) * p.mulh) * PW + (p.offw + (t % 3) * p.mulw);

  f32x4 rp[NPL];
  unsigned okm = 0;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_chunk = [&](int c) {
    const int b = c / (p.Hq / ROWS), q0 = (c - b * (p.Hq / ROWS)) * ROWS;
    okm = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int i = tid + 256 * j;
      const int l = i / SEG, seg = i - l * SEG;
      const int pr = l / PW, pc = l - pr * PW;
      const int ih = q0 + pr - 1, iw = pc - 1;
      const bool ok = i < PR * PW * SEG && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)W;
      const size_t off = ok ? ((size_t)(b * p.Hi + ih) * W + iw) * C + seg * 4 : (size_t)0;
      rp[j] = *reinterpret_cast<const f32x4*>(p.src0 + off);
      okm |= ok ? (1u << j) : 0u;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int i = tid + 256 * j;
      if (i < PR * PW * SEG) split_store(Pl + (i / SEG) * PS + (i % SEG) * 8, 2 * C, (okm & (1u << j)) ? rp[j] : zero4);
    }
  };
  auto mma = [&](const f32x4& a, const f32x4& b, AccT& c) {
    if constexpr (FR == 32)
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  };
  const size_t plane = (size_t)p.Ho * p.Wo;
  const int Cc = p.N >> 4;
  float l1_sum = 0.f;
  for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
    if (c == (int)blockIdx.x) load_chunk(c);
    __syncthreads();              // the previous chunk's fragment reads (and the weight stores) are done
    store_chunk();
    __syncthreads();
    if (c + (int)gridDim.x < chunks) load_chunk(c + gridDim.x);   // next chunk's loads fly under this chunk's MFMAs
    AccT acc[FM];
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[mi][e] = 0.f;
    const int prow0 = (wave + 1) * PW + 1;          // this wave's image row inside the patch, column 0
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const char* wp = Wl + frow * WS + (t * C + g * KI) * 2 + kq * 16;
        const f32x4 bh = *reinterpret_cast<const f32x4*>(wp), bl = *reinterpret_cast<const f32x4*>(wp + 2 * K);
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
          const char* ap = Pl + (prow0 + mi * FR + frow + shift[t]) * PS + g * KI * 2 + kq * 16;
          const f32x4 ah = *reinterpret_cast<const f32x4*>(ap), al = *reinterpret_cast<const f32x4*>(ap + 2 * C);
          mma(al, bh, acc[mi]);
          mma(ah, bl, acc[mi]);
          mma(ah, bh, acc[mi]);
        }
      }
    }
    // epilogue: rows = pixels of image row (q0 + wave), columns = output channels
    const int b = c / (p.Hq / ROWS), q = (c - b * (p.Hq / ROWS)) * ROWS + wave;
    const int n = lane & (FR - 1);
    const float sh = (p.shift != nullptr && n < p.N) ? p.shift[n] : 0.f;
    if constexpr (FR == 16) {
      if (p.l1_gt != nullptr) {       // (N == 16, NHWC, slope 1: host rule) the loss instead of the store
        l1_sum += l1_row_epilogue<FM>(p, acc, b, q, lane, sh);
        continue;
      }
    }
    if (n < p.N) {
#pragma unroll
      for (int mi = 0; mi < FM; ++mi) {
        if constexpr (FR == 16) {
          if (p.out_mode != M2H_OUT_NHWC && Cc == 1) {   // four consecutive frames of band n
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              v[e] = acc[mi][e] + sh;
              v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
            }
            *reinterpret_cast<f32x4*>(p.dst + (size_t)b * 16 * plane + (size_t)n * plane + (size_t)q * p.Wo + mi * FR + (lane >> 4) * 4) = v;
            continue;
          }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const int x = mi * FR + (FR == 32 ? (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) : (lane >> 4) * 4 + e);
          float v = acc[mi][e] + sh;
          v = v > 0.f ? v : v * p.slope;
          if (p.out_mode == M2H_OUT_NHWC) {
            p.dst[((size_t)(b * p.Ho + q) * p.Wo + x) * p.ldc + n] = v;
          } else {
            const size_t out = (size_t)b * 16 * plane + (size_t)q * p.Wo + x;
            p.dst[(out + (size_t)(n & 15) * plane) * Cc + (n >> 4)] = v;
          }
        }
      }
    }
  }
  if constexpr (FR == 16) {
    if (p.l1_gt != nullptr) l1_block_partial(p, l1_sum, reinterpret_cast<float*>(Pl), tid);
  }
}

// Shapes of the image-row 3x3 kernels, common to the fp32 and the bf16x3 one: a 3x3 / stride 1 / pad 1 conv (either tap direction) of
// one plain fp32 source over 32-pixel-wide images whose height is a multiple of 4, at least 512 four-row chunks, N <= 32 without BN
// scale, class plane or fused head.  The channel counts each kernel is built for are launch_row3x3's.
static bool row3x3_geometry(const IGemmP& p) {
  return g_row3x3 >= 0 && !p.convT && p.ntap / p.ntw == 3 && p.ntw == 3 && p.stride == 1 && p.os == 1 && p.ph == 0 && p.pw == 0 &&
         (p.mulh == 1 || p.mulh == -1) && p.offh == -p.mulh && p.mulw == p.mulh && p.offw == p.offh && p.C1 == 0 && p.Wq == 32 && p.Wi == 32 &&
         p.Hq == p.Hi && p.Ho == p.Hq && p.Wo == p.Wq && p.Hq % 4 == 0 && p.N <= 32 && p.N % 4 == 0 && p.scale == nullptr && p.cls_table == nullptr &&
         p.head_w == nullptr && !p.presplit && !p.dst_split && (long)p.B * (p.Hq / 4) >= 512 &&
         (p.out_mode == M2H_OUT_NHWC || p.N % 16 == 0);
}

// 3x3 / stride 1 / pad 1 over 16- or 32-channel, 32-pixel-wide images, many rows (AcousticMem in update_sep): the fp32 kernel, or in
// bf16x3 math (update_sep with sep_update_math / the far-target leg) the one with split operands in LDS and bf16 MFMAs.
// l1_loss != nullptr (with p.l1_gt / l1_part / l1_inv): the fused L1 loss, summed over the blocks' partials by a second launch.
int launch_row3x3(IGemmP& p, float* l1_loss, hipStream_t st) {
  if (!row3x3_geometry(p)) return NOT_THIS_ENGINE;
  const long chunks = (long)p.B * (p.Hq / 4);
  const dim3 blk(256);
  dim3 grid;
  if (p.math == 0 && (p.C0 == 16 || p.C0 == 32)) {
    grid = dim3((unsigned)(chunks < 512 ? chunks : 512));
    if (p.N <= 16 && p.C0 == 32) M2H_LAUNCH((conv3x3_row_kernel<16, 32>), grid, blk, 0, st, p);
    else if (p.N <= 16) M2H_LAUNCH((conv3x3_row_kernel<16, 16>), grid, blk, 0, st, p);
    else if (p.C0 == 32) M2H_LAUNCH((conv3x3_row_kernel<32, 32>), grid, blk, 0, st, p);
    else M2H_LAUNCH((conv3x3_row_kernel<32, 16>), grid, blk, 0, st, p);
  } else if (p.math == 1 && (p.C0 == 32 || (p.C0 == 16 && p.N > 16))) {
    const long cap = (p.N > 16 && p.C0 == 32) ? 512 : 768;      // resident blocks: two / three per CU (LDS)
    grid = dim3((unsigned)(chunks < cap ? chunks : cap));
    if (p.N <= 16) M2H_LAUNCH((conv3x3_row_bf16x3_kernel<16, 32>), grid, blk, 0, st, p);
    else if (p.C0 == 32) M2H_LAUNCH((conv3x3_row_bf16x3_kernel<32, 32>), grid, blk, 0, st, p);
    else M2H_LAUNCH((conv3x3_row_bf16x3_kernel<32, 16>), grid, blk, 0, st, p);
  } else {
    return NOT_THIS_ENGINE;
  }
  if (l1_loss != nullptr) {
    M2H_LAUNCH(l1_partials_sum_kernel, dim3(1), dim3(256), 0, st, p.l1_part, (int)grid.x, p.l1_inv, l1_loss);
    return launch_status(p.math == 0 ? "conv_igemm_f32 (image-row 3x3 + L1 loss)" : "conv_igemm_bf16x3 (image-row 3x3 + L1 loss)");
  }
  return launch_status(p.math == 0 ? "conv_igemm_f32 (image-row 3x3)" : "conv_igemm_bf16x3 (image-row 3x3)");
}

}  // namespace m2h

using namespace m2h;

extern "C" {

// the conv of m2h_conv3x3_l1_nhwc16 as conv_igemm_f32 sees it (pointers left null).  m2h_conv3x3_l1_nhwc16_supported below holds the SAME
// geometry as IGemmP fields: change the two together
static m2h_conv_args l1_conv_args(int B, int H, int T, int C) {
  m2h_conv_args a = {};
  a.C0 = C; a.B = B; a.Hi = H; a.Wi = T; a.Hq = H; a.Wq = T;
  a.stride = 1; a.nth = 3; a.ntw = 3; a.mulh = 1; a.offh = -1; a.mulw = 1; a.offw = -1;
  a.N = 16; a.slope = 1.f;
  a.Ho = H; a.Wo = T; a.os = 1; a.ldc = 16; a.out_mode = M2H_OUT_NHWC;
  return a;
}

// (1 iff the launch below would take an image-row 3x3 kernel for this shape: launch_row3x3's rule, on 32-channel 32 x 32 images)
int m2h_conv3x3_l1_nhwc16_supported(int B, int H, int T, int C) {
  IGemmP p = {};   // what row3x3_geometry reads of l1_conv_args' conv, as conv_igemm_f32 fills it
  p.C0 = C; p.B = B; p.Hi = H; p.Wi = T; p.Hq = H; p.Wq = T; p.Ho = H; p.Wo = T;
  p.stride = 1; p.ntap = 9; p.ntw = 3; p.mulh = 1; p.offh = -1; p.mulw = 1; p.offw = -1;
  p.N = 16; p.os = 1; p.out_mode = M2H_OUT_NHWC;
  return (B > 0 && H == 32 && C == 32 && row3x3_geometry(p)) ? 1 : 0;
}

int m2h_conv3x3_l1_nhwc16(const float* h, const float* wp, const float* gt_plane, float* dy, float* loss, float* partials, int B, int H, int T, int C,
                          m2h_stream stream) {
  M2H_REQUIRE(h && wp && gt_plane && dy && loss && partials, "conv3x3_l1_nhwc16: null pointer");
  M2H_REQUIRE(m2h_conv3x3_l1_nhwc16_supported(B, H, T, C), "conv3x3_l1_nhwc16: needs 32-channel, 32 x 32-pixel images and B >= 64 (the image-row kernels' shapes); "
              "use m2h_conv_igemm_f32 + m2h_l1_loss_nhwc16 otherwise");
  m2h_conv_args a = l1_conv_args(B, H, T, C);
  a.src0 = h; a.wp = wp; a.dst = dy;
  ConvL1 l1 = {gt_plane, partials, loss, 1.f / ((float)B * 16.f * (float)H * (float)T)};
  return conv_igemm_f32(a, as_stream(stream), &l1);
}

}  // extern "C"
