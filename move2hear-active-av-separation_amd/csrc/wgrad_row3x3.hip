// Weight gradient, the image-row 3x3 kernels (gfx950): fp32 MFMA, bf16x3, and bf16x3 with the next conv's input gradient fused in.
#include <type_traits>

#include "wgrad_common.h"

namespace m2h {

// Weight gradient of a 3x3 / stride 1 / pad 1 convolution over 32-channel, 32-pixel-wide images (both AcousticMem convs,
// rl/models/memory_nets.py:11-16, at 1.7 M pixels per update_sep epoch): the general kernel above gathers the nine taps of every
// pixel separately (1.15 KB per pixel through L2 -> LDS, 4.4 TB/s at 441 us) and pads N = 16 to a 32-wide fragment.  Here a
// reduction chunk is one IMAGE ROW: the three input rows it touches are staged once as a zero-padded 3 x 34-pixel patch (the
// nine taps are row / column shifts of that patch: 400 B per pixel), each wave owns 8 of the row's 32 pixels and ALL nine
// tap fragments of the output (no k padding: K = 288 exactly), and N <= 16 runs on v_mfma_f32_16x16x4_f32 (half the matrix
// work).  The four waves' partial tiles meet through LDS in wave order; splits over rows go to the usual slab + ordered reduce.
template <int FR>
__global__ __launch_bounds__(256) void wgrad3x3_row_kernel(const WGradP p) {
  constexpr int W = 32, C = 32, PW = W + 2;
  constexpr int CS = FR == 32 ? 32 : 48;            // patch pixel stride (floats): conflict-free fragment reads for both shapes
  constexpr int KH = 32 / FR;                       // channel halves per tap (16-wide fragments: 2)
  constexpr int KF = 9 * KH;                        // accumulator fragments per wave
  constexpr int MS = FR == 32 ? 2 : 4;              // pixels contracted per MFMA
  constexpr int STEPS = 8 / MS;                     // a wave owns 8 pixels of the row
  constexpr int NE = FR == 32 ? 16 : 4;
  constexpr int NPL = (3 * PW * 8 + 255) / 256;     // 16-byte patch loads per thread (816 in all)
  using AccT = typename std::conditional<FR == 32, f32x16, f32x4>::type;
  __shared__ __attribute__((aligned(16))) float Ps[2][3 * PW * CS];
  __shared__ __attribute__((aligned(16))) float Ys[2][W * FR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x;
  const int c0 = (int)(((long)p.chunks * split) / p.S), c1 = (int)(((long)p.chunks * (split + 1)) / p.S);

  f32x4 rp[NPL], ry;
  unsigned okm = 0;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int yrow = tid / (FR / 4), yseg = tid % (FR / 4);      // dY: 32 rows x FR/4 segments (FR = 16: the first 128 threads)
  auto load_chunk = [&](int c) {
    const int b = c / p.Hq, q = c - b * p.Hq;
    okm = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int i = tid + 256 * j;
      const int l = i >> 3, seg = i & 7;
      const int pr = l / PW, pc = l - pr * PW;
      const int ih = q + pr - 1, iw = pc - 1;
      const bool ok = i < 3 * PW * 8 && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)W;
      const size_t off = ok ? ((size_t)(b * p.Hi + ih) * W + iw) * C + seg * 4 : (size_t)0;
      rp[j] = *reinterpret_cast<const f32x4*>(p.src0 + off);
      okm |= ok ? (1u << j) : 0u;
    }
    const bool yok = yrow < W && yseg * 4 < p.N;
    ry = *reinterpret_cast<const f32x4*>(p.dy + (yok ? ((size_t)c * W + yrow) * p.ldy + yseg * 4 : (size_t)0));
    if (p.gate != nullptr) {   // m2h_act_bwd folded into the load: same values, no 3-tensor pass of its own
      const f32x4 gy = *reinterpret_cast<const f32x4*>(p.gate + (yok ? ((size_t)c * W + yrow) * p.ldy + yseg * 4 : (size_t)0));
#pragma unroll
      for (int e = 0; e < 4; ++e) ry[e] = gy[e] > 0.f ? ry[e] : ry[e] * p.gate_slope;
    }
    okm |= yok ? (1u << 8) : 0u;
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int i = tid + 256 * j;
      if (i < 3 * PW * 8) *reinterpret_cast<f32x4*>(&Ps[buf][(i >> 3) * CS + (i & 7) * 4]) = (okm & (1u << j)) ? rp[j] : zero4;
    }
    if (yrow < W) *reinterpret_cast<f32x4*>(&Ys[buf][yrow * FR + yseg * 4]) = (okm & (1u << 8)) ? ry : zero4;
  };

  AccT acc[KF];
#pragma unroll
  for (int f = 0; f < KF; ++f)
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[f][e] = 0.f;
  const int fi = lane & (FR - 1), fq = lane / FR;   // fragment row/column, pixel inside the MFMA's contraction
  const int m0 = wave * 8;
  auto compute = [&](int buf) {
    float av[STEPS];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) av[st] = Ys[buf][(m0 + MS * st + fq) * FR + fi];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ty = t / 3, tx = t - 3 * ty;
#pragma unroll
      for (int h = 0; h < KH; ++h) {
        float bv[STEPS];
#pragma unroll
        for (int st = 0; st < STEPS; ++st) bv[st] = Ps[buf][(ty * PW + m0 + MS * st + fq + tx) * CS + h * FR + fi];
#pragma unroll
        for (int st = 0; st < STEPS; ++st) {
          if constexpr (FR == 32)
            acc[t * KH + h] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[st], bv[st], acc[t * KH + h], 0, 0, 0);
          else
            acc[t * KH + h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st], bv[st], acc[t * KH + h], 0, 0, 0);
        }
      }
    }
  };

  if (c0 < c1) {
    load_chunk(c0);
    store_chunk(0);
    __syncthreads();
    int cur = 0;
    for (int c = c0; c + 1 < c1; ++c) {
      load_chunk(c + 1);
      compute(cur);
      store_chunk(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
    compute(cur);
  }
  __syncthreads();   // the stages become the cross-wave scratch

  // the four waves' partial tiles -> one tile, fragment by fragment: R[wave][n][k] in LDS, summed in wave order
  float* R = &Ps[0][0];                               // 4 x FR x FR floats <= 16 KB
  float* slab = p.ws + (size_t)split * p.N * p.Kpad;
#pragma unroll
  for (int f = 0; f < KF; ++f) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int n = FR == 32 ? (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) : (lane >> 4) * 4 + e;
      R[(wave * FR + n) * FR + fi] = acc[f][e];
    }
    __syncthreads();
    for (int i = tid; i < FR * FR; i += 256) {
      const int n = i / FR, kk = i - n * FR;
      const float v = (R[i] + R[FR * FR + i]) + (R[2 * FR * FR + i] + R[3 * FR * FR + i]);
      if (n < p.N) slab[(size_t)n * p.Kpad + (f / KH) * C + (f % KH) * FR + kk] = v;
    }
    __syncthreads();
  }
}

// The same weight gradient in bf16x3 arithmetic (M2H_MATH_BF16X3: lo*hi + hi*lo + hi*hi on the bf16 matrix pipe, fp32 accumulate).
// The reduction runs over PIXELS, so both operands of v_mfma_f32_16x16x32_bf16 (a lane holds eight consecutive k of its row) are
// needed pixel-contiguous: an image row of x is staged TRANSPOSED and split, XT[channel][32 pixels] as [hi | lo] bf16 (one MFMA
// contracts the whole 32-pixel row), and so is the row of dY, YT[n][32 pixels].  A tap's column shift is applied to dY instead of
// x -- dW[n][ty][tx][c] = sum_px' dY[px' - tx + 1][n] x[row + ty - 1][px'][c] -- and made in registers (a 16-byte fragment + the
// neighbouring dword, v_alignbit), so x rows are staged once, unshifted, in a ring of four (step c reads rows c - 1, c, c + 1 and
// row c + 2 arrives), and rows outside the image are skipped rather than staged as zeros.  Wave (nh, ch) owns the 16 x 16 tiles
// (n half, channel half) of all nine taps (N <= 16: channel half x taps 0-4 / 5-8): no cross-wave reduction.  One barrier per row.
// The fp32-MFMA kernel above is matrix-bound at 1.7 M pixels (324 us for the 32 x 288 gradient, 62 % of the fp32 peak); this one
// leaves the layer to its HBM stream (x + dY + gate: 660 MB).
constexpr int WRB_RS = 144;                         // row stride of the transposed stages, bytes: [hi 64 | lo 64 | 16]: 9 x 16 (odd)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- what the bf16x3 kernel and the one with the fused input gradient (below) share.  Their transposed store loops (store_t / store_x) and
// slab stores stay two copies: as shared helpers they moved instructions in the fused kernel (DESIGN appendix A).
__device__ __forceinline__ void wrb_mma(const f32x4& a, const f32x4& b, f32x4& c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ void wrb_split4(f32x4 v, bf16x4& hi, bf16x4& lo) {   // v ~ hi + lo
  hi = __builtin_convertvector(v, bf16x4);
  const f32x4 hf = __builtin_convertvector(hi, f32x4);
  lo = __builtin_convertvector(v - hf, bf16x4);
}
// dY fragments of the three column shifts (hi / lo) from this lane's 16 bytes yb of the staged row: the unshifted 16 bytes + the dword before / after
__device__ __forceinline__ void wrb_dy_frags(const char* yb, int kq, f32x4 (&ya)[3][2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const char* yp = yb + h * 64;
    const u32x4 d = *reinterpret_cast<const u32x4*>(yp);
    const unsigned before = kq > 0 ? *reinterpret_cast<const unsigned*>(yp - 4) : 0u;
    const unsigned after = kq < 3 ? *reinterpret_cast<const unsigned*>(yp + 16) : 0u;
    u32x4 l, r;                                    // l: element k takes dY[k + 1] (tap column 0); r: dY[k - 1] (tap column 2)
    l[0] = __builtin_amdgcn_alignbit(d[1], d[0], 16);
    l[1] = __builtin_amdgcn_alignbit(d[2], d[1], 16);
    l[2] = __builtin_amdgcn_alignbit(d[3], d[2], 16);
    l[3] = __builtin_amdgcn_alignbit(after, d[3], 16);
    r[0] = __builtin_amdgcn_alignbit(d[0], before, 16);
    r[1] = __builtin_amdgcn_alignbit(d[1], d[0], 16);
    r[2] = __builtin_amdgcn_alignbit(d[2], d[1], 16);
    r[3] = __builtin_amdgcn_alignbit(d[3], d[2], 16);
    ya[0][h] = __builtin_bit_cast(f32x4, l);
    ya[1][h] = __builtin_bit_cast(f32x4, d);
    ya[2][h] = __builtin_bit_cast(f32x4, r);
  }
}
// The three taps of kernel row ty (those in the wave's range [t_lo, t_hi)): three MFMAs each from the dY fragments of the column shifts and
// this lane's 16 bytes xb of the staged x row
__device__ __forceinline__ void wrb_tap_row(const f32x4 (&ya)[3][2], const char* xb, int ty, int t_lo, int t_hi, f32x4 (&acc)[9]) {
  const f32x4 bh = *reinterpret_cast<const f32x4*>(xb), bl = *reinterpret_cast<const f32x4*>(xb + 64);
#pragma unroll
  for (int tx = 0; tx < 3; ++tx) {
    const int t = ty * 3 + tx;
    if (t < t_lo || t >= t_hi) continue;
    wrb_mma(ya[tx][1], bh, acc[t]);
    wrb_mma(ya[tx][0], bl, acc[t]);
    wrb_mma(ya[tx][0], bh, acc[t]);
  }
}

template <int FR>
__global__ __launch_bounds__(256, 3) void wgrad3x3_row_bf16x3_kernel(const WGradP p) {
  constexpr int W = 32, C = 32;
  __shared__ __attribute__((aligned(16))) char XT[4][C * WRB_RS];      // ring over image rows (slot = row & 3)
  __shared__ __attribute__((aligned(16))) char YT[2][FR * WRB_RS];     // dY rows (slot = row & 1)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x;
  const int c0 = (int)(((long)p.chunks * split) / p.S), c1 = (int)(((long)p.chunks * (split + 1)) / p.S);
  const int rows_total = p.B * p.Hq;
  const int fi = lane & 15, kq = lane >> 4;
  const int nh = FR == 32 ? (wave >> 1) : 0, ch = wave & 1;
  const int t_lo = FR == 32 ? 0 : ((wave >> 1) ? 5 : 0), t_hi = FR == 32 ? 9 : ((wave >> 1) ? 9 : 5);

  // staging: thread (pixel = tid / 8, quad = tid % 8) moves 16 bytes = 4 channels of one pixel
  const int spx = tid >> 3, sq = tid & 7;
  f32x4 rx, ry;
  bool okx = false, oky = false;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_x = [&](int r) {                         // image row r (global row index b * Hq + ih)
    okx = r >= 0 && r < rows_total;
    rx = *reinterpret_cast<const f32x4*>(p.src0 + (okx ? ((size_t)r * W + spx) * C + sq * 4 : (size_t)0));
  };
  auto load_y = [&](int r) {
    oky = r < rows_total && sq * 4 < p.N;
    const size_t off = oky ? ((size_t)r * W + spx) * p.ldy + sq * 4 : (size_t)0;
    ry = *reinterpret_cast<const f32x4*>(p.dy + off);
    if (p.gate != nullptr) {   // m2h_act_bwd folded into the load
      const f32x4 gy = *reinterpret_cast<const f32x4*>(p.gate + off);
#pragma unroll
      for (int e = 0; e < 4; ++e) ry[e] = gy[e] > 0.f ? ry[e] : ry[e] * p.gate_slope;
    }
  };
  auto store_t = [&](char* base, f32x4 v) {          // rows 4 sq .. 4 sq + 3 of a transposed stage, column spx (second copy: the fused kernel's store_x)
    bf16x4 hi, lo;
    wrb_split4(v, hi, lo);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      char* d = base + (sq * 4 + e) * WRB_RS + spx * 2;
      *reinterpret_cast<__bf16*>(d) = hi[e];
      *reinterpret_cast<__bf16*>(d + 64) = lo[e];
    }
  };
  auto store_x = [&](int r) { if (okx) store_t(XT[r & 3], rx); };
  auto store_y = [&](int r) { if (sq * 4 < FR) store_t(YT[r & 1], oky ? ry : zero4); };

  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = zero4;
  auto compute = [&](int c) {
    const int q = c % p.Hq;
    f32x4 ya[3][2];
    wrb_dy_frags(YT[c & 1] + (nh * 16 + fi) * WRB_RS + kq * 16, kq, ya);
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
      if (3 * ty + 3 <= t_lo || 3 * ty >= t_hi) continue;            // (wave-uniform: none of this wave's taps)
      const int ih = q + ty - 1;
      if ((unsigned)ih >= (unsigned)p.Hq) continue;                  // the row above / below the image: zeros
      wrb_tap_row(ya, XT[(c + ty - 1) & 3] + (ch * 16 + fi) * WRB_RS + kq * 16, ty, t_lo, t_hi, acc);
    }
  };

  if (c0 < c1) {
    // prologue: rows c0 - 1, c0, c0 + 1 of x and row c0 of dY staged; rows c0 + 2 / c0 + 1 in registers
#pragma unroll 1
    for (int r = c0 - 1; r <= c0 + 1; ++r) {
      load_x(r);
      store_x(r);
    }
    load_y(c0);
    store_y(c0);
    load_x(c0 + 2);
    load_y(c0 + 1);
    __syncthreads();
#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
      store_x(c + 2);                  // slot (c + 2) & 3 held row c - 2: last read in step c - 1, before that step's barrier
      store_y(c + 1);
      if (c + 1 < c1) {
        load_x(c + 3);
        load_y(c + 2);
      }
      compute(c);
      __syncthreads();
    }
  }

  // each wave owns its tiles: slab[split][n][t * 32 + ch * 16 + col] (second copy: the end of the fused kernel)
  float* slab = p.ws + (size_t)split * p.N * p.Kpad;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    if (t < t_lo || t >= t_hi) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = nh * 16 + kq * 4 + e;
      if (n < p.N) slab[(size_t)n * p.Kpad + t * C + ch * 16 + fi] = acc[t][e];
    }
  }
}

// The bf16x3 image-row weight gradient with the INPUT GRADIENT OF THE NEXT CONV fused in (update_sep's backward through AcousticMem,
// memory_nets.py:11-16: conv 32 -> 32, ReLU, conv 32 -> 16): the gradient this layer's weight gradient contracts with -- d loss / d h,
// h = ReLU(conv0(x)) -- is itself conv1's input gradient, a 3x3 convolution of d loss / d y (16 channels) with conv1's weights.  As two
// launches that tensor (220 MB at 1680 samples) is written by the one and read back, with the ReLU gate's 220 MB, by the other; here a
// block makes each image row of it on the matrix pipe from a ring of three staged rows of d loss / d y (110 MB in all) and conv1's
// weights held in registers as A fragments, gates it with h and writes it -- transposed and split, as the weight-gradient MFMAs want
// their pixel-contracted operand -- straight into the LDS stage the plain kernel fills from memory.  Per row: 15 more MFMAs per wave,
// no second barrier (five-slot rings: row c + 3 is staged while rows c - 1 .. c + 2 are read).
// D[c][px] = sum_k A[c][k] B[k][px], k = (tap, n): lane (row c = lane & 15, k-quarter kq) of k-step s holds tap 2 s + (kq >> 1),
// channels 8 (kq & 1) .. + 7 of d loss / d y at pixel (r + 1 - ty, px + 1 - tx) -- one 16-byte read of the ring ([hi 16 | lo 16] bf16 per pixel).
constexpr int WRD_PS = 80;                          // d loss / d y ring: pixel stride, bytes ([hi 32 | lo 32 | 16]: 5 x 16, odd)
constexpr int WRD_RS = 34 * WRD_PS;                 // ring row: 32 pixels + a zero pixel on either side
__global__ __launch_bounds__(256, 3) void wgrad3x3_row_dgrad_bf16x3_kernel(const WGradP p) {
  constexpr int W = 32, C = 32, FR = 32;
  __shared__ __attribute__((aligned(16))) char XT[5][C * WRB_RS];      // x rows, transposed + split (slot = row % 5)
  __shared__ __attribute__((aligned(16))) char YT[2][FR * WRB_RS];     // rows of the fused gradient (slot = row & 1)
  __shared__ __attribute__((aligned(16))) char DY[5][WRD_RS];          // d loss / d y rows, pixel-major + split (slot = row % 5)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x;
  const int c0 = (int)(((long)p.chunks * split) / p.S), c1 = (int)(((long)p.chunks * (split + 1)) / p.S);
  const int rows_total = p.B * p.Hq;
  const int fi = lane & 15, kq = lane >> 4;
  const int nh = wave >> 1, ch = wave & 1;           // weight-gradient role: (output-channel half, x-channel half)
  const int dch = wave & 1, dpx = wave >> 1;         // input-gradient role: tile (channel half, pixel half) of the 32 x 32 row
  auto slot5 = [](int r) { return (r + 5) % 5; };
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // staging roles: x -- thread (pixel tid / 8, quad tid % 8); d loss / d y -- threads 0..127 (pixel tid / 4, quad tid % 4)
  const int spx = tid >> 3, sq = tid & 7;
  const int ypx = tid >> 2, yq = tid & 3;
  f32x4 rx, rd, rg, rg_next;
  bool okx = false, okd = false;
  auto load_x = [&](int r) {
    okx = r >= 0 && r < rows_total;
    rx = *reinterpret_cast<const f32x4*>(p.src0 + (okx ? ((size_t)r * W + spx) * C + sq * 4 : (size_t)0));
  };
  auto load_d = [&](int r) {
    okd = tid < 128 && r >= 0 && r < rows_total;
    rd = *reinterpret_cast<const f32x4*>(p.dy2 + (okd ? ((size_t)r * W + ypx) * 16 + yq * 4 : (size_t)0));
  };
  auto load_g = [&](int r) {                         // the gate (this layer's forward output) at this lane's four accumulator elements of row r
    const bool ok = r >= 0 && r < rows_total;
    return *reinterpret_cast<const f32x4*>(p.gate + (ok ? ((size_t)r * W + dpx * 16 + fi) * C + dch * 16 + kq * 4 : (size_t)0));
  };
  auto store_x = [&](int r) {                        // rows 4 sq .. 4 sq + 3 of the transposed stage, column spx (wgrad3x3_row_bf16x3_kernel's store_t)
    if (!okx) return;
    bf16x4 hi, lo;
    wrb_split4(rx, hi, lo);
    char* base = XT[slot5(r)];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      char* d = base + (sq * 4 + e) * WRB_RS + spx * 2;
      *reinterpret_cast<__bf16*>(d) = hi[e];
      *reinterpret_cast<__bf16*>(d + 64) = lo[e];
    }
  };
  auto store_d = [&](int r) {                        // pixel ypx + 1 of the ring row, channels 4 yq .. + 3
    if (!okd) return;
    bf16x4 hi, lo;
    wrb_split4(rd, hi, lo);
    char* d = DY[slot5(r)] + (ypx + 1) * WRD_PS + yq * 8;
    *reinterpret_cast<bf16x4*>(d) = hi;
    *reinterpret_cast<bf16x4*>(d + 32) = lo;
  };

  // conv1's weights as the A fragments of the input gradient, once per block: row c = dch * 16 + fi, k-step s, this lane's eight k
  f32x4 wa[5][2];
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int tap = 2 * s + (kq >> 1), n0 = (kq & 1) * 8;
    f32x4 v0 = zero4, v1 = zero4;
    if (tap < 9) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v0[j] = p.w2p[(size_t)(n0 + j) * (9 * C) + tap * C + dch * 16 + fi];
        v1[j] = p.w2p[(size_t)(n0 + 4 + j) * (9 * C) + tap * C + dch * 16 + fi];
      }
    }
    bf16x4 h0, l0, h1, l1;
    wrb_split4(v0, h0, l0);
    wrb_split4(v1, h1, l1);
    bf16x8 hh, ll;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hh[j] = h0[j]; hh[4 + j] = h1[j];
      ll[j] = l0[j]; ll[4 + j] = l1[j];
    }
    wa[s][0] = __builtin_bit_cast(f32x4, hh);
    wa[s][1] = __builtin_bit_cast(f32x4, ll);
  }
  // the ring rows' zero pixels (columns -1 and 32): never written again
  for (int i = tid; i < 5 * 2 * (WRD_PS / 16); i += 256) {
    const int sl = i / (2 * (WRD_PS / 16)), rem = i - sl * 2 * (WRD_PS / 16);
    const int side = rem / (WRD_PS / 16), q16 = rem - side * (WRD_PS / 16);
    *reinterpret_cast<f32x4*>(DY[sl] + (side ? 33 : 0) * WRD_PS + q16 * 16) = zero4;
  }

  // image row r of the fused gradient -> YT[r & 1] (gate values of the row in g)
  auto dgrad_row = [&](int r, const f32x4& g) {
    const int q = r % p.Hq;
    f32x4 acc = zero4, acc_b = zero4;                 // two accumulation chains (even / odd k-steps): half the dependent MFMA latency per row
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int tap = 2 * s + (kq >> 1);
      const int ty = tap / 3, tx = tap - 3 * ty;
      const int qq = q + 1 - ty;
      const bool ok = tap < 9 && (unsigned)qq < (unsigned)p.Hq;
      const char* bp = DY[slot5(ok ? r + 1 - ty : r)] + (dpx * 16 + fi + 2 - tx) * WRD_PS + (kq & 1) * 16;
      f32x4 bh = *reinterpret_cast<const f32x4*>(bp), bl = *reinterpret_cast<const f32x4*>(bp + 32);
      bh = ok ? bh : zero4;
      bl = ok ? bl : zero4;
      f32x4& a_ = (s & 1) ? acc_b : acc;
      wrb_mma(wa[s][1], bh, a_);
      wrb_mma(wa[s][0], bl, a_);
      wrb_mma(wa[s][0], bh, a_);
    }
    acc += acc_b;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = g[e] > 0.f ? acc[e] : acc[e] * p.gate_slope;
    bf16x4 hi, lo;
    wrb_split4(v, hi, lo);
    char* yb = YT[r & 1] + (dch * 16 + kq * 4) * WRB_RS + (dpx * 16 + fi) * 2;   // rows = channels (kq * 4 + e), column = pixel
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      *reinterpret_cast<__bf16*>(yb + e * WRB_RS) = hi[e];
      *reinterpret_cast<__bf16*>(yb + e * WRB_RS + 64) = lo[e];
    }
  };

  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = zero4;
  auto compute = [&](int c) {
    const int q = c % p.Hq;
    f32x4 ya[3][2];
    wrb_dy_frags(YT[c & 1] + (nh * 16 + fi) * WRB_RS + kq * 16, kq, ya);
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
      if (3 * ty + 3 <= 0 || 3 * ty >= 9) continue;            // (wave-uniform: none of this wave's taps)
      const int ih = q + ty - 1;
      if ((unsigned)ih >= (unsigned)p.Hq) continue;                  // the row above / below the image: zeros
      wrb_tap_row(ya, XT[slot5(c + ty - 1)] + (ch * 16 + fi) * WRB_RS + kq * 16, ty, 0, 9, acc);
    }
  };

  if (c0 < c1) {
    // prologue: rows c0 - 1 .. c0 + 2 of x and of d loss / d y staged, the fused gradient's row c0 made; row c0 + 3 in registers
#pragma unroll 1
    for (int r = c0 - 1; r <= c0 + 2; ++r) {
      load_x(r);
      store_x(r);
      load_d(r);
      store_d(r);
    }
    rg = load_g(c0);
    __syncthreads();
    dgrad_row(c0, rg);
    rg = load_g(c0 + 1);
    load_x(c0 + 3);
    load_d(c0 + 3);
    __syncthreads();
#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
      // slots of row c + 3 held row c - 2: last read in step c - 1 (x: its weight-gradient step read rows c - 2 .. c; d loss / d y: the
      // gradient row c was made from rows c - 1 .. c + 1 in step c - 1), before that step's barrier
      store_x(c + 3);
      store_d(c + 3);
      if (c + 1 < c1) {
        rg_next = load_g(c + 2);
        load_x(c + 4);
        load_d(c + 4);
        dgrad_row(c + 1, rg);      // reads ring rows c .. c + 2 (staged in earlier steps) -> YT[(c + 1) & 1], read after this step's barrier
        rg = rg_next;
      }
      compute(c);                  // reads YT[c & 1] (made in the previous step) and x rows c - 1 .. c + 1
      __syncthreads();
    }
  }

  // (wgrad3x3_row_bf16x3_kernel<32>'s slab store)
  float* slab = p.ws + (size_t)split * p.N * p.Kpad;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = nh * 16 + kq * 4 + e;
      if (n < p.N) slab[(size_t)n * p.Kpad + t * C + ch * 16 + fi] = acc[t][e];
    }
  }
}

// The shapes the image-row kernels take: 3x3 / stride 1 / pad 1 over one 32-channel source of 32-pixel-wide images, output grid == image,
// N <= 32 in whole 16-byte segments.  launch: with the conditions of the launch itself -- dy rows in whole 16-byte segments, knob 21 >= 0,
// one weight tile.
bool wgrad_row3x3_rule(const WGradP& p, bool launch) {
  const bool shape = !p.quad && p.ntap == 9 && p.ntw == 3 && p.stride == 1 && p.mulh == 1 && p.mulw == 1 && p.offh == -1 && p.offw == -1 &&
                     p.C0 == 32 && p.C1 == 0 && p.Wq == 32 && p.Wi == 32 && p.Hq == p.Hi && p.direct && p.N <= 32 && p.N % 4 == 0;
  return shape && (!launch || (p.ldy % 4 == 0 && g_wgrad_row3x3 >= 0 && p.ntiles * p.ktiles == 1));
}

int launch_wgrad_row3x3(WGradP& p, hipStream_t st) {
  if (!wgrad_row3x3_rule(p, true)) return NOT_THIS_ENGINE;
  p.chunks = p.B * p.Hq;   // one image row per reduction chunk
  if (p.S > p.chunks) p.S = p.chunks;
  const dim3 grid((unsigned)p.S), blk(256);
  if (p.dy2 != nullptr) M2H_LAUNCH(wgrad3x3_row_dgrad_bf16x3_kernel, grid, blk, 0, st, p);
  else if (tl_math_mode == 1) {   // the calling thread computes in bf16x3 (update_sep with sep_update_math, the far-target leg)
    if (p.N <= 16) M2H_LAUNCH((wgrad3x3_row_bf16x3_kernel<16>), grid, blk, 0, st, p);
    else M2H_LAUNCH((wgrad3x3_row_bf16x3_kernel<32>), grid, blk, 0, st, p);
  } else if (p.N <= 16) M2H_LAUNCH((wgrad3x3_row_kernel<16>), grid, blk, 0, st, p);
  else M2H_LAUNCH((wgrad3x3_row_kernel<32>), grid, blk, 0, st, p);
  return launch_status("conv_wgrad");
}

}  // namespace m2h
