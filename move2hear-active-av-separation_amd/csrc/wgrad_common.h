// Weight gradient of the implicit-GEMM convolution (gfx950): what its units share.
//
//   dW[n][k] = sum_m dY[m][n] * A[m][k]   (reduction over output pixels m; A gathered exactly as in the forward) = the weight gradient of
//   Conv2d / Linear in the packed [N][K] layout, K = (tap, channel).  The pixel range is split over blocks; partial tiles go to a slab
//   [split][N][Kpad] and an ordered reduce kernel sums them (deterministic, no atomics).
//
// conv_bwd.hip validates the arguments, fills WGradP, sizes the slabs and offers the launch to the kernel families in the order they are
// declared below; wgrad_finish (wgrad_reduce.hip) sums the slabs into the layout the caller asked for.  A family's unit holds its kernels,
// their launch code and its shape rule; the rule reads WGradP and the tuning knobs only.
#pragma once
#include "m2h_internal.h"

namespace m2h {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct WGradP {
  const float* src0;
  const float* src1;
  int C0, C1, Ctot;
  int B, Hi, Wi, Hq, Wq;
  int stride, ntw, ntap, mulh, offh, mulw, offw;
  const float* dy;  // row m -> output pixel (b, q*os+ph, r*os+pw) of an NHWC [B][Ho][Wo][ldy] tensor
  int ldy;
  int Ho, Wo, os, ph, pw;
  int direct;       // 1: pixel index == m (os 1, Ho x Wo == Hq x Wq)
  int N, K, Kpad;   // Kpad = K rounded up to 128
  int M;
  int S;            // splits over m (grid z)
  int chunks;       // ceil(M / 32)
  int ntiles, ktiles;  // output tiles along n and k
  float* ws;        // [S][N][Kpad]  (quad: [4 phases][S][N][Kpad])
  float* dw;        // [N][K]        (quad: the transposed conv's torch layout [Ci][N][4][4])
  int quad;         // 1: the four sub-pixel phases of a ConvTranspose2d(4,2,1) in one launch of the tiled kernel (grid y = phase: its taps'
                    // direction, its dy rows, its slabs); convT_wgrad_reduce_unpack_kernel sums the slabs and scatters them into dw
  const float* gate;  // optional (image-row 3x3 kernel): the forward output y of the layer, same layout as dy: dy is read as
  float gate_slope;   // dy * (y > 0 ? 1 : gate_slope) -- the backward of the layer's fused ReLU / LeakyReLU without a pass of its own
  int torch_ci;       // > 0: dw is nn.Conv2d's own layout [N][torch_ci][KH][KW] (channels torch_ci .. Ctot-1 of the packed k axis are input padding: dropped)
  // fused input gradient (wgrad3x3_row_dgrad_bf16x3_kernel): dy2 != nullptr -> `dy` is not read; the layer's output gradient is made in the
  // kernel, row by row, as the input gradient of the NEXT 3x3 conv: dy[r][px][c] = sum_{tap, n} dy2[r + 1 - ty][px + 1 - tx][n] w2p[n][tap][c]
  const float* dy2;   // [rows][32][16] NHWC gradient of the next conv's output
  const float* w2p;   // the next conv's packed weight [16][9 * 32] (m2h_pack_conv_weight_ex)
};

// phase (ph, pw) of a quad launch: taps step by 2 ph - 1 / 2 pw - 1 (separator_cnn.py:15-24 as four sub-pixel GEMMs)
struct WPhase {
  int ph, pw, mulh, mulw;
  size_t ws_off;
};
__device__ __forceinline__ WPhase wgrad_phase(const WGradP& p) {
  WPhase w{p.ph, p.pw, p.mulh, p.mulw, 0};
  if (p.quad) {
    const int phase = blockIdx.y;
    w.ph = phase >> 1;
    w.pw = phase & 1;
    w.mulh = 2 * w.ph - 1;
    w.mulw = 2 * w.pw - 1;
    w.ws_off = (size_t)phase * p.S * p.N * p.Kpad;
  }
  return w;
}
constexpr int WK = 128;  // k sub-tile (one 16-byte segment per thread of a 32-thread row group)
constexpr int WM = 32;   // pixels per reduction chunk

// ---- the kernel families, in dispatch order.  A launcher returns NOT_THIS_ENGINE when the launch is not one of its shapes (nothing was
// launched), 0 after a launch, an error code otherwise.
// wgrad_row3x3.hip: image-row kernels (3x3 / 1 / 1 over 32-channel, 32-pixel-wide images, N <= 32) in either arithmetic, with the optional
// activation gate and fused input gradient; sets p.chunks to image rows and caps p.S by them.
// wgrad_row3x3_rule: launch = false: the geometry alone; true: with the launch's own conditions (ldy % 4, knob 21, one weight tile).
bool wgrad_row3x3_rule(const WGradP& p, bool launch);
int launch_wgrad_row3x3(WGradP& p, hipStream_t st);
// wgrad_tiled.hip: the tiled kernel; takes every launch (never NOT_THIS_ENGINE).  wgrad_cfg: its block shape for (N, K) -- n extent,
// 128-wide k sub-tiles per block, blocks along k
void wgrad_cfg(int N, int K, int& bng, int& kt, int& ktiles, long M = 1L << 30);
int launch_wgrad_tiled(WGradP& p, hipStream_t st);
// wgrad_reduce.hip: the ordered split sum that ends every launch, into the layout the caller asked for (the backward's finish_splitk)
int wgrad_finish(const WGradP& p, hipStream_t st);

}  // namespace m2h
