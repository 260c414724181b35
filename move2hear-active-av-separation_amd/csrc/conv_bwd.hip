// Weight gradient of the implicit-GEMM convolution (gfx950): the dispatch.  Validates, fills WGradP, chooses the splits, offers the launch
// to the kernel families in order (wgrad_common.h: image-row first, then tiled) and ends with the ordered split sum (wgrad_finish).
// The other backward pieces: the input gradient runs on the FORWARD engines (conv_dispatch.hip) over m2h_pack_dgrad_weight's phase
// matrices; act_bwd, bias_grad and the weight re-layouts are bwd_pointwise.hip.
#include "wgrad_common.h"

namespace m2h {

// How a launch differs from the plain packed gradient of a conv.
struct WGradOpts {
  bool quad = false;            // the four phases of a ConvTranspose2d(4,2,1) in one launch (a = the geometry of one phase: taps 2x2, stride 1, os 2,
                                // Ho = 2 Hi; its ph / pw / mulh / mulw are ignored), dw in the torch layout, workspace four times the single-phase size
  const float* gate = nullptr;  // the layer's forward output: dy is read as dy * (y > 0 ? 1 : gate_slope) (image-row kernels only)
  float gate_slope = 1.f;
  int torch_ci = 0;             // > 0: dw in nn.Conv2d's own layout [N][torch_ci][KH][KW]
  const float* dy2 = nullptr;   // the fused input gradient (m2h_conv_wgrad_dgrad_fused_f32): `dy` may be NULL, it is made inside the bf16x3 image-row
  const float* w2p = nullptr;   // kernel from the NEXT conv's output gradient dy2 [B][H][W][16] and packed weight w2p [16][9 * 32] (N = C0 = 32, gate required)
};

// the fields of p that follow from the geometry alone (no pointers, no S): what the image-row rule and the split count read
static void wgrad_geometry(const m2h_conv_args& a, int ldy, bool quad, WGradP& p) {
  p.C0 = a.C0; p.C1 = a.C1; p.Ctot = a.C0 + a.C1;
  p.B = a.B; p.Hi = a.Hi; p.Wi = a.Wi; p.Hq = a.Hq; p.Wq = a.Wq;
  p.stride = a.stride; p.ntw = a.ntw; p.ntap = a.nth * a.ntw; p.mulh = a.mulh; p.offh = a.offh; p.mulw = a.mulw; p.offw = a.offw;
  p.Ho = a.Ho; p.Wo = a.Wo; p.os = a.os; p.ph = a.ph; p.pw = a.pw;
  p.quad = quad ? 1 : 0;
  p.direct = (a.os == 1 && a.ph == 0 && a.pw == 0 && a.Ho == a.Hq && a.Wo == a.Wq) ? 1 : 0;
  p.ldy = ldy; p.N = a.N; p.K = p.ntap * p.Ctot; p.Kpad = (p.K + WK - 1) / WK * WK;
  const long M = (long)a.B * a.Hq * a.Wq;
  p.M = (int)M; p.chunks = (int)((M + WM - 1) / WM);
  int bng, kt;
  wgrad_cfg(a.N, p.K, bng, kt, p.ktiles, M);
  p.ntiles = (a.N + bng - 1) / bng;
}

// Splits over the pixel range.  The image-row GEOMETRY decides the 768-block target even where ldy or knob 21 later sends the launch to the
// tiled kernel: the workspace size is a function of the shape alone, and the launch splits as the workspace was sized.
static int wgrad_splits(const WGradP& p) {
  const long tiles = (long)p.ntiles * p.ktiles;
  // one wave front, no tail round: 3 resident blocks per CU for the one-sub-tile kernels (40 / 64 KB LDS, <= 176 VGPRs), 2 for
  // the wide-k ones (196-240 VGPRs); the image-row kernels (one block per split, 46 KB LDS) fill 3 per CU as well
  // (round 4: 512 for every tiled shape -- at 768 the one-sub-tile kernels' extra splits cost more in slabs and reduce than the third
  // resident block returned: the pre-training step 2.44 -> 2.41 ms); knob 11 (g_wgrad_blocks) > 0: that target instead
  const long target = g_wgrad_blocks > 0 ? g_wgrad_blocks : (wgrad_row3x3_rule(p, false) ? 768 : 512);
  long S = (target + tiles - 1) / tiles;
  if (S > p.chunks / 4) S = p.chunks / 4;   // at least 4 chunks per split
  if (S > 1024) S = 1024;
  if (S < 1) S = 1;
  return (int)S;
}

size_t conv_wgrad_workspace_bytes(const m2h_conv_args& a) {
  WGradP p;
  wgrad_geometry(a, a.N, false, p);
  return (size_t)wgrad_splits(p) * p.N * p.Kpad * sizeof(float);
}

int conv_wgrad_f32(const m2h_conv_args& a, const float* dy, int ldy, float* dw, hipStream_t st, const WGradOpts& o) {
  // which options go together (the two that need the image-row kernels: below, once the launch's shape is known)
  M2H_REQUIRE(o.torch_ci >= 0 && o.torch_ci <= a.C0 + a.C1 && (!o.quad || o.torch_ci == 0), "conv_wgrad: torch_ci (%d) must lie in 1 .. C0 + C1", o.torch_ci);
  M2H_REQUIRE(a.src0 != nullptr && (dy != nullptr || o.dy2 != nullptr) && dw != nullptr, "conv_wgrad: null pointer");
  M2H_REQUIRE((o.dy2 == nullptr) == (o.w2p == nullptr), "conv_wgrad: fused input gradient needs both dy2 and w2p");
  M2H_REQUIRE(ldy >= a.N || o.dy2 != nullptr, "conv_wgrad: ldy (%d) < N (%d)", ldy, a.N);
  // the geometry
  M2H_REQUIRE(a.conv_transpose == 0, "conv_wgrad: describe a transposed conv by its phase geometry (m2h_convT_wgrad_f32)");
  M2H_REQUIRE(!o.quad || (a.nth == 2 && a.ntw == 2 && a.stride == 1 && a.os == 2 && a.offh == 0 && a.offw == 0 && a.Hq == a.Hi && a.Wq == a.Wi &&
                          a.Ho == 2 * a.Hi && a.Wo == 2 * a.Wi),
              "convT_wgrad: phase geometry of ConvTranspose2d(4,2,1) expected (taps 2x2, stride 1, os 2, Ho = 2 Hi)");
  M2H_REQUIRE(a.C0 > 0 && a.C0 % 4 == 0 && a.C1 >= 0 && a.C1 % 4 == 0, "conv_wgrad: C0/C1 must be multiples of 4");
  M2H_REQUIRE((a.C1 == 0) == (a.src1 == nullptr), "conv_wgrad: src1/C1 mismatch");
  M2H_REQUIRE(a.B > 0 && a.Hi > 0 && a.Wi > 0 && a.Hq > 0 && a.Wq > 0 && a.N > 0 && a.nth > 0 && a.ntw > 0 && a.stride > 0, "conv_wgrad: bad sizes");
  M2H_REQUIRE((long)a.B * a.Hq * a.Wq < (1L << 30) && (long)a.B * a.Hi * a.Wi < (1L << 30), "conv_wgrad: too many pixels");
  M2H_REQUIRE(a.os >= 1 && (a.Hq - 1) * a.os + a.ph < a.Ho && (a.Wq - 1) * a.os + a.pw < a.Wo, "conv_wgrad: output pixel grid exceeds Ho x Wo");
  WGradP p;
  wgrad_geometry(a, ldy, o.quad, p);
  p.src0 = a.src0; p.src1 = a.src1; p.dy = dy; p.dw = dw;
  p.gate = o.gate; p.gate_slope = o.gate_slope; p.torch_ci = o.torch_ci; p.dy2 = o.dy2; p.w2p = o.w2p;
  const bool row3x3 = wgrad_row3x3_rule(p, true);
  M2H_REQUIRE(o.gate == nullptr || row3x3, "conv_wgrad: the activation gate is built into the image-row 3x3 kernel only (3x3 / stride 1 / pad 1, 32 channels, 32-pixel rows)");
  M2H_REQUIRE(o.dy2 == nullptr || (row3x3 && tl_math_mode == 1 && a.N == 32 && o.gate != nullptr),
              "conv_wgrad: the fused input gradient is built into the bf16x3 image-row 3x3 kernel only (N = 32, with the activation gate)");
  // splits and their slabs
  p.S = wgrad_splits(p);
  const size_t need = ((size_t)(o.quad ? 4 : 1) * p.S * p.N * p.Kpad + (o.quad ? (size_t)4 * p.N * p.K : 0)) * sizeof(float);
  M2H_REQUIRE(a.workspace != nullptr && a.workspace_bytes >= need, "conv_wgrad: workspace too small (need %zu bytes)", need);
  p.ws = static_cast<float*>(a.workspace);
  // the families in order, then the ordered split sum
  int rc = launch_wgrad_row3x3(p, st);
  if (rc == NOT_THIS_ENGINE) rc = launch_wgrad_tiled(p, st);
  return rc ? rc : wgrad_finish(p, st);
}

}  // namespace m2h

using namespace m2h;

extern "C" {

size_t m2h_conv_wgrad_workspace_bytes(const m2h_conv_args* args) { return args ? conv_wgrad_workspace_bytes(*args) : 0; }

int m2h_conv_wgrad_f32(const m2h_conv_args* args, const float* dy, int ldy, float* dw, m2h_stream stream) {
  M2H_REQUIRE(args != nullptr, "conv_wgrad: null args");
  return conv_wgrad_f32(*args, dy, ldy, dw, as_stream(stream), WGradOpts{});
}

int m2h_conv_wgrad_gated_f32(const m2h_conv_args* args, const float* dy, int ldy, const float* y, float slope, float* dw, m2h_stream stream) {
  M2H_REQUIRE(args != nullptr && y != nullptr, "conv_wgrad_gated: null pointer");
  WGradOpts o;
  o.gate = y; o.gate_slope = slope;
  return conv_wgrad_f32(*args, dy, ldy, dw, as_stream(stream), o);
}

int m2h_conv_wgrad_dgrad_fused_supported(const m2h_conv_args* args) {
  if (args == nullptr) return 0;
  WGradP p;
  wgrad_geometry(*args, args->N, false, p);
  return (wgrad_row3x3_rule(p, true) && tl_math_mode == 1 && p.N == 32) ? 1 : 0;
}

int m2h_conv_wgrad_dgrad_fused_f32(const m2h_conv_args* args, const float* dy2, const float* w2_packed, const float* y, float slope, float* dw, int Ci,
                                   m2h_stream stream) {
  M2H_REQUIRE(args != nullptr && dy2 != nullptr && w2_packed != nullptr && y != nullptr, "conv_wgrad_dgrad_fused: null pointer");
  M2H_REQUIRE(m2h_conv_wgrad_dgrad_fused_supported(args), "conv_wgrad_dgrad_fused: needs the bf16x3 arithmetic and the image-row shape (3x3 / 1 / 1, 32 -> 32 "
              "channels over 32-pixel rows); use m2h_conv_igemm_f32 (input gradient) + m2h_conv_wgrad_torch_f32 otherwise");
  WGradOpts o;
  o.gate = y; o.gate_slope = slope; o.torch_ci = Ci; o.dy2 = dy2; o.w2p = w2_packed;
  return conv_wgrad_f32(*args, nullptr, args->N, dw, as_stream(stream), o);
}

int m2h_conv_wgrad_torch_f32(const m2h_conv_args* args, const float* dy, int ldy, const float* y, float slope, float* dw, int Ci, m2h_stream stream) {
  M2H_REQUIRE(args != nullptr && Ci > 0, "conv_wgrad_torch: null args / Ci <= 0");
  WGradOpts o;
  o.gate = y; o.gate_slope = slope; o.torch_ci = Ci;
  return conv_wgrad_f32(*args, dy, ldy, dw, as_stream(stream), o);
}

// four phases of slabs + 4 * N * K floats that held the packed per-phase gradients: nothing writes those any more (the reduce scatters
// straight into the torch layout), but the size is part of the contract
size_t m2h_convT_wgrad_workspace_bytes(const m2h_conv_args* args) {
  return args ? 4 * conv_wgrad_workspace_bytes(*args) + (size_t)4 * args->N * args->nth * args->ntw * (args->C0 + args->C1) * sizeof(float) : 0;
}

int m2h_convT_wgrad_f32(const m2h_conv_args* args, const float* dy, int ldy, float* dw, m2h_stream stream) {
  M2H_REQUIRE(args != nullptr, "convT_wgrad: null args");
  WGradOpts o;
  o.quad = true;
  return conv_wgrad_f32(*args, dy, ldy, dw, as_stream(stream), o);
}

}  // extern "C"
