// Forward dispatch of the implicit-GEMM convolution: conv_igemm_f32 validates an m2h_conv_args, fills the kernels' IGemmP (tap window
// included) and offers the launch to the engines in a fixed order (igemm_common.h: one launcher per engine, each with its own shape
// rule); conv_igemm_workspace_bytes sizes the split-K scratch such a launch can use.  Also home of the calling thread's arithmetic mode
// and of the library's launch counter.
#include "igemm_common.h"

namespace m2h {

thread_local int tl_math_mode = 0;   // m2h_set_math_mode: the calling thread's arithmetic (0 fp32 MFMA, 1 bf16x3 split products)
std::atomic<long long> g_launch_count{0};   // M2H_LAUNCH (m2h_internal.h)
thread_local int tl_hi_only = 0;     // m2h_set_math_mode(M2H_MATH_BF16): tl_math_mode = 1 for every dispatch decision, and the engines listed in m2h.h drop the two cross products

// arithmetic of a launch: the M2H_FMT_MATH_* bit of its operand_format, else the calling thread's mode (0 fp32 MFMA, 1 bf16x3)
static int math_of(int operand_format) {
  return (operand_format & M2H_FMT_MATH_BF16X3) ? 1 : (operand_format & M2H_FMT_MATH_FP32) ? 0 : tl_math_mode;
}

// Tap window (see IGemmP): the contiguous range of kernel rows / columns that reach inside the image for at least one output
// pixel.  conv: ih = q*stride + off + t*mul, q in [0, Q); transposed conv: both sub-pixel phases (mul = -1, +1, off = 0) must agree.
static void tap_range(int ntaps, int Q, int stride, int off, int mul, int extent, int& t0, int& tn) {
  int lo = ntaps, hi = -1;
  for (int t = 0; t < ntaps; ++t) {
    bool any = false;
    for (int q = 0; q < Q && !any; ++q) {
      const int i = q * stride + off + t * mul;
      any = i >= 0 && i < extent;
    }
    if (any) {
      lo = t < lo ? t : lo;
      hi = t > hi ? t : hi;
    }
  }
  if (hi < 0) { t0 = 0; tn = ntaps; return; }   // nothing reaches the image: keep the full walk (all-zero result either way)
  t0 = lo;
  tn = hi - lo + 1;
}

static void tap_window(const m2h_conv_args& a, int& th0, int& thn, int& tw0, int& twn) {
  th0 = 0; thn = a.nth; tw0 = 0; twn = a.ntw;
  if (a.Hq > 64 || a.Wq > 4096 || g_tap_window < 0) return;   // large images: every tap is reached, skip the scan
  if (a.conv_transpose) {
    int a0, an, b0, bn;
    tap_range(a.nth, a.Hq, 1, 0, -1, a.Hi, a0, an);
    tap_range(a.nth, a.Hq, 1, 0, +1, a.Hi, b0, bn);
    if (a0 == b0 && an == bn) { th0 = a0; thn = an; }
    tap_range(a.ntw, a.Wq, 1, 0, -1, a.Wi, a0, an);
    tap_range(a.ntw, a.Wq, 1, 0, +1, a.Wi, b0, bn);
    if (a0 == b0 && an == bn) { tw0 = a0; twn = an; }
  } else {
    tap_range(a.nth, a.Hq, a.stride, a.offh, a.mulh, a.Hi, th0, thn);
    tap_range(a.ntw, a.Wq, a.stride, a.offw, a.mulw, a.Wi, tw0, twn);
  }
}

// Reduction length the launch will walk: the tap window applies to the scalar-decode loader only.
static int walked_K(const m2h_conv_args& a) {
  const int Ctot = a.C0 + a.C1;
  const bool fast = a.C0 % BK == 0 && a.C1 % BK == 0 && a.C0 > 0;
  if (!fast) return a.nth * a.ntw * Ctot;
  int th0, thn, tw0, twn;
  tap_window(a, th0, thn, tw0, twn);
  return thn * twn * Ctot;
}

size_t conv_igemm_workspace_bytes(const m2h_conv_args& a) {
  // the exact split-K scratch of the automatic choice for these arguments: phases * S * M * N floats
  const long M = (long)a.B * a.Hq * a.Wq;
  const int phases = a.conv_transpose ? 4 : 1;
  const int K = walked_K(a);
  int BM, BN;
  pick_tile(M, a.N, BM, BN);
  const int S = splitk_for(M, a.N, K, phases, BM, BN);
  size_t bytes = S <= 1 ? 0 : (size_t)phases * S * M * a.N * sizeof(float);
  // split32 operands in bf16x3 math: the LDS-DMA engine's two-K-halves launch of the 256 x 128 tile (conv_dma.hip) takes its slabs
  // from this workspace too -- report them, so that a caller who sizes the workspace by this function gets the same kernel (and the
  // same fp32 summation order) as the whole-network runner, whose scratch is the maximum over its stages
  const int both = M2H_FMT_SRC_SPLIT | M2H_FMT_W_SPLIT;
  if (math_of(a.operand_format) == 1 && (a.operand_format & both) == both && a.head_w == nullptr && a.C0 % BK == 0 && a.C1 % BK == 0 && M > 64 && g_force_splitk <= 0) {
    const size_t need = (size_t)phases * 2 * M * a.N * sizeof(float);
    if (dma_split2_rule(M, a.N, K, phases, true, need)) {
      if (need > bytes) bytes = need;
    } else {
      const int Sd = dma_deep_split(M, a.N, K, phases);   // ... and its S K-parts launch on the deepest stages
      const size_t needd = (size_t)phases * Sd * M * a.N * sizeof(float);
      if (Sd > 1 && needd > bytes) bytes = needd;
    }
  }
  return bytes;
}

// the m2h_conv_args -> IGemmP fill alone (sizes checked positive by the caller)
static IGemmP conv_params(const m2h_conv_args& a) {
  IGemmP p = {};   // (MT, NT, S, pmaj: the launcher's)
  p.src0 = a.src0; p.src1 = a.src1; p.C0 = a.C0; p.C1 = a.C1; p.Ctot = a.C0 + a.C1;
  p.B = a.B; p.Hi = a.Hi; p.Wi = a.Wi; p.Hq = a.Hq; p.Wq = a.Wq; p.stride = a.stride;
  p.wq_sh = (a.Wq & (a.Wq - 1)) == 0 ? __builtin_ctz((unsigned)a.Wq) : -1;
  p.hq_sh = (a.Hq & (a.Hq - 1)) == 0 ? __builtin_ctz((unsigned)a.Hq) : -1;
  p.ntw = a.ntw; p.ntap = a.nth * a.ntw;
  p.mulh = a.mulh; p.offh = a.offh; p.mulw = a.mulw; p.offw = a.offw; p.convT = a.conv_transpose ? 1 : 0;
  p.w = a.wp; p.N = a.N; p.K = p.ntap * p.Ctot;
  p.scale = a.scale; p.shift = a.shift; p.slope = a.slope; p.cls_table = a.cls_table; p.cls_val = a.cls_val;
  p.head_w = a.head_w; p.head_b = a.head_b;
  p.math = math_of(a.operand_format);
  p.hi_only = (p.math == 1 && tl_hi_only) ? 1 : 0;
  const int both = M2H_FMT_SRC_SPLIT | M2H_FMT_W_SPLIT;
  p.presplit = (a.operand_format & both) == both ? 1 : 0;
  p.dst_split = (a.operand_format & M2H_FMT_DST_SPLIT) ? 1 : 0;
  p.dst = a.dst; p.Ho = a.Ho; p.Wo = a.Wo; p.os = a.os; p.ph = a.ph; p.pw = a.pw; p.ldc = a.ldc; p.out_mode = a.out_mode;
  p.M = (int)((long)a.B * a.Hq * a.Wq);
  {
    const size_t pix = (size_t)a.B * a.Hi * a.Wi;
    const size_t lim = (size_t)1 << 32;
    p.fast_ok = (a.C0 % BK == 0 && a.C1 % BK == 0 && a.C0 > 0 && pix * a.C0 * 4 < lim && pix * (size_t)a.C1 * 4 < lim &&
                 (size_t)a.N * p.K * 4 < lim) ? 1 : 0;
  }
  tap_window(a, p.th0, p.thn, p.tw0, p.twn);
  p.Kw = p.thn * p.twn * p.Ctot;
  p.ws = static_cast<float*>(a.workspace);
  return p;
}

// l1: optional fused L1 loss (m2h_conv3x3_l1_nhwc16): honoured by the image-row 3x3 kernels' 16-channel instantiations only -- any other
// dispatch is an error, never a silent plain conv
int conv_igemm_f32(const m2h_conv_args& a, hipStream_t st, const ConvL1* l1) {
  M2H_REQUIRE(a.src0 != nullptr && a.wp != nullptr && a.dst != nullptr, "conv_igemm: null pointer");
  M2H_REQUIRE(a.B > 0 && a.Hi > 0 && a.Wi > 0 && a.Hq > 0 && a.Wq > 0 && a.N > 0, "conv_igemm: non-positive size");
  M2H_REQUIRE(a.C0 > 0 && a.C0 % 4 == 0 && a.C1 >= 0 && a.C1 % 4 == 0, "conv_igemm: C0/C1 must be multiples of 4 (got %d, %d)", a.C0, a.C1);
  M2H_REQUIRE((a.C1 == 0) == (a.src1 == nullptr), "conv_igemm: src1/C1 mismatch");
  M2H_REQUIRE(a.nth > 0 && a.ntw > 0 && a.stride > 0 && a.os > 0, "conv_igemm: bad taps/stride");
  M2H_REQUIRE(a.Ho > 0 && a.Wo > 0, "conv_igemm: bad output size");
  if (a.conv_transpose) {
    M2H_REQUIRE(a.nth == 2 && a.ntw == 2 && a.stride == 1 && a.os == 2, "conv_igemm: transposed conv is 4x4/s2/p1 (2x2 taps per phase)");
    M2H_REQUIRE(a.Hq == a.Hi && a.Wq == a.Wi && a.Ho == 2 * a.Hi && a.Wo == 2 * a.Wi, "conv_igemm: transposed conv geometry");
  } else {
    M2H_REQUIRE((a.Hq - 1) * a.os + a.ph < a.Ho && (a.Wq - 1) * a.os + a.pw < a.Wo, "conv_igemm: output pixel grid exceeds Ho x Wo");
  }
  M2H_REQUIRE((long)a.B * a.Hq * a.Wq < (1L << 30), "conv_igemm: M too large");
  M2H_REQUIRE((long)a.B * a.Hi * a.Wi < (1L << 30), "conv_igemm: input pixel count too large");
  M2H_REQUIRE((long)a.B * 16 * a.Ho * a.Wo < (1L << 31), "conv_igemm: output pixel count too large");
  M2H_REQUIRE((long)a.B * a.Hi * a.Wi * (a.C0 > a.C1 ? a.C0 : a.C1) < (1L << 32), "conv_igemm: source tensor exceeds 32-bit element offsets");
  M2H_REQUIRE((long)a.N * a.nth * a.ntw * (a.C0 + a.C1) < (1L << 32), "conv_igemm: weight matrix exceeds 32-bit element offsets");
  if (a.out_mode == M2H_OUT_DESLICE) {
    M2H_REQUIRE(a.N % 16 == 0, "conv_igemm: de-slice needs N %% 16 == 0");
  } else {
    M2H_REQUIRE(a.out_mode == M2H_OUT_NHWC && a.ldc >= a.N, "conv_igemm: bad out_mode/ldc");
  }
  M2H_REQUIRE((a.cls_table == nullptr) == (a.cls_val == nullptr), "conv_igemm: cls_table/cls_val mismatch");

  IGemmP p = conv_params(a);
  {
    const int fmt = a.operand_format;
    M2H_REQUIRE((fmt & (M2H_FMT_MATH_BF16X3 | M2H_FMT_MATH_FP32)) != (M2H_FMT_MATH_BF16X3 | M2H_FMT_MATH_FP32),
                "conv_igemm: operand_format names both arithmetic modes");
    M2H_REQUIRE((fmt & (M2H_FMT_SRC_SPLIT | M2H_FMT_W_SPLIT | M2H_FMT_DST_SPLIT)) == 0 || p.math == 1,
                "conv_igemm: split32 operands need the bf16x3 math mode");
    const int both = M2H_FMT_SRC_SPLIT | M2H_FMT_W_SPLIT;
    M2H_REQUIRE((fmt & both) == 0 || (fmt & both) == both, "conv_igemm: sources and weights must be split32 together");
    M2H_REQUIRE(!p.dst_split || (a.out_mode == M2H_OUT_NHWC && a.N % 32 == 0 && a.ldc % 32 == 0 && a.head_w == nullptr),
                "conv_igemm: split32 output needs NHWC, N %% 32 == 0, ldc %% 32 == 0, no fused head");
  }
  if (a.head_w != nullptr) {
    M2H_REQUIRE(a.head_b != nullptr && (a.N == 32 || a.N == 16) && a.out_mode == M2H_OUT_DESLICE && a.workspace == nullptr && a.cls_table == nullptr,
                "conv_igemm: fused head needs N in {16,32}, de-sliced output, no split-K workspace, no class plane");
  }
  if (l1 != nullptr) {
    M2H_REQUIRE(l1->gt && l1->partials && l1->loss && a.N == 16 && a.ldc == 16 && a.out_mode == M2H_OUT_NHWC && a.slope == 1.f && a.scale == nullptr,
                "conv_igemm: the fused L1 loss needs N = 16 NHWC output without scale or activation");
    p.l1_gt = l1->gt; p.l1_part = l1->partials; p.l1_inv = l1->inv;
  }
  M2H_REQUIRE(p.K % 4 == 0, "conv_igemm: K must be a multiple of 4");
  M2H_REQUIRE(!p.presplit || p.fast_ok, "conv_igemm: split32 operands need channel counts that are multiples of 32");
  const size_t wsb = a.workspace != nullptr ? a.workspace_bytes : 0;

  // The engines in order; the first whose rule holds takes the launch (igemm_common.h).
  int rc;
  if ((rc = launch_igemm_patch(p, wsb, st)) != NOT_THIS_ENGINE) return finish_splitk(rc, p, st, "igemm_patch<256,128> + split-K reduce");
  if ((rc = launch_convT_quad(p, st)) != NOT_THIS_ENGINE) return rc;
  if ((rc = launch_convT_tap(p, st)) != NOT_THIS_ENGINE) return rc;
  if ((rc = launch_skinny_rows(p, st)) != NOT_THIS_ENGINE) return rc;
  if ((rc = launch_skinny_gather(p, st)) != NOT_THIS_ENGINE) return rc;
  if ((rc = launch_row3x3(p, l1 != nullptr ? l1->loss : nullptr, st)) != NOT_THIS_ENGINE) return rc;
  M2H_REQUIRE(l1 == nullptr, "conv_igemm: the fused L1 loss is built into the image-row 3x3 kernels only (3x3 / 1 / 1 over 32-channel, 32-pixel-wide images, "
                            "N = 16, B x H / 4 >= 512)");
  if ((rc = launch_igemm_dma(p, wsb, st)) != NOT_THIS_ENGINE) return finish_splitk(rc, p, st, "igemm_dma<256,128> + split-K reduce");
  return launch_igemm_reg(p, wsb, st);
}

}  // namespace m2h
