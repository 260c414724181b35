// Skinny weight-streaming engines (fp32 MFMA, no LDS staging, no split-K): skinny_rows_kernel for M <= 16 rows that are each one
// contiguous run of floats, skinny_gather_kernel for small pixel counts; each with its block-shape choice and its shape rule.
#include "igemm_common.h"

namespace m2h {

// ---------------------------------------------------------------------------------------------------------------------------
// Skinny dense GEMM, M <= 16 rows (fp32 MFMA): D[m][n] = act(scale[n] * sum_k X[m][k] W[n][k] + shift[n]) where every GEMM row is
// one contiguous run of floats -- nn.Linear at the rollout width (the GRU's input projection, 1536 x 1536), the full-spatial
// "conv as Linear" of VisualCNN / AudioCNN (visual_cnn.py:140-141: 4608 -> 512), and the two U-Net stages around the 1 x 1
// bottleneck at the rollout batch: the deepest encoder conv (its tap window covers the whole 2 x 2 input: the sample IS the row)
// and the first transposed conv (one tap per sub-pixel phase).  These are weight streams (4-17 MB against 14 rows): the tiled
// engine needs split-K slabs and a reduce launch to occupy the chip (20-28 us per layer).  Here a block owns COLS output
// channels of one phase; BOTH operands go straight from global memory into v_mfma_f32_16x16x4_f32 registers (lane (row,
// k-quarter) loads 16 bytes of its row: four consecutive MFMAs' worth; X is a few hundred KB and stays in L2), the four waves
// split K, and their partial tiles meet through 4 KB of LDS in wave order.  No LDS staging, no barrier in the k-loop.
// COLS = 16 fills the MFMA tile; COLS = 4 (the other columns repeat the last row) quadruples the block count for N <= 512.
// K is walked as thn segments of twn*Ctot floats: X contiguous, W at tap (th0 + seg, tw0) of its (nth x ntw x Ctot) row.
// NW = waves per block (4, 8 or 16): they split the walked reduction, so a long K over few blocks is a short chain per wave.
template <int COLS, int NW>
__global__ __launch_bounds__(64 * NW) void skinny_rows_kernel(const IGemmP p) {
  __shared__ float R[NW][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int nblk = (p.N + COLS - 1) / COLS;
  const int phase = blockIdx.x / nblk;
  const int n0 = (blockIdx.x - phase * nblk) * COLS;
  const int L = p.twn * p.Ctot;                               // floats per segment
  const int sps = L >> 4;                                     // 16-float steps per segment
  const int steps = p.thn * sps;
  const int s0 = (steps * wave) / NW, s1 = (steps * (wave + 1)) / NW;
  const float* xr = p.src0 + (size_t)min(i, p.M - 1) * ((size_t)p.thn * L) + 4 * kq;   // rows past M re-read row M-1 (never stored)
  const float* wr = p.w + ((size_t)phase * p.N + min(n0 + min(i, COLS - 1), p.N - 1)) * p.K + (size_t)p.tw0 * p.Ctot + 4 * kq;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int seg = s0 / sps, s = s0 - seg * sps;
#pragma unroll 8
  for (int t = s0; t < s1; ++t) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(xr + (size_t)seg * L + 16 * s);
    const f32x4 b = *reinterpret_cast<const f32x4*>(wr + (size_t)(p.th0 + seg) * p.ntw * p.Ctot + 16 * s);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
    if (++s == sps) {
      s = 0;
      ++seg;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) R[wave][kq * 4 + e][i] = acc[e];   // D[m = kq*4 + e][column i]
  __syncthreads();
  const int m = tid >> 4, c = tid & 15, n = n0 + c;
  if (tid < 256 && m < p.M && c < COLS && n < p.N) {
    float x = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) x += R[w][m][c];              // wave order
    const float sc = p.scale != nullptr ? p.scale[n] : 1.f;
    const float sh = p.shift != nullptr ? p.shift[n] : 0.f;
    x = x * sc + sh;
    const size_t pix = p.convT ? ((size_t)m * p.Ho + (phase >> 1)) * p.Wo + (phase & 1) : (size_t)m;
    p.dst[pix * p.ldc + n] = x > 0.f ? x : x * p.slope;
  }
}

// Skinny implicit-GEMM conv for small pixel counts (M <= 1024 rows per phase: the U-Net's deeper stages at the rollout batch, the
// policy's Linear layers over a 280-sample update batch), fp32
// MFMA, no LDS staging: a block computes a 16*MGB (pixels) x 16 (channels) tile of one phase; lane (row i, k-quarter) loads 16 bytes
// of its weight row and of each of its MGB pixel rows (gathered per tap exactly as the register engine does, zero outside the image;
// the activations are a few hundred KB and stay in L1 / L2) straight into v_mfma_f32_16x16x4_f32 registers; the four waves split
// the walked reduction (tap window x both sources x channels) and meet through LDS in wave order; BN scale / shift, activation
// and the NHWC store follow.  The tiled engine occupies the chip at these sizes only through split-K (slabs + a reduce launch,
// 24-45 us per layer against 2-17 MB of weights); here the weights are streamed MG/MGB times and the activations N/16 times.
// NCG = 16-column groups per block (1; 2 for the update batch's wide Linear layers: the activations' share of the L2 -> CU stream, one pass per
// column block, halves)
template <int MGB, int NW, int NCG = 1>
__global__ __launch_bounds__(64 * NW) void skinny_gather_kernel(const IGemmP p) {
  __shared__ float R[NW][MGB * NCG][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int NB = (p.N + 16 * NCG - 1) / (16 * NCG), MS = (p.MT + MGB - 1) / MGB;     // p.MT = 16-row groups of M
  int L = blockIdx.x;
  const int ms = L % MS;
  L /= MS;
  const int nb = L % NB, phase = L / NB;
  int mulh = p.mulh, offh = p.offh, mulw = p.mulw, offw = p.offw, ph = p.ph, pw = p.pw;
  const float* wbase = p.w;
  if (p.convT) {
    ph = phase >> 1;
    pw = phase & 1;
    mulh = 2 * ph - 1;
    mulw = 2 * pw - 1;
    offh = 0;
    offw = 0;
    wbase += (size_t)phase * p.N * p.K;
  }
  int qh[MGB], rw[MGB], bpix[MGB];
#pragma unroll
  for (int g = 0; g < MGB; ++g) {
    const int m = (ms * MGB + g) * 16 + i;
    qh[g] = rw[g] = -(1 << 24);
    bpix[g] = 0;
    if (m < p.M) {
      int q, rr, b, out, bc;
      decode_row(p, m, ph, pw, q, rr, b, out, bc);
      qh[g] = q * p.stride + offh;
      rw[g] = rr * p.stride + offw;
      bpix[g] = b * p.Hi * p.Wi;
    }
  }
  const float* wrow[NCG];
#pragma unroll
  for (int cg = 0; cg < NCG; ++cg) wrow[cg] = wbase + (size_t)min((nb * NCG + cg) * 16 + i, p.N - 1) * p.K + 4 * kq;
  const int spt = p.Ctot >> 4;                                   // 16-float steps per tap
  const int steps = p.thn * p.twn * spt;
  const int s0 = (steps * wave) / NW, s1 = (steps * (wave + 1)) / NW;
  f32x4 acc[MGB][NCG];
#pragma unroll
  for (int g = 0; g < MGB; ++g)
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) acc[g][cg] = {0.f, 0.f, 0.f, 0.f};
  int tap = s0 / spt, ci = (s0 - tap * spt) * 16;
  int th = p.th0 + tap / p.twn, tw = p.tw0 + tap % p.twn;
  unsigned offA[MGB];                                            // float offset of the row's pixel at the current tap, per source stride
  bool okA[MGB];
  auto at_tap = [&]() {
#pragma unroll
    for (int g = 0; g < MGB; ++g) {
      const int ih = qh[g] + th * mulh, iw = rw[g] + tw * mulw;
      okA[g] = (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
      offA[g] = okA[g] ? (unsigned)(bpix[g] + ih * p.Wi + iw) : 0u;
    }
  };
  at_tap();
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int t = s0; t < s1;) {
    // one run of steps inside the current (tap, source): addresses advance by 16 floats, no branches -> the loads of the next
    // steps are issued under the MFMAs of the current ones
    const bool second = ci >= p.C0;
    const int seg_end = second ? p.Ctot : p.C0;                  // end of this source's channels
    const int nrun = min(s1 - t, (seg_end - ci) >> 4);
    const float* src = second ? p.src1 : p.src0;
    const unsigned Cs = second ? p.C1 : p.C0, c = (second ? ci - p.C0 : ci) + 4 * kq;
    const size_t wofs = (size_t)(th * p.ntw + tw) * p.Ctot + ci;
    const float* ap[MGB];
#pragma unroll
    for (int g = 0; g < MGB; ++g) ap[g] = src + (size_t)offA[g] * Cs + c;   // (rows outside the image: pixel 0, masked below)
#pragma unroll 4
    for (int k = 0; k < nrun; ++k) {
      f32x4 b[NCG];
#pragma unroll
      for (int cg = 0; cg < NCG; ++cg) b[cg] = *reinterpret_cast<const f32x4*>(wrow[cg] + wofs + 16 * k);
      f32x4 a[MGB];
#pragma unroll
      for (int g = 0; g < MGB; ++g) a[g] = *reinterpret_cast<const f32x4*>(ap[g] + 16 * k);
#pragma unroll
      for (int g = 0; g < MGB; ++g) {
        const f32x4 av = okA[g] ? a[g] : zero4;
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[g][cg] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b[cg][j], acc[g][cg], 0, 0, 0);
      }
    }
    t += nrun;
    ci += 16 * nrun;
    if (ci == p.Ctot) {
      ci = 0;
      if (++tw == p.tw0 + p.twn) {
        tw = p.tw0;
        ++th;
      }
      at_tap();
    }
  }
#pragma unroll
  for (int g = 0; g < MGB; ++g)
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg)
#pragma unroll
      for (int e = 0; e < 4; ++e) R[wave][g * NCG + cg][kq * 4 + e][i] = acc[g][cg][e];    // D[row kq*4 + e][channel i]
  __syncthreads();
#pragma unroll
  for (int gc = 0; gc < MGB * NCG; ++gc) {
    const int g = gc / NCG, cg = gc % NCG;
    const int r16 = tid >> 4, c16 = tid & 15;
    const int m = (ms * MGB + g) * 16 + r16, n = (nb * NCG + cg) * 16 + c16;
    if (tid < 256 && m < p.M && n < p.N) {
      float x = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) x += R[w][gc][r16][c16];       // wave order
      int q, rr, b, out, bc;
      decode_row(p, m, ph, pw, q, rr, b, out, bc);
      if (p.cls_table != nullptr) x += p.cls_val[bc >> 4] * p.cls_table[(size_t)(bc & 15) * p.N + n];   // the class plane (as the tiled engine's epilogues)
      const float sc = p.scale != nullptr ? p.scale[n] : 1.f;
      const float sh = p.shift != nullptr ? p.shift[n] : 0.f;
      x = x * sc + sh;
      p.dst[(size_t)out * p.ldc + n] = x > 0.f ? x : x * p.slope;
    }
  }
}

// waves per block of the skinny kernels: they split the walked reduction, and a wave's share is a chain of dependent load rounds
// (runs of at most Ctot / 16 steps between tap changes), so short shares win: more than 32 steps -> 16 waves, more than 16 -> 8
// (A/B on one box, tools/train_ab.sh: rollout 74.2 -> 71.6 ms per cycle against the round-2 thresholds 160 / 80)
static int skinny_waves(int steps) { return steps > 32 ? 16 : (steps > 16 ? 8 : 4); }
// fewer blocks than this leave most CUs without one: the skinny kernels then take their smaller blocks (16 rows / two columns)
constexpr long SKINNY_MIN_BLOCKS = 192;

// M <= 16 rows that are each one contiguous run of floats: Linear; a conv whose tap window covers the whole image and gives
// one output pixel; a transposed conv over a 1 x 1 image (one tap per phase).  Weight streaming on the skinny kernel, from 16 K weights
// (round 5; was 256 K: the fused audio pair's third conv and Linear at the rollout batch took a tiled launch + split-K reduce / a 32-row
// tile for 14 rows).
int launch_skinny_rows(IGemmP& p, hipStream_t st) {
  if (!(p.math == 0 && g_skinny_linear >= 0 && p.fast_ok && p.M <= 16 && p.C1 == 0 && p.Hq == 1 && p.Wq == 1 && p.os >= 1 && p.N % 4 == 0 &&
        p.out_mode == M2H_OUT_NHWC && p.cls_table == nullptr && p.head_w == nullptr && !p.presplit && !p.dst_split &&
        (size_t)p.N * p.Kw * (p.convT ? 4 : 1) >= ((size_t)1 << 14)))
    return NOT_THIS_ENGINE;
  bool dense;
  if (p.convT) dense = p.Hi == 1 && p.Wi == 1 && p.thn == 1 && p.twn == 1 && p.th0 == 0 && p.tw0 == 0 && p.Ho == 2 && p.Wo == 2;
  else dense = p.Ho == 1 && p.Wo == 1 && p.ph == 0 && p.pw == 0 && p.thn == p.Hi && p.twn == p.Wi && p.mulh == 1 && p.mulw == 1 &&
               p.offh + p.th0 == 0 && p.offw + p.tw0 == 0;
  if (!dense) return NOT_THIS_ENGINE;
  const int phases = p.convT ? 4 : 1;
  const int nw = skinny_waves(p.Kw / 16);
  const bool wide = p.N * phases >= 64 * 16;
  // two columns per block where four would leave most CUs without a block (N = 512 of one phase: 128 blocks): as the skinny gather
  // kernel's 16-row blocks, the weights stream at a per-CU rate.  Same values (a column's sum does not depend on its neighbours).
  const bool two = !wide && p.N % 2 == 0 && (long)phases * ((p.N + 3) / 4) < SKINNY_MIN_BLOCKS;
  const dim3 grid((unsigned)(phases * (wide ? (p.N + 15) / 16 : two ? (p.N + 1) / 2 : (p.N + 3) / 4))), blk(64 * nw);
#define M2H_SKINNY_ROWS(NW_)                                                        \
  do {                                                                              \
    if (wide) M2H_LAUNCH((skinny_rows_kernel<16, NW_>), grid, blk, 0, st, p);       \
    else if (two) M2H_LAUNCH((skinny_rows_kernel<2, NW_>), grid, blk, 0, st, p);    \
    else M2H_LAUNCH((skinny_rows_kernel<4, NW_>), grid, blk, 0, st, p);             \
  } while (0)
  if (nw == 4) M2H_SKINNY_ROWS(4);
  else if (nw == 8) M2H_SKINNY_ROWS(8);
  else M2H_SKINNY_ROWS(16);
#undef M2H_SKINNY_ROWS
  return launch_status("conv_igemm_f32 (skinny rows)");
}

// small pixel counts per phase (<= 1024; knob 24 > 0 overrides the limit): 32 x 16 tiles without LDS staging or split-K.
// Also 1024 < M <= 4096 pixels against TINY weights (< 64 K elements: the rollout batch's first encoder stage, 3584 pixels x 512 x 64, and the
// visual encoder's second and third convs): the tiled engine fills the chip there only through split-K slabs + a reduce launch (10 + 5 us
// for 0.2 GFLOP)
int launch_skinny_gather(IGemmP& p, hipStream_t st) {
  const bool tiny_w = (size_t)p.N * p.Kw * (p.convT ? 4 : 1) < ((size_t)1 << 16);
  const long skinny_lim = g_skinny_gather > 0 ? g_skinny_gather : (tiny_w ? 4096 : 1024);
  if (!(p.math == 0 && g_skinny_gather >= 0 && p.fast_ok && p.M > 16 && p.M <= skinny_lim &&
        p.N % 16 == 0 && p.out_mode == M2H_OUT_NHWC && p.head_w == nullptr && !p.presplit && !p.dst_split &&
        p.Ctot % 16 == 0 && (tiny_w ? p.M > 1024 : p.cls_table == nullptr)))
    return NOT_THIS_ENGINE;
  const int phases = p.convT ? 4 : 1;
  p.MT = (p.M + 15) / 16;
  const long blocks2 = (long)phases * (p.N / 16) * ((p.MT + 1) / 2);
  const int nw = skinny_waves(p.Kw / 16);
  // 32 pixel rows per block where that fills the chip; 16 where it would leave most CUs without a block (the deep U-Net stages at the
  // rollout batch: 56 rows x 512 channels = 64 blocks of 32 rows): the weights stream at a per-CU rate, so twice the blocks stream them
  // twice as fast, and their second read comes out of L2.  Same values: a row's sum does not depend on the rows beside it.
  const bool one = p.MT >= 2 && blocks2 < SKINNY_MIN_BLOCKS;
  // 64 rows x 32 columns per block (eight waves) where that still gives the chip a block per CU (the update batch's 280-row Linear layers
  // against 1536 / 4608 columns: 864 / 2592 blocks of 32 x 16): such a launch is bound by the L2 -> CU operand stream -- the weights
  // pass once per row block, the activations once per column block -- and both shares halve
  const long blocks4 = (long)phases * ((p.N + 31) / 32) * ((p.MT + 3) / 4);   // 64 rows x 32 columns
  // (both wide forms for ONE-pixel outputs only -- nn.Linear and the encoders' full-spatial convs over the update batch, where they were measured:
  // 38 -> 25, 35 -> 31, 37 -> 26, 55 -> 41 us per policy epoch; on the passive step's U-Net stages of 256-1024 pixels they measured 2 % slower)
  const bool dense = p.Hq == 1 && p.Wq == 1 && !p.convT;
  const bool four = dense && !one && p.MT >= 8 && blocks4 >= 240;
  const long blocks2w = (long)phases * ((p.N + 31) / 32) * ((p.MT + 1) / 2);   // 32 rows x 32 columns (the 280-row layers against 512 columns)
  const bool wide2 = dense && !one && !four && p.MT >= 8 && blocks2w >= 128;
  const long blocks = four ? blocks4 : (wide2 ? blocks2w : (one ? (long)phases * (p.N / 16) * p.MT : blocks2));
#define M2H_SKINNY_GATHER(NW_)                                                                              \
  do {                                                                                                      \
    if (four) M2H_LAUNCH((skinny_gather_kernel<4, (NW_ > 8 ? 8 : NW_), 2>), dim3((unsigned)blocks), dim3(64 * (NW_ > 8 ? 8 : NW_)), 0, st, p); \
    else if (wide2) M2H_LAUNCH((skinny_gather_kernel<2, NW_, 2>), dim3((unsigned)blocks), dim3(64 * NW_), 0, st, p); \
    else if (one) M2H_LAUNCH((skinny_gather_kernel<1, NW_>), dim3((unsigned)blocks), dim3(64 * NW_), 0, st, p);  \
    else M2H_LAUNCH((skinny_gather_kernel<2, NW_>), dim3((unsigned)blocks), dim3(64 * NW_), 0, st, p);      \
  } while (0)
  if (nw == 4) M2H_SKINNY_GATHER(4);
  else if (nw == 8) M2H_SKINNY_GATHER(8);
  else M2H_SKINNY_GATHER(16);
#undef M2H_SKINNY_GATHER
  return launch_status("conv_igemm_f32 (skinny gather)");
}

}  // namespace m2h
