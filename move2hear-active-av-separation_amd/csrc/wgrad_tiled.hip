// Weight gradient, the tiled kernel (gfx950, fp32 MFMA): every shape the image-row kernels do not take.
//
// Tiling: block = BNG (n) x 128*KT (k) output tile, 4 waves, fp32 v_mfma_f32_32x32x2; the reduction runs over 32-pixel
// chunks staged [m][n] / [m][k] in LDS (prefetched through registers); fragments are ds_read_b32 column reads
// (consecutive lanes -> consecutive addresses, conflict free).  The pixel range is split over grid.z; partial tiles go to a
// slab [split][N][Kpad] and an ordered reduce kernel sums them (deterministic, no atomics).
#include "wgrad_common.h"

namespace m2h {

// BNG = n extent of the block (32 | 128); KT = number of 128-wide k sub-tiles of the block (k extent 128*KT).
// Narrow layers (N <= 32) would give a wave ONE 32x32 fragment per chunk (16 MFMAs beside ~300 other instructions: the first
// version ran issue-bound at 30 % matrix-pipe utilisation); with KT = 2 or 3 a wave owns KT fragments that share one dY
// operand, the input rows are fetched once per chunk instead of once per k-tile, and the row bookkeeping is amortised.
// NST = LDS stages (2: one barrier per chunk; 1: two barriers, for the wide-k blocks whose tile would not fit twice).
template <int BNG, int KT, int NST>
__global__ __launch_bounds__(256) void wgrad_kernel(const WGradP p) {
  constexpr int WKB = WK * KT;                    // k extent of the block
  constexpr int WN_ = (BNG == 128) ? 2 : 1;       // waves along n
  constexpr int WK_ = 4 / WN_;                    // waves along k
  constexpr int TN = BNG / WN_, TK = WKB / WK_;   // wave tile
  constexpr int FN = TN / 32, FK = TK / 32;
  constexpr int YSEG = BNG / 4;                   // 16-byte segments per dY row
  constexpr int YR = (WM * YSEG + 255) / 256;     // dY segments per thread
  constexpr int YSTEP = 256 / YSEG;
  static_assert(TK % 32 == 0 && FK >= 1, "wave k extent must be whole fragments");
  __shared__ __attribute__((aligned(16))) float Ys[NST][WM * BNG];
  __shared__ __attribute__((aligned(16))) float As[NST][WM * WKB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave / WK_, wk = wave % WK_;
  const WPhase wp_ = wgrad_phase(p);
  // 1-D grid, XCD-aware: the (n-tile, k-tile) blocks of one pixel split are consecutive blocks of ONE XCD (L % 8), so the
  // split's input rows and dY rows meet in that XCD's L2
  const int L = blockIdx.x;
  const int tiles = p.ntiles * p.ktiles;
  int tile, split;
  if (p.S >= 8) {
    const int idx = L >> 3;
    tile = idx % tiles;
    split = (idx / tiles) * 8 + (L & 7);
    if (split >= p.S) return;  // padding blocks of the XCD map (whole block, before any barrier)
  } else {  // few splits (short M): plain order, tiles spread over all XCDs
    tile = L % tiles;
    split = L / tiles;
  }
  const int n0 = (tile / p.ktiles) * BNG;
  const int k0 = (tile % p.ktiles) * WKB;
  const int c0 = (int)(((long)p.chunks * split) / p.S), c1 = (int)(((long)p.chunks * (split + 1)) / p.S);

  // this thread's fixed A columns (one per k sub-tile): decode (tap, channel) once
  const int aseg = tid & 31;  // 32 segments of 4 floats = 128 k
  const int arow = tid >> 5;  // 0..7, rows arow + 8*i
  bool kok[KT];
  int dh[KT], dw[KT], Cs[KT], cc[KT];
  const float* src[KT];
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    const int k = k0 + c * WK + aseg * 4;
    kok[c] = k < p.K;
    int tap = 0, ci = k;
    if (p.ntap > 1) {
      tap = (unsigned)k / (unsigned)p.Ctot;
      ci = k - tap * p.Ctot;
    }
    const int th = (unsigned)tap / (unsigned)p.ntw, tw = tap - th * p.ntw;
    dh[c] = th * wp_.mulh + p.offh;
    dw[c] = tw * wp_.mulw + p.offw;
    src[c] = p.src0;
    Cs[c] = p.C0;
    cc[c] = ci;
    if (ci >= p.C0 && p.src1 != nullptr) {  // (padding columns k >= K of a single-source conv keep src0: their loads are masked, not skipped)
      src[c] = p.src1;
      Cs[c] = p.C1;
      cc[c] = ci - p.C0;
    }
  }
  const int yseg = tid % YSEG, yrow0 = tid / YSEG;  // dY: rows yrow0 + YSTEP*i

  f32x16 acc[FN][FK];
#pragma unroll
  for (int a = 0; a < FN; ++a)
#pragma unroll
    for (int b = 0; b < FK; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  f32x4 ra[4][KT], ry[YR];
  unsigned okm = 0;  // validity bits of the staged registers (A: bit i*KT+c, dY: bit 16+i); selects happen at the LDS write
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // Row state (b, q, r) of the rows this thread stages, advanced by 32 pixels per chunk WITHOUT divisions.
  // 32 = d_b * Hq*Wq + d_q * Wq + d_r  (uniform), so one conditional carry per digit suffices.
  const int d_r = WM % p.Wq, d_q = (WM / p.Wq) % p.Hq, d_b = WM / (p.Wq * p.Hq);
  struct Row { int m, b, q, r; };
  auto row_init = [&](int m) {
    Row w;
    w.m = m;
    w.r = m % p.Wq;
    const int t = m / p.Wq;
    w.q = t % p.Hq;
    w.b = t / p.Hq;
    return w;
  };
  auto row_next = [&](Row& w) {
    w.m += WM;
    w.r += d_r;
    const int c1_ = w.r >= p.Wq ? 1 : 0;
    w.r -= c1_ ? p.Wq : 0;
    w.q += d_q + c1_;
    const int c2_ = w.q >= p.Hq ? 1 : 0;
    w.q -= c2_ ? p.Hq : 0;
    w.b += d_b + c2_;
  };
  Row rowA[4], rowY[YR];
#pragma unroll
  for (int i = 0; i < 4; ++i) rowA[i] = row_init(c0 * WM + arow + 8 * i);
#pragma unroll
  for (int i = 0; i < YR; ++i) rowY[i] = row_init(c0 * WM + yrow0 + YSTEP * i);
  const int ny = n0 + yseg * 4;
  const bool yvec = ny + 3 < p.N && (p.ldy & 3) == 0;

  // loads the chunk the row state points at (unconditional loads from a clamped offset; no divergent branches), then advances
  auto load_chunk = [&]() {
    okm = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const Row& w = rowA[i];
      const int bpix = w.b * p.Hi * p.Wi, qs = w.q * p.stride, rs = w.r * p.stride;
      const bool rok = w.m < p.M;
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        const int ih = qs + dh[c], iw = rs + dw[c];
        const bool ok = kok[c] && rok && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
        const size_t off = ok ? ((size_t)(bpix + ih * p.Wi + iw)) * (size_t)Cs[c] + (size_t)cc[c] : (size_t)0;
        ra[i][c] = *reinterpret_cast<const f32x4*>(src[c] + off);
        okm |= ok ? (1u << (i * KT + c)) : 0u;
      }
      row_next(rowA[i]);
    }
#pragma unroll
    for (int i = 0; i < YR; ++i) {
      const Row& w = rowY[i];
      const int row = yrow0 + YSTEP * i;
      const bool ok = row < WM && w.m < p.M && ny < p.N;
      size_t pix = (size_t)w.m;
      if (!p.direct) pix = ((size_t)w.b * p.Ho + (size_t)(w.q * p.os + wp_.ph)) * p.Wo + (size_t)(w.r * p.os + wp_.pw);
      const float* yp = p.dy + (ok ? pix * p.ldy + ny : (size_t)0);
      if (yvec) {
        ry[i] = *reinterpret_cast<const f32x4*>(yp);
      } else {  // ragged N or unaligned rows (heads): scalar tail, block-uniform branch
        ry[i] = zero4;
        if (ok)
          for (int j = 0; j < 4; ++j)
            if (ny + j < p.N) ry[i][j] = yp[j];
      }
      okm |= ok ? (1u << (16 + i)) : 0u;
      row_next(rowY[i]);
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < KT; ++c)
        *reinterpret_cast<f32x4*>(&As[buf][(arow + 8 * i) * WKB + c * WK + aseg * 4]) = (okm & (1u << (i * KT + c))) ? ra[i][c] : zero4;
#pragma unroll
    for (int i = 0; i < YR; ++i) {
      const int row = yrow0 + YSTEP * i;
      if (row < WM) *reinterpret_cast<f32x4*>(&Ys[buf][row * BNG + yseg * 4]) = (okm & (1u << (16 + i))) ? ry[i] : zero4;
    }
  };
  const int fi = lane & 31, fh = lane >> 5;
  // The fragment reads of half a chunk are issued together and the MFMAs follow (the first version's read -> wait -> MFMA
  // chain exposed the LDS latency 16 times per chunk).
  auto compute = [&](int buf) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      float av[WM / 4][FN], bv[WM / 4][FK];
#pragma unroll
      for (int j = 0; j < WM / 4; ++j) {
        const int m = 2 * (half * (WM / 4) + j) + fh;
#pragma unroll
        for (int x = 0; x < FN; ++x) av[j][x] = Ys[buf][m * BNG + wn * TN + x * 32 + fi];
#pragma unroll
        for (int x = 0; x < FK; ++x) bv[j][x] = As[buf][m * WKB + wk * TK + x * 32 + fi];
      }
#pragma unroll
      for (int j = 0; j < WM / 4; ++j)
#pragma unroll
        for (int x = 0; x < FN; ++x)
#pragma unroll
          for (int y = 0; y < FK; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j][x], bv[j][y], acc[x][y], 0, 0, 0);
    }
  };

  if (c0 < c1) {
    load_chunk();
    store_chunk(0);
    __syncthreads();
    if constexpr (NST == 2) {
      int cur = 0;
      for (int c = c0; c + 1 < c1; ++c) {  // straight-line body; the last chunk is peeled
        load_chunk();
        compute(cur);
        store_chunk(cur ^ 1);
        __syncthreads();
        cur ^= 1;
      }
      compute(cur);
    } else {
      for (int c = c0; c + 1 < c1; ++c) {
        load_chunk();
        compute(0);
        __syncthreads();  // everyone is done reading the stage
        store_chunk(0);
        __syncthreads();
      }
      compute(0);
    }
  }

  // partial tile -> slab[split][n][k]
  float* slab = p.ws + wp_.ws_off + (size_t)split * p.N * p.Kpad;
  const int col = lane & 31, rhalf = (lane >> 5) * 4;
#pragma unroll
  for (int x = 0; x < FN; ++x)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = n0 + wn * TN + x * 32 + (e & 3) + 8 * (e >> 2) + rhalf;
      if (n >= p.N) continue;
#pragma unroll
      for (int y = 0; y < FK; ++y) {
        const int kk = k0 + wk * TK + y * 32 + col;
        if (kk < p.Kpad) slab[(size_t)n * p.Kpad + kk] = acc[x][y][e];
      }
    }
}

// block shape for (N, K): n extent, k sub-tiles per block, blocks along k
void wgrad_cfg(int N, int K, int& bng, int& kt, int& ktiles, long M) {
  const int kt128 = (K + WK - 1) / WK;
  bng = N > 64 ? 128 : (N > 32 ? 64 : 32);        // (64: round 4 -- a 64-channel layer on the 128-wide block spent half its MFMAs on padding)
  // a few hundred rows (the update batch's Linear layers: 280 x 1536 x 1536): the reduction is nine chunks long and a block's time is its
  // MFMAs -- 64-wide blocks, twice as many, each half as long: 33 -> 28, 21 -> 14, 31 -> 27 us per policy epoch (knob 25 = -1: the 128-wide blocks)
  if (M <= 1024 && N > 64 && K <= 2048 && g_wgrad_small_m >= 0) bng = 64;   // (K <= 2048: the 4608-deep full-spatial conv re-reads its input rows once per n-block: 34 -> 54 us)
  kt = bng == 32 ? (kt128 >= 3 ? 3 : kt128) : (bng == 64 ? (kt128 >= 2 && N <= 64 ? 2 : 1) : 1);  // narrow layers: up to three k sub-tiles per block share the dY operand
  // ... unless two sub-tiles per block leave fewer padding columns (K = 512: two blocks of 256 instead of two of 384 -- the last decoder
  // stage's weight gradient, 65 536 pixels x 512 x 16 | 32, spent a third of its MFMAs and input loads on columns beyond K; knob 12 = -1: the old rule)
  if (bng == 32 && kt == 3 && g_wgrad_kt3 >= 0 && ((kt128 + 1) / 2) * 2 < ((kt128 + 2) / 3) * 3) kt = 2;
  ktiles = (kt128 + kt - 1) / kt;
}

int launch_wgrad_tiled(WGradP& p, hipStream_t st) {
  int bng, kt, ktiles;
  wgrad_cfg(p.N, p.K, bng, kt, ktiles, p.M);
  const long nblk = (long)(p.S >= 8 ? (p.S + 7) / 8 * 8 : p.S) * p.ntiles * p.ktiles;
  M2H_REQUIRE(nblk < 0x7fffffffL, "conv_wgrad: grid too large");
  const dim3 grid((unsigned)nblk, p.quad ? 4u : 1u), blk(256);
  if (bng == 128) M2H_LAUNCH((wgrad_kernel<128, 1, 2>), grid, blk, 0, st, p);
  else if (bng == 64 && kt == 2) M2H_LAUNCH((wgrad_kernel<64, 2, 1>), grid, blk, 0, st, p);
  else if (bng == 64) M2H_LAUNCH((wgrad_kernel<64, 1, 2>), grid, blk, 0, st, p);
  else if (kt == 1) M2H_LAUNCH((wgrad_kernel<32, 1, 2>), grid, blk, 0, st, p);
  else if (kt == 2) M2H_LAUNCH((wgrad_kernel<32, 2, 1>), grid, blk, 0, st, p);
  else M2H_LAUNCH((wgrad_kernel<32, 3, 1>), grid, blk, 0, st, p);
  return launch_status("conv_wgrad");
}

}  // namespace m2h
