// Tap-sharing transposed-conv engine: convT_tap_kernel, its 128- / 256-output tile choice and its shape rule.
#include "igemm_common.h"

namespace m2h {

// Tap-sharing transposed-conv kernel (bf16x3 math, N <= 64): one sub-pixel phase of ConvTranspose2d(4, 2, 1) is a 2x2-tap
// stride-1 conv, and its four taps read the SAME input pixels shifted by one row / one column.  The register-staged engine
// (conv_igemm.hip) treats each tap as its own k-tile and fetches the 128-pixel operand tile four times; with the cheap bf16 products that
// re-fetch (L1/TA traffic, splits, LDS writes, barriers) is what the narrow late decoder stages spend their time on.  Here a
// k-step is a 32-CHANNEL chunk: the block stages the (R+1) x (Wq+1) input pixels its 128 output pixels touch ONCE per chunk
// (R = 128 / Wq image rows), plus the four taps' weight rows, and runs the four taps' MFMAs from row-shifted windows of that
// one LDS image.  Per thread the global offsets are fixed for the whole kernel (only a uniform channel base advances).
// Requires: conv_transpose, FAST channels, 128 % Wq == 0, Wq >= 32, Hq % (128 / Wq) == 0.  Tile, accumulators and epilogue
// (incl. the fused head) are those of igemm_f32_kernel<128, BN, 4, 1, *, FR, 1, 1>.
template <int BN, int FR, int PRE = 0, int BM = 128, int WM = 4>   // PRE: operands already in the split32 layout (plain copies into LDS)
__global__ __launch_bounds__(64 * WM, WM == 4 ? 2 : 1) void convT_tap_kernel(const IGemmP p) {
  // BM = 256 (two image rows of 128, ...): the staged image grows by one row instead of doubling and the weight rows are
  // shared by twice the outputs -- the kernel is bound by L2 -> LDS traffic (PMC: 49 % of wave cycles parked on waits,
  // matrix pipe 24 % busy), so bytes per output are what counts.
  // WM = 8 (512 threads, one block per CU, twice the outputs per block): the same wave tiles, but the staged image has one halo
  // row per 2 x as many rows and the weight rows serve 2 x the outputs: ~25 % fewer L2 -> LDS bytes per output.
  constexpr int WN = 1, NT = 64 * WM, RPP = NT / 8;
  constexpr int TM = BM / WM;                    // rows per wave
  constexpr int FM = TM / FR, FN = BN / FR;
  constexpr int GK = FR == 32 ? 8 : 16;
  constexpr int NG = BK / GK, NSTEP = NG / 2;
  constexpr int NE = FR == 32 ? 16 : 4;
  using AccT = typename std::conditional<FR == 32, f32x16, f32x4>::type;
  constexpr int PMAX = (BM / 128 + 1) * 129;     // staged input pixels: (R+1)*(Wq+1) <= this for Wq in {32, 64, 128}
  constexpr int AR = (PMAX * 8 + NT - 1) / NT;   // 16-byte loads per thread for the input image
  constexpr int BROWS = 4 * BN;                  // weight rows per chunk (4 taps x BN channels)
  constexpr int BRL = BROWS * 8 / NT;            // loads per thread for them
  static_assert(BROWS * 8 % NT == 0 && FM >= 1 && FN >= 1, "tile shape");
  __shared__ __attribute__((aligned(16))) float As[PMAX * LDK];
  __shared__ __attribute__((aligned(16))) float Bs[BROWS * LDK];
  __shared__ int ri_out[BM], ri_bc[BM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane & (FR - 1);
  const int fk = (lane / FR) * 4;
  const int seg = tid & 7, srow = tid >> 3;

  // ---- block -> (m-tile, phase): phase fastest, m-tiles round-robin over the XCDs ----
  const int L = blockIdx.x;
  const int xcd = L & 7;
  int idx = L >> 3;
  const int phase = idx & 3;
  idx >>= 2;
  const int mt = idx * 8 + xcd;
  if (mt >= p.MT) return;
  const int m0 = mt * BM;
  const int ph = phase >> 1, pw = phase & 1;
  const int dh = 2 * ph - 1, dw = 2 * pw - 1;
  const int hoff = dh < 0 ? dh : 0, woff = dw < 0 ? dw : 0;
  const float* wbase = p.w + (size_t)phase * p.N * p.K;
  const int Wq = p.Wq, W1 = Wq + 1;
  const int R = BM / Wq;
  const int P = (R + 1) * W1;
  const int b0 = m0 / (p.Hq * Wq);
  const int q0 = (m0 / Wq) % p.Hq;

  for (int r = tid; r < BM; r += NT) {
    const int m = m0 + r;
    int out = -1, bc = 0;
    if (m < p.M) {
      int q, rr, b;
      decode_row(p, m, ph, pw, q, rr, b, out, bc);
    }
    ri_out[r] = out;
    ri_bc[r] = bc;
  }

  // ---- fixed per-thread geometry of the staged input image and weight rows ----
  int pixA[AR];        // input pixel index (b, ih, iw) of staged row l = srow + 32 i, or -1
  unsigned voffA[AR], voffB[BRL];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int l = srow + RPP * i;
    const int qi = l / W1, rr = l - qi * W1;
    const int ih = q0 + qi + hoff, iw = rr + woff;
    const bool ok = l < P && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi && b0 < p.B;
    pixA[i] = ok ? (b0 * p.Hi + ih) * p.Wi + iw : -1;
  }
#pragma unroll
  for (int j = 0; j < BRL; ++j) {
    const int row = srow + RPP * j;               // tap * BN + n
    const int tap = row / BN, n = min(row - tap * BN, p.N - 1);   // rows past N re-read row N-1 (never stored)
    voffB[j] = ((unsigned)n * (unsigned)p.K + (unsigned)(tap * p.Ctot + seg * 4)) * 4u;
  }
  auto set_source = [&](int second) {
    const int Cs = second ? p.C1 : p.C0;
#pragma unroll
    for (int i = 0; i < AR; ++i) voffA[i] = pixA[i] >= 0 ? ((unsigned)pixA[i] * (unsigned)Cs + (unsigned)(seg * 4)) * 4u : 0u;
  };

  AccT acc[FM][FN];
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[mi][ni][e] = 0.f;

  // LDS rows of this lane's fragments for tap (0,0)-relative addressing: row(qi, r) = qi*W1 + r, tap adds (a*W1 + b)
  int fragrow[FM];
#pragma unroll
  for (int mi = 0; mi < FM; ++mi) {
    const int ml = wave * TM + mi * FR;          // first tile row of the fragment; FR <= Wq keeps it inside one image row
    fragrow[mi] = (ml / Wq) * W1 + (ml % Wq) + frow;
  }
  int tapoff[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) tapoff[t] = ((t >> 1) * dh - hoff) * W1 + ((t & 1) * dw - woff);

  f32x4 ra[AR], rb[BRL];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  int c_ci = 0, c_second = 0, c_k = 0;           // channel offset inside the source, source, chunk index (uniform)
  auto load_chunk = [&]() {
    const char* baseA = reinterpret_cast<const char*>((c_second ? p.src1 : p.src0) + c_ci);
    const char* baseB = reinterpret_cast<const char*>(wbase + (c_second ? p.C0 : 0) + c_ci);
#pragma unroll
    for (int i = 0; i < AR; ++i) ra[i] = *reinterpret_cast<const f32x4*>(baseA + voffA[i]);
#pragma unroll
    for (int j = 0; j < BRL; ++j) rb[j] = *reinterpret_cast<const f32x4*>(baseB + voffB[j]);
  };
  auto next_chunk = [&]() {
    ++c_k;
    c_ci += BK;
    if (c_ci == (c_second ? p.C1 : p.C0) && !c_second && p.src1 != nullptr) {
      c_second = 1;
      c_ci = 0;
      set_source(1);
    }
  };
  auto store_split = [&](float* rowp, f32x4 v) {
    const bf16x4 hi = __builtin_convertvector(v, bf16x4);
    const f32x4 hf = __builtin_convertvector(hi, f32x4);
    const bf16x4 lo = __builtin_convertvector(v - hf, bf16x4);
    char* base = reinterpret_cast<char*>(rowp) + seg * 8;
    *reinterpret_cast<bf16x4*>(base) = hi;
    *reinterpret_cast<bf16x4*>(base + 64) = lo;
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int l = srow + RPP * i;
      if (l < PMAX) {
        const f32x4 v = pixA[i] >= 0 ? ra[i] : zero4;
        if constexpr (PRE)
          *reinterpret_cast<f32x4*>(&As[l * LDK + seg * 4]) = v;
        else
          store_split(&As[l * LDK], v);
      }
    }
#pragma unroll
    for (int j = 0; j < BRL; ++j) {
      if constexpr (PRE)
        *reinterpret_cast<f32x4*>(&Bs[(srow + RPP * j) * LDK + seg * 4]) = rb[j];
      else
        store_split(&Bs[(srow + RPP * j) * LDK], rb[j]);
    }
  };
  auto mfma_bf16 = [&](const f32x4& a, const f32x4& b, AccT& c) {
    if constexpr (FR == 32)
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  };
  auto compute_chunk = [&]() {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int st = 0; st < NSTEP; ++st) {
        f32x4 ah[FM], al[FM], bh[FN], bl[FN];
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
          const float* rp = &As[(fragrow[mi] + tapoff[t]) * LDK + fk];
          ah[mi] = *reinterpret_cast<const f32x4*>(rp + st * GK);
          al[mi] = *reinterpret_cast<const f32x4*>(rp + (st + NSTEP) * GK);
        }
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          const float* rp = &Bs[(t * BN + ni * FR + frow) * LDK + fk];
          bh[ni] = *reinterpret_cast<const f32x4*>(rp + st * GK);
          bl[ni] = *reinterpret_cast<const f32x4*>(rp + (st + NSTEP) * GK);
        }
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
          for (int ni = 0; ni < FN; ++ni) {
            mfma_bf16(al[mi], bh[ni], acc[mi][ni]);
            mfma_bf16(ah[mi], bl[ni], acc[mi][ni]);
            mfma_bf16(ah[mi], bh[ni], acc[mi][ni]);
          }
      }
    }
  };

  const int nch = p.Ctot / BK;
  set_source(0);
  load_chunk();
  store_chunk();
  __syncthreads();
  for (int c = 0; c + 1 < nch; ++c) {
    next_chunk();
    load_chunk();
    compute_chunk();
    __syncthreads();   // everyone is done reading the stage
    store_chunk();
    __syncthreads();
  }
  compute_chunk();
  __syncthreads();     // the staged image becomes the epilogue's scratch

  fused_epilogue<BM, BN, WM, WN, FR, AccT, PMAX * LDK * 4>(p, acc, As, Bs, ri_out, ri_bc, 0, tid);
}

// narrow transposed convs in bf16x3 math: the four taps of a phase share one staged input image (convT_tap_kernel)
int launch_convT_tap(IGemmP& p, hipStream_t st) {
  if (!(p.convT && p.math == 1 && p.fast_ok && p.N <= 64 && p.Wq >= 32 && 128 % p.Wq == 0 && p.Hq % (128 / p.Wq) == 0 && g_force_splitk <= 0 &&
        p.M >= 128L * 256))
    return NOT_THIS_ENGINE;
  // 256-output tiles when the image geometry and the block count allow (bytes per output: see the kernel): eight-wave blocks (one
  // per CU) for N = 64 (pair_ab, headline pair: 3.392 -> 3.364 ms), four-wave blocks for N <= 32 (512-output tiles measured no
  // gain there: 3.388 / 3.388); 128-output tiles otherwise
  const bool big = p.Hq % (256 / p.Wq) == 0 && p.M >= 256L * 512;
  const int bm = big ? 256 : 128, waves = (big && p.N > 32) ? 8 : 4;
  p.MT = (int)(((long)p.M + bm - 1) / bm);
  p.NT = 1;
  p.S = 1;
  const long nblk = ((long)p.MT + 7) / 8 * 8 * 4;
  // measured (layer_bench, B=256, 512x256, 128-output tiles): N=16 368 -> 308 us, N=64 277 -> 249 us; N=32 no change, so the
  // 32-wide stage uses this kernel only with split32 operands (runner)
  const int w = p.N <= 16 ? 16 : (p.N <= 32 ? 32 : 64);
  if (nblk > 0x7fffffffL || (w == 32 && !p.presplit)) return NOT_THIS_ENGINE;
  const dim3 grid((unsigned)nblk), blk(64 * waves);
#define M2H_TAP_P(BN_, FR_, PRE_, WM256_)   /* WM256_: waves of the 256-output tile's block */                  \
  do {                                                                                                         \
    if (big) M2H_LAUNCH((convT_tap_kernel<BN_, FR_, PRE_, 256, WM256_>), grid, blk, 0, st, p);                 \
    else M2H_LAUNCH((convT_tap_kernel<BN_, FR_, PRE_, 128>), grid, blk, 0, st, p);                             \
  } while (0)
#define M2H_TAP(BN_, FR_, WM256_)                       \
  do {                                                  \
    if (p.presplit) M2H_TAP_P(BN_, FR_, 1, WM256_);     \
    else M2H_TAP_P(BN_, FR_, 0, WM256_);                \
  } while (0)
  if (w == 16) M2H_TAP(16, 16, 4);
  else if (w == 32) M2H_TAP(32, 32, 4);
  else M2H_TAP(64, 32, 8);
#undef M2H_TAP
#undef M2H_TAP_P
  return launch_status(w == 16 ? "igemm_convT_tap<16>" : (w == 32 ? "igemm_convT_tap<32>" : "igemm_convT_tap<64>"));
}

}  // namespace m2h
