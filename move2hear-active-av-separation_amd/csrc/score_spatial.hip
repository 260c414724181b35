// Scorer, interaural cues (m2h/audio/score.py holds the definition, "Spatial"): for every (recording, one-second tile, signal x of G
// (target), E (estimate), B (baseline: the mixture)) and each of the 32 bands of 16 bins, the four sums over the band's 16 bins x 32 frames
// of the two ears' spectrograms X_L, X_R
//
//   0 PL = sum |X_L|^2   1 PR = sum |X_R|^2   2 CRE = sum Re(X_L conj X_R)   3 CIM = sum Im(X_L conj X_R)
//
// straight from the waveforms: no frame and no spectrum is ever written to memory.  The spectrogram, the folded transform on
// v_mfma_f32_16x16x4_f32, its table, the LDS bank skew and the staging by index arithmetic are score_spectral.hip's (read there why):
// the tile zero-extended to 16000 samples, reflect-padded by 511 inside the tile, 32 frames of 1023 samples every 512, periodic Hann,
// 1023-point DFT, bins 0 .. 511; nothing outside a row's [start, start + L) is read.
//
// One 512-thread workgroup per (signal, tile, recording) works through the tile's two halves of 16 frames one after the other.  A half's
// padded samples of the signal's TWO EARS are staged in LDS (2 x 8772 words, 69 KB; one workgroup per CU all the same: two would need
// 128 registers or fewer, and capped there the compiler spills -- DESIGN.md 8.9).  Wave w owns the bins 64 w .. 64 w + 63, which are the bands 4 w .. 4 w + 3 whole: four 16-bin column tiles = four bands, for
// each the cos and the sin fragment, applied to the two ears' M-tile of the same 16 frames -- 2 x 4 x (re, im) accumulators of 4
// registers, so a lane holds Re and Im of both ears at the same (frame, bin) and the products need no exchange.  Per k-step of 4 samples a
// wave issues 4 LDS reads, 8 coalesced 256-byte table reads (prefetched one step ahead) and 16 MFMAs.
//
// The four fp32 values of an element are converted to double first and multiplied and added in double (the product of two fp32 values is
// exact in fp64, so contraction into an fma changes no bit); a lane's 2 x 16 elements are added in a fixed order, and a band's sum is then
// the xor butterfly of its wave over 64 lanes and nothing else: no cross-wave reduction, no LDS, no atomics.  The same bits on every run,
// and for any batch, stride or alignment around a recording (only the staged values enter the arithmetic).
#include "score_common.h"

namespace m2h {

namespace {

constexpr int SX_THREADS = 512;
constexpr int SX_TILE = 16000, SX_PAD = 511, SX_HOP = 512, SX_KSTEPS = 128;
constexpr int SX_HALF = 16 * SX_HOP;                        // padded samples between the first frames of the two halves
constexpr int SX_SPAN = 15 * SX_HOP + 1024;                 // staged positions of a half: 8703 samples and one zero (the partner of n = 0 in the last frame)
constexpr int SX_ROW = SX_SPAN + 4 * (SX_SPAN >> 9);        // with the bank skew: 8772 words >= the largest address 8767 + 1
constexpr int SX_TABLE_BT = SX_KSTEPS * 2 * 64;             // table words per 16-bin column tile
constexpr int SX_BANDS = 32, SX_SUMS = 4, SX_SIGNALS = 3;   // out [R][J][3][32][4]

using f32x4 = __attribute__((ext_vector_type(4))) float;

}  // namespace

__global__ __launch_bounds__(SX_THREADS) void score_spatial_kernel(ScoreSignals a, const long long* __restrict__ target, int target0, int S,
                                                                   const float* __restrict__ dft, double* __restrict__ out, long long L, long long J,
                                                                   const int* __restrict__ lag, int D) {
  extern __shared__ __attribute__((aligned(16))) float smem[];          // [2][SX_ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                                        // = (r * J + j) * 3 + x
  const int x = (int)(b % SX_SIGNALS);
  const long long rj = b / SX_SIGNALS;
  const long long j = rj % J, r = rj / J;
  const long long t = score_target(target, target0, r, S), shift = score_lag(lag, 2 * r, D);    // clamped to [0, S) and to [-D, D]; ONE lag, the left ear's, for both ears
  const long long t0 = j * (long long)SX_TILE + D;
  const long long left = L - j * (long long)SX_TILE;
  const int n = left < SX_TILE ? (int)left : SX_TILE;                    // samples of this tile, >= 1; the rest of the second is zeros
  const float* pl = x == 0 ? row(a.refs, r, t, 0) + t0 : x == 1 ? row(a.est, r, 0) + t0 + shift : row(a.mix, r, 0) + t0;
  const float* pr = pl + (x == 0 ? a.refs.sc : x == 1 ? a.est.sc : a.mix.sc);

  float* sl = smem;
  float* sr = smem + SX_ROW;

  // A fragment: lane l holds A[frame l & 15][k = l >> 4]; B fragment: B[k = l >> 4][bin l & 15]; C/D: bin l & 15, frame 4 (l >> 4) + reg
  const int m = lane & 15, kq = lane >> 4;
  const int lo0 = SX_HOP * m + kq + 4 * m;                               // word of sample n = kq of frame m (then + 4 per k-step)
  const int hi0 = SX_HOP * m + 1023 - kq + 4 * (m + 1);                  // word of its partner 1023 - n (then - 4 per k-step)
  const float* tb = dft + (size_t)(4 * wave) * SX_TABLE_BT + lane;

  double sum[4][SX_SUMS];
#pragma unroll
  for (int y = 0; y < 4; ++y)
#pragma unroll
    for (int k = 0; k < SX_SUMS; ++k) sum[y][k] = 0.0;

#pragma unroll 1
  for (int h = 0; h < 2; ++h) {                                          // (not unrolled: one half's accumulators live at a time)
    if (h) __syncthreads();                                              // every wave is done with the first half's samples
    static_assert(SX_SPAN % SX_THREADS == 0, "a thread stages SX_SPAN / SX_THREADS positions of each ear");
    float vl[SX_SPAN / SX_THREADS], vr[SX_SPAN / SX_THREADS];
#pragma unroll
    for (int u = 0; u < SX_SPAN / SX_THREADS; ++u) {                     // every load of the half in flight at once: the index of a
      const int q = tid + u * SX_THREADS;                               // zero is clamped to sample 0, which every tile has
      int i = h * SX_HALF + q - SX_PAD;                                  // the tile's sample behind padded position h * 8192 + q
      i = i < 0 ? -i : i;
      i = i > SX_TILE - 1 ? 2 * (SX_TILE - 1) - i : i;
      const bool ok = q < SX_SPAN - 1 && i < n;
      i = ok ? i : 0;
      const float l0 = pl[i], r0 = pr[i];
      vl[u] = ok ? l0 : 0.f;
      vr[u] = ok ? r0 : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SX_SPAN / SX_THREADS; ++u) {
      const int q = tid + u * SX_THREADS;
      const int w = q + 4 * (q >> 9);
      sl[w] = vl[u];
      sr[w] = vr[u];
    }
    __syncthreads();

    f32x4 re[2][4], im[2][4];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int y = 0; y < 4; ++y) re[c][y] = im[c][y] = f32x4{0.f, 0.f, 0.f, 0.f};

    float bc[4], bs[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      bc[y] = tb[y * SX_TABLE_BT];
      bs[y] = tb[y * SX_TABLE_BT + 64];
    }
#pragma unroll 2
    for (int ks = 0; ks < SX_KSTEPS; ++ks) {
      const int kn = ks + 1 < SX_KSTEPS ? ks + 1 : ks;                   // the next step's table fragments, in flight under this step's MFMAs
      float nc[4], ns[4];
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        nc[y] = tb[y * SX_TABLE_BT + kn * 128];
        ns[y] = tb[y * SX_TABLE_BT + kn * 128 + 64];
      }
      const int lo = lo0 + 4 * ks, hi = hi0 - 4 * ks;
      const float l0 = sl[lo], l1 = sl[hi], r0 = sr[lo], r1 = sr[hi];
      const float as[2] = {l0 + l1, r0 + r1};
      const float ad[2] = {l0 - l1, r0 - r1};
#pragma unroll
      for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          re[c][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[c], bc[y], re[c][y], 0, 0, 0);
          im[c][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[c], bs[y], im[c][y], 0, 0, 0);
        }
#pragma unroll
      for (int y = 0; y < 4; ++y) bc[y] = nc[y], bs[y] = ns[y];
    }

#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double lr = (double)re[0][y][i], li = (double)im[0][y][i], rr = (double)re[1][y][i], ri = (double)im[1][y][i];
        sum[y][0] += lr * lr + li * li;
        sum[y][1] += rr * rr + ri * ri;
        sum[y][2] += lr * rr + li * ri;
        sum[y][3] += li * rr - lr * ri;
      }
  }

  double* o = out + b * (long long)(SX_BANDS * SX_SUMS) + (4 * wave) * SX_SUMS;      // this wave's four bands
#pragma unroll
  for (int y = 0; y < 4; ++y)
#pragma unroll
    for (int k = 0; k < SX_SUMS; ++k) {
      double s = sum[y][k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) o[y * SX_SUMS + k] = s;
    }
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_score_spatial(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr,
                                 long long est_sc, const float* mix, long long mix_sr, long long mix_sc, const long long* target, int target0,
                                 const float* dft, double* out, int R, int S, long long L, const int* lag, int D, m2h_stream stream) {
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}};
  long long J;
  if (int rc = check_signals("score_spatial", a, true, out, R, S, 2, L, D, 0, 1)) return rc;
  M2H_REQUIRE(dft, "score_spatial: null pointer (dft)");
  if (int rc = check_lag("score_spatial", lag, D)) return rc;
  if (int rc = check_target("score_spatial", target, target0, S)) return rc;
  M2H_REQUIRE((reinterpret_cast<size_t>(out) & 7) == 0, "score_spatial: out must be 8-byte aligned");
  const long long Ls = L - 2ll * D;
  if (int rc = check_tiles("score_spatial", Ls, SX_TILE, (long long)R * SX_SIGNALS, J)) return rc;
  const size_t lds = sizeof(float) * 2 * SX_ROW;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(score_spatial_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail((int)e, "score_spatial: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
  M2H_LAUNCH(score_spatial_kernel, dim3((unsigned)(J * R * SX_SIGNALS)), dim3(SX_THREADS), lds, as_stream(stream), a, target, target0, S, dft, out, Ls, J,
             lag, D);
  return launch_status("score_spatial");
}
