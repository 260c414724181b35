// Scorer, interaural cues (m2h/audio/score.py holds the definition, "Spatial"): for every (recording, one-second tile, signal x of G
// (target), E (estimate), B (baseline: the mixture)) and each of the 32 bands of 16 bins, the four sums over the band's 16 bins x 32 frames
// of the two ears' spectrograms X_L, X_R
//
//   0 PL = sum |X_L|^2   1 PR = sum |X_R|^2   2 CRE = sum Re(X_L conj X_R)   3 CIM = sum Im(X_L conj X_R)
//
// straight from the waveforms.  The spectrogram, its folded transform and the staging are score_stft.h's (read there why), with two
// signals, the TWO EARS of x: one 512-thread workgroup per (signal, tile, recording), 69 KB of LDS (one workgroup per CU all the same: two
// would need 128 registers or fewer, and capped there the compiler spills -- DESIGN.md 8.9), and a wave issues 4 LDS reads and 16 MFMAs
// per k-step.  A wave's bins 64 w .. 64 w + 63 are the bands 4 w .. 4 w + 3 whole, one per column tile, and a lane holds Re and Im of both
// ears at the same (frame, bin), so the products need no exchange.
//
// The four fp32 values of an element are converted to double first and multiplied and added in double (the product of two fp32 values is
// exact in fp64, so contraction into an fma changes no bit); a lane's 2 x 16 elements are added in a fixed order, and a band's sum is then
// the xor butterfly of its wave over 64 lanes and nothing else: no cross-wave reduction, no LDS, no atomics.  The same bits on every run.
#include "score_stft.h"

namespace m2h {

namespace {

constexpr int SX_BANDS = 32, SX_SUMS = 4, SX_SIGNALS = 3;   // out [R][J][3][32][4]

}  // namespace

__global__ __launch_bounds__(STFT_THREADS) void score_spatial_kernel(ScoreSignals a, const long long* __restrict__ target, int target0, int S,
                                                                     const float* __restrict__ dft, double* __restrict__ out, long long L, long long J,
                                                                     const int* __restrict__ lag, int D) {
  extern __shared__ __attribute__((aligned(16))) float smem[];          // [2][STFT_ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                                        // = (r * J + j) * 3 + x
  const int x = (int)(b % SX_SIGNALS);
  const long long rj = b / SX_SIGNALS;
  const long long j = rj % J, r = rj / J;
  const long long t = score_target(target, target0, r, S), shift = score_lag(lag, 2 * r, D);    // clamped to [0, S) and to [-D, D]; ONE lag, the left ear's, for both ears
  const long long t0 = j * (long long)STFT_TILE + D;
  const long long left = L - j * (long long)STFT_TILE;
  const int n = left < STFT_TILE ? (int)left : STFT_TILE;                // samples of this tile, >= 1; the rest of the second is zeros
  const float* pl = x == 0 ? row(a.refs, r, t, 0) + t0 : x == 1 ? row(a.est, r, 0) + t0 + shift : row(a.mix, r, 0) + t0;
  const float* pr = pl + (x == 0 ? a.refs.sc : x == 1 ? a.est.sc : a.mix.sc);

  double sum[4][SX_SUMS];
#pragma unroll
  for (int y = 0; y < 4; ++y)
#pragma unroll
    for (int k = 0; k < SX_SUMS; ++k) sum[y][k] = 0.0;

#pragma unroll 1
  for (int h = 0; h < 2; ++h) {                                          // (not unrolled: one half's accumulators live at a time)
    if (h) __syncthreads();                                              // every wave is done with the first half's samples
    stft_stage<2>(smem, h, n, tid, [&](int i, float (&v)[2]) { v[0] = pl[i], v[1] = pr[i]; });
    __syncthreads();

    f32x4 re[2][4], im[2][4];
    stft_half<2>(smem, dft, lane, wave, re, im);

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
      const double s = wave_sum(sum[y][k]);
      if (lane == 0) o[y * SX_SUMS + k] = s;
    }
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_score_spatial(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr,
                                 long long est_sc, const float* mix, long long mix_sr, long long mix_sc, const long long* target, int target0,
                                 const float* dft, double* out, int R, int S, long long L, const int* lag, int D, m2h_stream stream) {
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}};
  long long Ls, J;
  size_t lds;
  if (int rc = check_stft("score_spatial", a, target, target0, dft, out, R, S, 2, L, lag, D, (long long)R * SX_SIGNALS, Ls, J)) return rc;
  if (int rc = reserve_stft_lds<2>(score_spatial_kernel, "score_spatial", lds)) return rc;
  M2H_LAUNCH(score_spatial_kernel, dim3((unsigned)(J * R * SX_SIGNALS)), dim3(STFT_THREADS), lds, as_stream(stream), a, target, target0, S, dft, out, Ls,
             J, lag, D);
  return launch_status("score_spatial");
}
