// Scorer, STFT distance (m2h/audio/score.py holds the definition, "Spectral"): for every (recording, channel, one-second tile) the seven
// sums over the 512 x 32 bins of the tile's spectrograms G (target), E (estimate), B (baseline)
//
//   0 sum |G|^2   1 sum |E|^2   2 sum |B|^2   3 sum (|E| - |G|)^2   4 sum |E - G|^2   5 sum (|B| - |G|)^2   6 sum |B - G|^2
//
// straight from the waveforms.  The spectrogram, its folded transform and the staging are score_stft.h's (read there why), with three
// signals: one 512-thread workgroup per (tile, c, r) stages target, estimate at its lag and the baseline, formed on the way in (103 KB of
// LDS), and a wave issues 6 LDS reads and 24 MFMAs per k-step.
//
// Magnitudes and differences are fp32; every square is converted to double before it is added: a lane's 2 x 16 elements in a fixed order,
// then score.hip's reduction -- the xor butterfly of a wave, then the eight waves in order.  No atomics: the same bits on every run.
#include "score_stft.h"

namespace m2h {

namespace {

constexpr int SP_WAVES = STFT_THREADS / 64;

__device__ __forceinline__ double sq(float v) { return (double)v * (double)v; }

}  // namespace

__global__ __launch_bounds__(STFT_THREADS) void score_spectral_kernel(ScoreSignals a, const long long* __restrict__ target, int target0, int S,
                                                                      const float* __restrict__ dft, double* __restrict__ out, int C, long long L,
                                                                      long long J, const int* __restrict__ lag, int D) {
  extern __shared__ __attribute__((aligned(16))) float smem[];          // [3][STFT_ROW]
  __shared__ double red[SP_WAVES][7];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                                        // = (r * C + c) * J + j
  const long long j = b % J, rc = b / J;
  const long long c = rc % C, r = rc / C;
  const long long t = score_target(target, target0, r, S), shift = score_lag(lag, rc, D);       // clamped to [0, S) and to [-D, D]
  const long long t0 = j * (long long)STFT_TILE + D;
  const long long left = L - j * (long long)STFT_TILE;
  const int n = left < STFT_TILE ? (int)left : STFT_TILE;                // samples of this tile, >= 1; the rest of the second is zeros
  const float* pg = row(a.refs, r, t, c) + t0;
  const float* pe = row(a.est, r, c) + t0 + shift;
  const float* pm = row(a.mix, r, 0) + (C == 2 ? c * a.mix.sc : 0) + t0;
  const long long mix_other = C == 2 ? 0 : a.mix.sc;                      // C = 1: the baseline is the mean of the two channels

  double sum[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) sum[k] = 0.0;

#pragma unroll 1
  for (int h = 0; h < 2; ++h) {                                          // (not unrolled: one half's accumulators live at a time)
    if (h) __syncthreads();                                              // every wave is done with the first half's samples
    stft_stage<3>(smem, h, n, tid, [&](int i, float (&x)[3]) {
      const float gv = pg[i], ev = pe[i], m0 = pm[i], m1 = pm[i + mix_other];
      x[0] = gv, x[1] = ev, x[2] = C == 2 ? m0 : 0.5f * (m0 + m1);
    });
    __syncthreads();

    f32x4 re[3][4], im[3][4];
    stft_half<3>(smem, dft, lane, wave, re, im);

#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float gr = re[0][y][i], gi = im[0][y][i], er = re[1][y][i], ei = im[1][y][i], br = re[2][y][i], bi = im[2][y][i];
        const float mg = sqrtf(gr * gr + gi * gi), me = sqrtf(er * er + ei * ei), mb = sqrtf(br * br + bi * bi);
        sum[0] += sq(gr) + sq(gi);
        sum[1] += sq(er) + sq(ei);
        sum[2] += sq(br) + sq(bi);
        sum[3] += sq(me - mg);
        sum[4] += sq(er - gr) + sq(ei - gi);
        sum[5] += sq(mb - mg);
        sum[6] += sq(br - gr) + sq(bi - gi);
      }
  }

#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double s = wave_sum(sum[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (tid < 7) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < SP_WAVES; ++w) s += red[w][tid];
    out[b * 7 + tid] = s;
  }
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_score_spectral(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr,
                                  long long est_sc, const float* mix, long long mix_sr, long long mix_sc, const long long* target, int target0,
                                  const float* dft, double* out, int R, int S, int C, long long L, const int* lag, int D, m2h_stream stream) {
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}};
  long long Ls, J;
  size_t lds;
  if (int rc = check_stft("score_spectral", a, target, target0, dft, out, R, S, C, L, lag, D, (long long)R * C, Ls, J)) return rc;
  if (int rc = reserve_stft_lds<3>(score_spectral_kernel, "score_spectral", lds)) return rc;
  M2H_LAUNCH(score_spectral_kernel, dim3((unsigned)(J * R * C)), dim3(STFT_THREADS), lds, as_stream(stream), a, target, target0, S, dft, out, C, Ls, J,
             lag, D);
  return launch_status("score_spectral");
}
