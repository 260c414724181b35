// Scorer, broadband ITD (m2h/audio/score.py holds the definition, "ITD"): two launches.
//
// m2h_score_itd: for every (recording, one-second tile, signal x of G (target), E (estimate), B (baseline: the mixture)) and every bin
// k = 0 .. 255 the cross-spectrum of the two ears' spectrograms X_L, X_R summed over the tile's 32 frames,
//
//   0 CRE_k = sum_f Re(X_L conj X_R)   1 CIM_k = sum_f Im(X_L conj X_R)
//
// straight from the waveforms: score_spatial.hip's cross term per bin instead of per band.  The spectrogram, its folded transform and the
// staging are score_stft.h's with two signals, the TWO EARS of x, one 512-thread workgroup per (signal, tile, recording), 69 KB of LDS --
// but only the lower half of the bins is wanted, so the transform runs with two column tiles per wave, wave w owning the bins
// 32 w .. 32 w + 31: 4 LDS reads and 8 MFMAs per k-step and 32 accumulator registers where the spatial kernel has 16 and 64.
//
// In the C/D fragment a lane holds bin l & 15 at the frames 4 (l >> 4) + reg.  The four fp32 values of an element are converted to double
// first and multiplied and added in double (the product of two fp32 values is exact in fp64, so contraction into an fma changes no bit);
// a lane's 4 registers x 2 halves are added in a fixed order, the four lane groups by the xor-16 and xor-32 exchanges, and the lanes
// 0 .. 15 store the column tile's 16 bins x 2 doubles, 256 contiguous bytes.  No LDS, no atomics, no cross-wave step: the same bits on
// every run.
//
// m2h_itd_gcc: the PHAT-weighted cross-correlation of a row of (window) sums at the lags i / 8 samples, i = -128 .. 128.  One workgroup
// per row: the band's bins are normalised once into LDS in fp64 (a bin of magnitude 0 stays 0), then thread t owns lag i = t - 128 and
// adds the bins in ascending k; the twiddle of (k, i) is the table's entry (k i) mod 8184, reduced in integers.  The bits of a row depend
// on nothing but the row.
#include "score_stft.h"

namespace m2h {

namespace {

constexpr int ITD_BINS = 256, ITD_SIGNALS = 3, ITD_NY = 2;   // out [R][J][3][256][2]
constexpr int ITD_LAGS = 257, ITD_HALF = 128;                // the lags i / 8 samples, i = -128 .. 128
constexpr int ITD_PERIOD = 1023 * 8;                         // the twiddle table's entries: exp(j 2 pi t / 8184)
constexpr int ITD_GCC_THREADS = 320, ITD_GCC_AHEAD = 8;

}  // namespace

__global__ __launch_bounds__(STFT_THREADS) void score_itd_kernel(ScoreSignals a, const long long* __restrict__ target, int target0, int S,
                                                                 const float* __restrict__ dft, double* __restrict__ out, long long L, long long J,
                                                                 const int* __restrict__ lag, int D) {
  extern __shared__ __attribute__((aligned(16))) float smem[];          // [2][STFT_ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                                        // = (r * J + j) * 3 + x
  const int x = (int)(b % ITD_SIGNALS);
  const long long rj = b / ITD_SIGNALS;
  const long long j = rj % J, r = rj / J;
  const long long t = score_target(target, target0, r, S), shift = score_lag(lag, 2 * r, D);    // clamped to [0, S) and to [-D, D]; ONE lag, the left ear's, for both ears
  const long long t0 = j * (long long)STFT_TILE + D;
  const long long left = L - j * (long long)STFT_TILE;
  const int n = left < STFT_TILE ? (int)left : STFT_TILE;                // samples of this tile, >= 1; the rest of the second is zeros
  const float* pl = x == 0 ? row(a.refs, r, t, 0) + t0 : x == 1 ? row(a.est, r, 0) + t0 + shift : row(a.mix, r, 0) + t0;
  const float* pr = pl + (x == 0 ? a.refs.sc : x == 1 ? a.est.sc : a.mix.sc);

  double cre[ITD_NY], cim[ITD_NY];
#pragma unroll
  for (int y = 0; y < ITD_NY; ++y) cre[y] = cim[y] = 0.0;

#pragma unroll 1
  for (int h = 0; h < 2; ++h) {                                          // (not unrolled: one half's accumulators live at a time)
    if (h) __syncthreads();                                              // every wave is done with the first half's samples
    stft_stage<2>(smem, h, n, tid, [&](int i, float (&v)[2]) { v[0] = pl[i], v[1] = pr[i]; });
    __syncthreads();

    f32x4 re[2][ITD_NY], im[2][ITD_NY];
    stft_half<2, ITD_NY>(smem, dft, lane, wave, re, im);

#pragma unroll
    for (int y = 0; y < ITD_NY; ++y)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double lr = (double)re[0][y][i], li = (double)im[0][y][i], rr = (double)re[1][y][i], ri = (double)im[1][y][i];
        cre[y] += lr * rr + li * ri;
        cim[y] += li * rr - lr * ri;
      }
  }

  double* o = out + b * (long long)(ITD_BINS * 2) + (16 * ITD_NY * wave + (lane & 15)) * 2;     // this lane's bin of the wave's first column tile
#pragma unroll
  for (int y = 0; y < ITD_NY; ++y) {
    double c = cre[y], s = cim[y];
    c += __shfl_xor(c, 16, 64);                                          // the four lane groups: the frames 4 g .. 4 g + 3, g = l >> 4
    s += __shfl_xor(s, 16, 64);
    c += __shfl_xor(c, 32, 64);
    s += __shfl_xor(s, 32, 64);
    if (lane < 16) o[y * 32] = c, o[y * 32 + 1] = s;
  }
}

__global__ __launch_bounds__(ITD_GCC_THREADS) void itd_gcc_kernel(const double* __restrict__ sums, const double* __restrict__ table,
                                                                  double* __restrict__ gcc, int k_lo, int k_hi) {
  __shared__ double ph[ITD_BINS][2];
  const int tid = threadIdx.x;
  const long long rw = blockIdx.x;
  if (tid >= k_lo && tid < k_hi) {                                       // (tid < 256 here: k_hi <= 256, checked by the entry point)
    const double c = sums[(rw * ITD_BINS + tid) * 2], s = sums[(rw * ITD_BINS + tid) * 2 + 1];
    const double mag = sqrt(c * c + s * s);
    ph[tid][0] = mag > 0.0 ? c / mag : 0.0;
    ph[tid][1] = mag > 0.0 ? s / mag : 0.0;
  }
  __syncthreads();
  if (tid >= ITD_LAGS) return;
  const int i = tid - ITD_HALF;
  int t = ((k_lo * i) % ITD_PERIOD + ITD_PERIOD) % ITD_PERIOD;           // (k i) mod 8184, |k i| <= 255 * 128; then + i per bin
  const int step = (i + ITD_PERIOD) % ITD_PERIOD;
  double acc = 0.0;
  for (int k0 = k_lo; k0 < k_hi; k0 += ITD_GCC_AHEAD) {                  // the twiddles of ITD_GCC_AHEAD bins in flight at once (a lane's reads are
    double c[ITD_GCC_AHEAD], s[ITD_GCC_AHEAD];                           // 16 bytes each, k entries apart from its neighbour's); added in ascending k
#pragma unroll
    for (int u = 0; u < ITD_GCC_AHEAD; ++u) {
      c[u] = table[2 * t], s[u] = table[2 * t + 1];                      // (past k_hi - 1 the index still lies in the table; the value is not used)
      t += step;
      t = t >= ITD_PERIOD ? t - ITD_PERIOD : t;
    }
#pragma unroll
    for (int u = 0; u < ITD_GCC_AHEAD; ++u)
      if (k0 + u < k_hi) acc += ph[k0 + u][0] * c[u] + ph[k0 + u][1] * s[u];          // Re(phat_k exp(-j 2 pi k i / 8184))
  }
  gcc[rw * ITD_LAGS + tid] = acc / (double)(k_hi - k_lo);
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_score_itd(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr,
                             long long est_sc, const float* mix, long long mix_sr, long long mix_sc, const long long* target, int target0,
                             const float* dft, double* out, int R, int S, long long L, const int* lag, int D, m2h_stream stream) {
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}};
  long long Ls, J;
  size_t lds;
  if (int rc = check_stft("score_itd", a, target, target0, dft, out, R, S, 2, L, lag, D, (long long)R * ITD_SIGNALS, Ls, J)) return rc;
  if (int rc = reserve_stft_lds<2>(score_itd_kernel, "score_itd", lds)) return rc;
  M2H_LAUNCH(score_itd_kernel, dim3((unsigned)(J * R * ITD_SIGNALS)), dim3(STFT_THREADS), lds, as_stream(stream), a, target, target0, S, dft, out, Ls, J,
             lag, D);
  return launch_status("score_itd");
}

extern "C" int m2h_itd_gcc(const double* sums, const double* table, double* gcc, long long rows, int k_lo, int k_hi, m2h_stream stream) {
  M2H_REQUIRE(sums && table && gcc, "itd_gcc: null pointer (sums %p, table %p, gcc %p)", (const void*)sums, (const void*)table, (const void*)gcc);
  M2H_REQUIRE(k_lo >= 0 && k_lo < k_hi && k_hi <= ITD_BINS, "itd_gcc: bins k_lo = %d .. k_hi = %d; 0 <= k_lo < k_hi <= %d is required", k_lo, k_hi, ITD_BINS);
  M2H_REQUIRE(rows >= 1 && rows <= 0x7fffffffLL, "itd_gcc: rows = %lld; 1 .. 2^31 - 1 are supported", rows);
  M2H_REQUIRE(((reinterpret_cast<size_t>(sums) | reinterpret_cast<size_t>(table) | reinterpret_cast<size_t>(gcc)) & 7) == 0,
              "itd_gcc: sums, table and gcc must be 8-byte aligned");
  M2H_LAUNCH(itd_gcc_kernel, dim3((unsigned)rows), dim3(ITD_GCC_THREADS), 0, as_stream(stream), sums, table, gcc, k_lo, k_hi);
  return launch_status("itd_gcc");
}
