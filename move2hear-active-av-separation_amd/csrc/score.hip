// Scorer (m2h/audio/score.py holds the definition): the sums and the Gram matrix of the N = S + 3 signals of one (recording, channel,
// tile) in ONE pass over the samples, in fp64 -- everything scale_bss_eval (common/eval_metrics.py:12-122) computes for a window
// follows from them, for any number of reference sources.
//
//   signals a_0 .. a_{N-1}: the S references' channel c, the estimate's channel c, the mixture's left and right channel
//   out[r][c][j][0 .. N)             = sum_t a_i[t]                         t over tile j: [j * tile, min((j + 1) * tile, L))
//   out[r][c][j][N .. N + N(N+1)/2)  = sum_t a_i[t] * a_k[t]                i <= k, row-major
//
// One 256-thread workgroup per (tile, c, r); every signal is read once.  A thread takes the groups of four consecutive samples
// 4g .. 4g + 3, g = thread, thread + 256, ..., and keeps the N + N(N+1)/2 <= 54 accumulators as doubles in registers (the kernel is a
// template on N: every index is a constant, nothing goes to scratch).  The floats are converted to double before the multiply, so each
// product is exact (48 bits) and only the additions round: a thread's chain of ceil(tile / 256) additions, then the block's tree.
// The tree has a fixed order: the xor butterfly of a wave, then the four waves in order -- no atomics, so the result is the same on
// every run.  A signal's group is one 16-byte load where that signal's row base + tile offset is 16-byte aligned and the group is whole,
// four 4-byte loads otherwise; a thread's samples and their order are the same on both paths, so the result does not depend on the
// alignment.  Samples past the tile's end enter as zeros, which change no accumulator.
//
// m2h_score_gram_lag (the Scorer's alignment) is the same kernel on the region [D, L - D) of every row, with the estimate of (r, c) read
// lag[r C + c] samples later; the lag comes from device memory and is clamped to [-D, D].  m2h_score_gram passes no lag and D = 0: the
// addresses, the samples of a thread and their order are what they were.
//
// m2h_score_windows adds the tiles of every window in tile order: a window's Gram is never a difference of prefix sums, so a
// window's score does not depend on what precedes it.
#include "score_common.h"

#include <cstdint>

namespace m2h {

constexpr int SCORE_THREADS = 256;

template <int N>
__global__ __launch_bounds__(SCORE_THREADS) void score_gram_kernel(ScoreSignals a, double* __restrict__ out, int C, long long L, int tile,
                                                                   long long J, const int* __restrict__ lag, int D) {
  constexpr int S = N - 3, K = N + N * (N + 1) / 2;
  __shared__ double sh[SCORE_THREADS / 64][K];
  const long long b = blockIdx.x;                      // = (r * C + c) * J + j
  const long long j = b % J, rc = b / J;
  const long long c = rc % C, r = rc / C;
  // m2h_score_gram_lag: the scored region starts at sample D of every row and the estimate is read lag[r C + c] samples later, clamped
  // to [-D, D].  m2h_score_gram: lag is null, D is 0.
  const long long shift = score_lag(lag, rc, D);
  const long long t0 = j * (long long)tile + D;
  const long long left = L - j * (long long)tile;
  const int n = left < tile ? (int)left : tile;        // samples of this tile, >= 1

  const float* p[N];
#pragma unroll
  for (int i = 0; i < S; ++i) p[i] = row(a.refs, r, i, c) + t0;
  p[S] = row(a.est, r, c) + t0 + shift;
  p[S + 1] = row(a.mix, r, 0) + t0;
  p[S + 2] = row(a.mix, r, 1) + t0;
  bool aligned[N];
#pragma unroll
  for (int i = 0; i < N; ++i) aligned[i] = (reinterpret_cast<uintptr_t>(p[i]) & 15) == 0;

  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;

  for (int g = threadIdx.x * 4; g < n; g += SCORE_THREADS * 4) {
    const bool whole = g + 4 <= n;
    float v[N][4];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (whole && aligned[i]) {
        const float4 q = *reinterpret_cast<const float4*>(p[i] + g);
        v[i][0] = q.x, v[i][1] = q.y, v[i][2] = q.z, v[i][3] = q.w;
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[i][t] = g + t < n ? p[i][g + t] : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double d[N];
#pragma unroll
      for (int i = 0; i < N; ++i) d[i] = (double)v[i][t];
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] += d[i];
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int m = i; m < N; ++m) acc[N + i * N - i * (i - 1) / 2 + m - i] += d[i] * d[m];      // exact product: fused or not, one rounding
    }
  }

#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double s = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < SCORE_THREADS / 64; ++w) s += sh[w][threadIdx.x];
    out[b * K + threadIdx.x] = s;
  }
}

// out[rc][m][k] = sum of tiles[rc][j][k] over j = m * hop .. min(m * hop + window, J) - 1, in that order (0 for a window without tiles)
__global__ __launch_bounds__(256) void score_windows_kernel(const double* __restrict__ tiles, double* __restrict__ out, long long RC, long long J,
                                                            int K, long long M, long long window, long long hop) {
  const long long total = RC * M * K;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const long long m = (i / K) % M, rc = i / ((long long)K * M);
    const long long j0 = m * hop;
    const long long j1 = window < J - j0 ? j0 + window : J;
    double s = 0.0;
    if (j0 < J) {
      const double* q = tiles + (rc * J + j0) * K + k;
      s = q[0];
      for (long long j = j0 + 1; j < j1; ++j) s += q[(j - j0) * K];
    }
    out[i] = s;
  }
}

// The checks and the launch behind both entry points: the L - 2 D samples from sample D on are scored; D is at least min_D.
static int score_gram_launch(const char* what, const ScoreSignals& a, double* out, int R, int S, int C, long long L, int tile, const int* lag, int D,
                             int min_D, m2h_stream stream) {
  static decltype(&score_gram_kernel<4>) const kernels[] = {score_gram_kernel<4>, score_gram_kernel<5>, score_gram_kernel<6>,
                                                            score_gram_kernel<7>, score_gram_kernel<8>, score_gram_kernel<9>};      // N = S + 3
  long long J;
  if (int rc = check_signals(what, a, true, out, R, S, C, L, D, min_D, 1)) return rc;
  if (int rc = check_lag(what, lag, D)) return rc;
  L -= 2ll * D;
  if (int rc = check_tiles(what, L, tile, (long long)R * C, J)) return rc;
  M2H_LAUNCH(kernels[S - 1], dim3((unsigned)(J * R * C)), dim3(SCORE_THREADS), 0, as_stream(stream), a, out, C, L, tile, J, lag, D);
  return launch_status(what);
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_score_gram(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr, long long est_sc,
                   const float* mix, long long mix_sr, long long mix_sc, double* out, int R, int S, int C, long long L, int tile, m2h_stream stream) {
  return score_gram_launch("score_gram", {{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}}, out, R, S, C, L, tile, nullptr, 0, 0, stream);
}

int m2h_score_gram_lag(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr, long long est_sc,
                       const float* mix, long long mix_sr, long long mix_sc, double* out, int R, int S, int C, long long L, int tile, const int* lag, int D,
                       m2h_stream stream) {
  return score_gram_launch("score_gram_lag", {{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}}, out, R, S, C, L, tile, lag, D, 1, stream);
}

int m2h_score_windows(const double* tiles, double* out, long long RC, long long J, int K, long long M, long long window, long long hop,
                      m2h_stream stream) {
  M2H_REQUIRE(tiles && out, "score_windows: null pointer (tiles %p, out %p)", (const void*)tiles, (void*)out);
  M2H_REQUIRE(RC >= 1 && J >= 1 && K >= 1 && M >= 1, "score_windows: RC = %lld, J = %lld, K = %d, M = %lld must all be positive", RC, J, K, M);
  M2H_REQUIRE(window >= 1 && hop >= 1, "score_windows: window = %lld and hop = %lld tiles must be positive", window, hop);
  M2H_REQUIRE(M <= 0x7fffffffffffffffLL / K / RC, "score_windows: RC * M * K = %lld * %lld * %d overflows", RC, M, K);
  const long long total = RC * M * K;
  const long long g = (total + 255) / 256;
  M2H_LAUNCH(score_windows_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, as_stream(stream), tiles, out, RC, J, K, M, window, hop);
  return launch_status("score_windows");
}

}  // extern "C"
