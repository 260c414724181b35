// Scorer, BSS-eval SDR / SIR / SAR with a distortion filter of T <= 512 taps (m2h/audio/score.py holds the definition, "BSS").  Two kernels,
// both fp64 on the vector unit: every fp32 sample is converted to double before it is multiplied, so a product is exact, and every sum has
// an order fixed by the recording alone -- no atomics, nothing depends on the batch, the strides or a row's alignment.
//
// m2h_bss_corr: the one-sided lagged correlations of every tile,
//
//   out[r][c][j][i][k][d] = sum_{t in tile j} s_i[t] * v_k[t + d]     d = 0 .. T - 1,  i < S,  v_0 .. v_{S-1} = the references, v_S = the
//                                                                     estimate at its lag, v_{S+1} = the baseline
//
// on the region [D, L - D) of every row, every signal zero past the region's end.  One 256-thread workgroup per (tile, c, r) and pair
// (i, k) walks its tile in chunks of 1024 samples: s_i's chunk and v_k's chunk + 512 go to LDS as floats; lane l of every wave owns the
// eight lags 8 l .. 8 l + 7, and wave w takes the steps w, w + 4, ... of eight samples: 16 floats of v_k and 8 of s_i feed 64 FMAs.  A
// lane's chain runs over its steps in order; the four waves are added in order.
//
// m2h_bss_project: the filters applied and the ten energies of every tile, no component signal ever stored,
//
//   s_t[n] = sum_a g[a] s_j[n - a]      P[n] = sum_i sum_a h_i[a] s_i[n - a]      (i ascending, then a ascending; once per right-hand side)
//   out[r][c][j][0 .. 5)  = sum_n s_t^2, (x - s_t)^2, (P - s_t)^2, P^2, (x - P)^2      [5 .. 10): the same for the baseline and its filters
//
// over the tile's n; the last tile also owns the tail [Lr, Lr + T - 1), where x is zero.  One workgroup per (tile, c, r) walks chunks of
// 1024 outputs: the S references' chunk + 512 history go to LDS as floats, the 2 (S + 1) filters as doubles, zero-extended to a multiple
// of four taps; a thread owns four consecutive outputs and takes four taps a step: two 16-byte LDS reads of samples and the broadcast
// coefficients feed 32 FMAs per reference (64 for the target).  A thread's ten sums run over its outputs in order, then the xor butterfly
// of a wave, then the four waves in order.
//
// Why the vector unit and not v_mfma_f64_16x16x4_f64: on this chip the published peak of the fp64 matrix path equals the vector path's,
// so the matrix form buys no rate; it would cost a Hankel view of the samples built per lane (one f64 A and B element per lane per four
// taps, the converted samples re-read from LDS for every 16 x 16 block), where the sliding window here converts a sample once for eight
// lags (or four outputs).  Both kernels compile without scratch (DESIGN.md 8.11 has the resource report).
#include "score_common.h"

namespace m2h {

constexpr int BSS_MAXT = 512;                       // the longest filter
constexpr int BSS_THREADS = 256;
constexpr int BSS_WAVES = BSS_THREADS / 64;
constexpr int BSS_CHUNK = 1024;                     // samples (corr) or outputs (project) staged at a time
constexpr int BSS_WINDOW = BSS_CHUNK + BSS_MAXT;    // a chunk plus the 512 samples after it (corr) or before it (project)

namespace {
__device__ __forceinline__ void to_double(const float4 q, double* d) { d[0] = (double)q.x, d[1] = (double)q.y, d[2] = (double)q.z, d[3] = (double)q.w; }
}  // namespace

__global__ __launch_bounds__(BSS_THREADS) void bss_corr_kernel(ScoreSignals a, double* __restrict__ out, int S, int C, long long Lr, int tile,
                                                               long long J, int T, const int* __restrict__ lag, int D) {
  __shared__ __attribute__((aligned(16))) float sa[BSS_CHUNK];
  __shared__ __attribute__((aligned(16))) float sv[BSS_WINDOW];
  __shared__ double red[BSS_WAVES][BSS_MAXT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                      // = (r * C + c) * J + j
  const long long j = b % J, rc = b / J;
  const long long c = rc % C, r = rc / C;
  const int i = (int)blockIdx.y / (S + 2), k = (int)blockIdx.y % (S + 2);
  const float* pa = row(a.refs, r, i, c) + D;
  const float* pv;
  long long other = 0;                                 // C = 1: the baseline is the mean of the mixture's two channels
  bool mono = false;
  if (k < S) {
    pv = row(a.refs, r, k, c) + D;
  } else if (k == S) {
    pv = row(a.est, r, c) + D + score_lag(lag, rc, D);   // clamped to [-D, D]
  } else {
    pv = row(a.mix, r, C == 2 ? c : 0) + D;
    mono = C == 1, other = a.mix.sc;
  }
  const long long g0 = j * (long long)tile;
  const long long left = Lr - g0;
  const int n = left < tile ? (int)left : tile;        // samples of this tile, >= 1

  double acc[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) acc[l] = 0.0;

  for (int off = 0; off < n; off += BSS_CHUNK) {
    if (off) __syncthreads();                          // every wave is done with the chunk before
    for (int u = tid; u < BSS_CHUNK; u += BSS_THREADS) sa[u] = off + u < n ? pa[g0 + off + u] : 0.f;
    for (int u = tid; u < BSS_WINDOW; u += BSS_THREADS) {
      const long long g = g0 + off + u;
      float v = 0.f;                                   // zero past the region: no sample outside it is read
      if (g < Lr) {
        v = pv[g];
        if (mono) v = 0.5f * (v + pv[g + other]);
      }
      sv[u] = v;
    }
    __syncthreads();
    const int m = n - off < BSS_CHUNK ? n - off : BSS_CHUNK;
    const int steps = (m + 7) >> 3;                    // samples past the tile's end are zeros in sa: they change no accumulator
    for (int s = wave; s < steps; s += BSS_WAVES) {
      const int t = s << 3;
      double x[8], w[16];
      to_double(*reinterpret_cast<const float4*>(sa + t), x);
      to_double(*reinterpret_cast<const float4*>(sa + t + 4), x + 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) to_double(*reinterpret_cast<const float4*>(sv + t + 8 * lane + 4 * q), w + 4 * q);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[l] = fma(x[u], w[u + l], acc[l]);      // exact product, one rounding
    }
  }

#pragma unroll
  for (int l = 0; l < 8; ++l) red[wave][8 * lane + l] = acc[l];
  __syncthreads();
  double* o = out + (b * gridDim.y + blockIdx.y) * T;
  for (int d = tid; d < T; d += BSS_THREADS) o[d] = ((red[0][d] + red[1][d]) + red[2][d]) + red[3][d];
}

__global__ __launch_bounds__(BSS_THREADS) void bss_project_kernel(ScoreSignals a, const long long* __restrict__ target, int target0,
                                                                  const double* __restrict__ h, double* __restrict__ out, int S, int C,
                                                                  long long Lr, int tile, long long J, int T, const int* __restrict__ lag, int D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bss_lds[];
  __shared__ double red[BSS_WAVES][10];
  const int Tp = (T + 3) & ~3;
  double* hd = reinterpret_cast<double*>(bss_lds);                          // [2][S + 1][Tp]
  float* sr = reinterpret_cast<float*>(hd + 2 * (S + 1) * Tp);             // [S][BSS_WINDOW]: index u is the region's sample n0 - 512 + u
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                      // = (r * C + c) * J + j
  const long long j = b % J, rc = b / J;
  const long long c = rc % C, r = rc / C;
  const int tg = (int)score_target(target, target0, r, S);                  // clamped to [0, S)
  const float* px = row(a.est, r, c) + D + score_lag(lag, rc, D);
  const float* pm = row(a.mix, r, C == 2 ? c : 0) + D;
  const long long other = C == 2 ? 0 : a.mix.sc;
  const long long begin = j * (long long)tile;
  const long long end = j == J - 1 ? Lr + T - 1 : begin + tile;             // the last tile also owns the tail

  const double* hrc = h + rc * 2 * (S + 1) * T;
  for (int u = tid; u < 2 * (S + 1) * Tp; u += BSS_THREADS) {
    const int f = u / Tp, t = u % Tp;
    hd[u] = t < T ? hrc[f * T + t] : 0.0;
  }

  double sum[10];
#pragma unroll
  for (int q = 0; q < 10; ++q) sum[q] = 0.0;

  for (long long n0 = begin; n0 < end; n0 += BSS_CHUNK) {
    __syncthreads();                                   // the filters are staged; every wave is done with the chunk before
    for (int i = 0; i < S; ++i) {
      const float* p = row(a.refs, r, i, c) + D;
      for (int u = tid; u < BSS_WINDOW; u += BSS_THREADS) {
        const long long g = n0 - BSS_MAXT + u;
        sr[i * BSS_WINDOW + u] = g >= 0 && g < Lr ? p[g] : 0.f;
      }
    }
    __syncthreads();

    double P[2][4], St[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) P[q][e] = 0.0, St[q][e] = 0.0;
    for (int i = 0; i < S; ++i) {
      const float* s = sr + i * BSS_WINDOW + BSS_MAXT + 4 * tid - 4;        // w[4 + e - a'] is the sample of output e at tap a0 + a'
      const double* h0 = hd + i * Tp;
      const double* h1 = hd + (S + 1 + i) * Tp;
      const bool is_target = i == tg;
      for (int a0 = 0; a0 < Tp; a0 += 4) {
        double w[8], c0[4], c1[4];
        to_double(*reinterpret_cast<const float4*>(s - a0), w);
        to_double(*reinterpret_cast<const float4*>(s - a0 + 4), w + 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) c0[t] = h0[a0 + t], c1[t] = h1[a0 + t];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) P[0][e] = fma(c0[t], w[4 + e - t], P[0][e]), P[1][e] = fma(c1[t], w[4 + e - t], P[1][e]);
        if (is_target) {                               // the target alone: slot S of either right-hand side
#pragma unroll
          for (int t = 0; t < 4; ++t) c0[t] = hd[S * Tp + a0 + t], c1[t] = hd[(2 * S + 1) * Tp + a0 + t];
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) St[0][e] = fma(c0[t], w[4 + e - t], St[0][e]), St[1][e] = fma(c1[t], w[4 + e - t], St[1][e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long n = n0 + 4 * tid + e;
      if (n < end) {
        double y[2] = {0.0, 0.0};                      // the estimate and the baseline, zero in the tail
        if (n < Lr) {
          const float m0 = pm[n], m1 = pm[n + other];
          y[0] = (double)px[n];
          y[1] = (double)(C == 2 ? m0 : 0.5f * (m0 + m1));
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const double st = St[q][e], p = P[q][e], d0 = y[q] - st, d1 = p - st, d2 = y[q] - p;
          sum[5 * q + 0] = fma(st, st, sum[5 * q + 0]);
          sum[5 * q + 1] = fma(d0, d0, sum[5 * q + 1]);
          sum[5 * q + 2] = fma(d1, d1, sum[5 * q + 2]);
          sum[5 * q + 3] = fma(p, p, sum[5 * q + 3]);
          sum[5 * q + 4] = fma(d2, d2, sum[5 * q + 4]);
        }
      }
    }
  }

#pragma unroll
  for (int q = 0; q < 10; ++q) {
    const double s = wave_sum(sum[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (tid < 10) out[b * 10 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

namespace {
// What both entry points check: the signals, the lag rule, T, the alignment of the fp64 buffers, the tiles of the region.
int check_bss(const char* what, const ScoreSignals& a, const void* out, int R, int S, int C, long long L, int tile, int T, const int* lag, int D,
              long long& Lr, long long& J) {
  if (int rc = check_signals(what, a, true, out, R, S, C, L, D, 0, 1)) return rc;
  if (int rc = check_lag(what, lag, D)) return rc;
  M2H_REQUIRE(T >= 1 && T <= BSS_MAXT, "%s: T = %d taps; 1 .. %d are supported", what, T, BSS_MAXT);
  M2H_REQUIRE((reinterpret_cast<size_t>(out) & 7) == 0, "%s: out must be 8-byte aligned", what);
  Lr = L - 2ll * D;
  return check_tiles(what, Lr, tile, (long long)R * C, J);
}
}  // namespace

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_bss_corr(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr, long long est_sc,
                 const float* mix, long long mix_sr, long long mix_sc, double* out, int R, int S, int C, long long L, int tile, int T, const int* lag,
                 int D, m2h_stream stream) {
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}};
  long long Lr, J;
  if (int rc = check_bss("bss_corr", a, out, R, S, C, L, tile, T, lag, D, Lr, J)) return rc;
  M2H_LAUNCH(bss_corr_kernel, dim3((unsigned)(J * R * C), S * (S + 2)), dim3(BSS_THREADS), 0, as_stream(stream), a, out, S, C, Lr, tile, J, T, lag, D);
  return launch_status("bss_corr");
}

int m2h_bss_project(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr, long long est_sc,
                    const float* mix, long long mix_sr, long long mix_sc, const long long* target, int target0, const double* h, double* out, int R,
                    int S, int C, long long L, int tile, int T, const int* lag, int D, m2h_stream stream) {
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}};
  long long Lr, J;
  if (int rc = check_bss("bss_project", a, out, R, S, C, L, tile, T, lag, D, Lr, J)) return rc;
  M2H_REQUIRE(h, "bss_project: null pointer (h)");
  M2H_REQUIRE((reinterpret_cast<size_t>(h) & 7) == 0, "bss_project: h must be 8-byte aligned");
  if (int rc = check_target("bss_project", target, target0, S)) return rc;
  const size_t lds = sizeof(double) * 2 * (S + 1) * ((T + 3) & ~3) + sizeof(float) * S * BSS_WINDOW;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bss_project_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail((int)e, "bss_project: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
  M2H_LAUNCH(bss_project_kernel, dim3((unsigned)(J * R * C)), dim3(BSS_THREADS), lds, as_stream(stream), a, target, target0, h, out, S, C, Lr, tile, J,
             T, lag, D);
  return launch_status("bss_project");
}

}  // extern "C"
