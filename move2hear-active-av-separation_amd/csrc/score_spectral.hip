// Scorer, STFT distance (m2h/audio/score.py holds the definition, "Spectral"): for every (recording, channel, one-second tile) the seven
// sums over the 512 x 32 bins of the tile's spectrograms G (target), E (estimate), B (baseline)
//
//   0 sum |G|^2   1 sum |E|^2   2 sum |B|^2   3 sum (|E| - |G|)^2   4 sum |E - G|^2   5 sum (|B| - |G|)^2   6 sum |B - G|^2
//
// straight from the waveforms: no frame and no spectrum is ever written to memory.  The spectrogram is the Separator's (m2h.audio.stft):
// the tile zero-extended to 16000 samples, reflect-padded by 511 inside the tile, 32 frames of 1023 samples every 512, periodic Hann,
// 1023-point DFT, bins 0 .. 511.
//
// The transform is a GEMM on the exact fp32 matrix instruction v_mfma_f32_16x16x4_f32: rows = frames (A operand: samples), columns =
// bins (B operand: the host-built table, window folded in).  The window and the DFT are both symmetric under n <-> 1023 - n (w[0] = 0),
// so with s[n] = x[n] + x[1023 - n] and d[n] = x[n] - x[1023 - n], n = 1 .. 511,
//     Re X[k] = sum_n  w[n] cos(2 pi k n / 1023) s[n]          Im X[k] = sum_n -w[n] sin(2 pi k n / 1023) d[n]
// which halves K (512 with the zero column n = 0) and the table (2 MB: it stays in L2).
//
// One 512-thread workgroup per (tile, c, r) works through the tile's two halves of 16 frames one after the other.  A half's padded
// samples of the three signals (8703 each; reflection and zero extension are index arithmetic on the way in, nothing outside the row's
// [start, start + L) is read) are staged in LDS, 103 KB; sample p sits at word p + 4 (p >> 9), so that the 16 frames x 4 samples of an A
// fragment fall into 64 different banks.  Wave w owns the bins 64 w .. 64 w + 63: four 16-bin column tiles, for each the cos and the sin
// fragment, applied to the three signals' M-tile of the same 16 frames -- 3 x 4 x (re, im) accumulators of 4 registers, so a lane holds
// Re and Im of G, E and B of the same (frame, bin) and the epilogue needs no exchange.  Per k-step of 4 samples a wave issues 6 LDS reads,
// 8 coalesced 256-byte table reads (prefetched one step ahead) and 24 MFMAs.
//
// Magnitudes and differences are fp32; every square is converted to double before it is added: a lane's 2 x 16 elements in a fixed order,
// then score.hip's reduction -- the xor butterfly of a wave, then the eight waves in order.  No atomics: the same bits on every run, and
// for any batch, stride or alignment around a recording (only the staged values enter the arithmetic).
#include "score_common.h"

namespace m2h {

namespace {

constexpr int SP_THREADS = 512, SP_WAVES = SP_THREADS / 64;
constexpr int SP_TILE = 16000, SP_PAD = 511, SP_HOP = 512, SP_KSTEPS = 128;
constexpr int SP_HALF = 16 * SP_HOP;                        // padded samples between the first frames of the two halves
constexpr int SP_SPAN = 15 * SP_HOP + 1024;                 // staged positions of a half: 8703 samples and one zero (the partner of n = 0 in the last frame)
constexpr int SP_ROW = SP_SPAN + 4 * (SP_SPAN >> 9);        // with the bank skew: 8772 words >= the largest address 8767 + 1
constexpr int SP_TABLE_BT = SP_KSTEPS * 2 * 64;             // table words per 16-bin column tile

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ double sq(float v) { return (double)v * (double)v; }

}  // namespace

__global__ __launch_bounds__(SP_THREADS) void score_spectral_kernel(ScoreSignals a, const long long* __restrict__ target, int target0, int S,
                                                                    const float* __restrict__ dft, double* __restrict__ out, int C, long long L,
                                                                    long long J, const int* __restrict__ lag, int D) {
  extern __shared__ __attribute__((aligned(16))) float smem[];          // [3][SP_ROW]
  __shared__ double red[SP_WAVES][7];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;                                        // = (r * C + c) * J + j
  const long long j = b % J, rc = b / J;
  const long long c = rc % C, r = rc / C;
  const long long t = score_target(target, target0, r, S), shift = score_lag(lag, rc, D);       // clamped to [0, S) and to [-D, D]
  const long long t0 = j * (long long)SP_TILE + D;
  const long long left = L - j * (long long)SP_TILE;
  const int n = left < SP_TILE ? (int)left : SP_TILE;                    // samples of this tile, >= 1; the rest of the second is zeros
  const float* pg = row(a.refs, r, t, c) + t0;
  const float* pe = row(a.est, r, c) + t0 + shift;
  const float* pm = row(a.mix, r, 0) + (C == 2 ? c * a.mix.sc : 0) + t0;
  const long long mix_other = C == 2 ? 0 : a.mix.sc;                      // C = 1: the baseline is the mean of the two channels

  float* sg = smem;
  float* se = smem + SP_ROW;
  float* sb = smem + 2 * SP_ROW;

  // A fragment: lane l holds A[frame l & 15][k = l >> 4]; B fragment: B[k = l >> 4][bin l & 15]; C/D: bin l & 15, frame 4 (l >> 4) + reg
  const int m = lane & 15, kq = lane >> 4;
  const int lo0 = SP_HOP * m + kq + 4 * m;                               // word of sample n = kq of frame m (then + 4 per k-step)
  const int hi0 = SP_HOP * m + 1023 - kq + 4 * (m + 1);                  // word of its partner 1023 - n (then - 4 per k-step)
  const float* tb = dft + (size_t)(4 * wave) * SP_TABLE_BT + lane;

  double sum[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) sum[k] = 0.0;

#pragma unroll 1
  for (int h = 0; h < 2; ++h) {                                          // (not unrolled: one half's accumulators live at a time)
    if (h) __syncthreads();                                              // every wave is done with the first half's samples
    static_assert(SP_SPAN % SP_THREADS == 0, "a thread stages SP_SPAN / SP_THREADS positions of each signal");
    float g[SP_SPAN / SP_THREADS], e[SP_SPAN / SP_THREADS], v[SP_SPAN / SP_THREADS];
#pragma unroll
    for (int u = 0; u < SP_SPAN / SP_THREADS; ++u) {                     // every load of the half in flight at once: the index of a
      const int q = tid + u * SP_THREADS;                               // zero is clamped to sample 0, which every tile has
      int i = h * SP_HALF + q - SP_PAD;                                  // the tile's sample behind padded position h * 8192 + q
      i = i < 0 ? -i : i;
      i = i > SP_TILE - 1 ? 2 * (SP_TILE - 1) - i : i;
      const bool ok = q < SP_SPAN - 1 && i < n;
      i = ok ? i : 0;
      const float gv = pg[i], ev = pe[i], m0 = pm[i], m1 = pm[i + mix_other];
      g[u] = ok ? gv : 0.f;
      e[u] = ok ? ev : 0.f;
      v[u] = ok ? (C == 2 ? m0 : 0.5f * (m0 + m1)) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SP_SPAN / SP_THREADS; ++u) {
      const int q = tid + u * SP_THREADS;
      const int w = q + 4 * (q >> 9);
      sg[w] = g[u];
      se[w] = e[u];
      sb[w] = v[u];
    }
    __syncthreads();

    f32x4 re[3][4], im[3][4];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) re[x][y] = im[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};

    float bc[4], bs[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      bc[y] = tb[y * SP_TABLE_BT];
      bs[y] = tb[y * SP_TABLE_BT + 64];
    }
#pragma unroll 2
    for (int ks = 0; ks < SP_KSTEPS; ++ks) {
      const int kn = ks + 1 < SP_KSTEPS ? ks + 1 : ks;                   // the next step's table fragments, in flight under this step's MFMAs
      float nc[4], ns[4];
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        nc[y] = tb[y * SP_TABLE_BT + kn * 128];
        ns[y] = tb[y * SP_TABLE_BT + kn * 128 + 64];
      }
      const int lo = lo0 + 4 * ks, hi = hi0 - 4 * ks;
      const float g0 = sg[lo], g1 = sg[hi], e0 = se[lo], e1 = se[hi], v0 = sb[lo], v1 = sb[hi];
      const float as[3] = {g0 + g1, e0 + e1, v0 + v1};
      const float ad[3] = {g0 - g1, e0 - e1, v0 - v1};
#pragma unroll
      for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 3; ++x) {
          re[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[x], bc[y], re[x][y], 0, 0, 0);
          im[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[x], bs[y], im[x][y], 0, 0, 0);
        }
#pragma unroll
      for (int y = 0; y < 4; ++y) bc[y] = nc[y], bs[y] = ns[y];
    }

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
    double s = sum[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
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
  long long J;
  if (int rc = check_signals("score_spectral", a, true, out, R, S, C, L, D, 0, 1)) return rc;
  M2H_REQUIRE(dft, "score_spectral: null pointer (dft)");
  if (int rc = check_lag("score_spectral", lag, D)) return rc;
  if (int rc = check_target("score_spectral", target, target0, S)) return rc;
  M2H_REQUIRE((reinterpret_cast<size_t>(out) & 7) == 0, "score_spectral: out must be 8-byte aligned");
  const long long Ls = L - 2ll * D;
  if (int rc = check_tiles("score_spectral", Ls, SP_TILE, (long long)R * C, J)) return rc;
  const size_t lds = sizeof(float) * 3 * SP_ROW;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(score_spectral_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail((int)e, "score_spectral: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
  M2H_LAUNCH(score_spectral_kernel, dim3((unsigned)(J * R * C)), dim3(SP_THREADS), lds, as_stream(stream), a, target, target0, S, dft, out, C, Ls, J, lag,
             D);
  return launch_status("score_spectral");
}
