// The Scorer's tile spectrogram, stated once for score_spectral.hip (three signals: target, estimate, baseline), score_spatial.hip and
// score_itd.hip (the two ears of one signal).  It is the Separator's (m2h.audio.stft): the one-second tile zero-extended to 16000
// samples, reflect-padded by 511 inside the tile, 32 frames of 1023 samples every 512, periodic Hann, 1023-point DFT, bins 0 .. 511.  No
// frame and no spectrum is ever written to memory.
//
// The transform is a GEMM on the exact fp32 matrix instruction v_mfma_f32_16x16x4_f32: rows = frames (A operand: samples), columns =
// bins (B operand: the host-built table, window folded in).  The window and the DFT are both symmetric under n <-> 1023 - n (w[0] = 0),
// so with s[n] = x[n] + x[1023 - n] and d[n] = x[n] - x[1023 - n], n = 1 .. 511,
//     Re X[k] = sum_n  w[n] cos(2 pi k n / 1023) s[n]          Im X[k] = sum_n -w[n] sin(2 pi k n / 1023) d[n]
// which halves K (512 with the zero column n = 0) and the table (2 MB: it stays in L2).
//
// A 512-thread workgroup works through a tile's two halves of 16 frames one after the other.  stft_stage puts a half's padded samples of
// its NS signals (8703 each; reflection and zero extension are index arithmetic on the way in, nothing outside the row's
// [start, start + L) is read) into LDS, NS rows of 8772 words; sample p sits at word p + 4 (p >> 9), so that the 16 frames x 4 samples
// of an A fragment fall into 64 different banks.  stft_half is one wave's share: wave w owns the bins 64 w .. 64 w + 63, four 16-bin
// column tiles, for each the cos and the sin fragment, applied to the NS signals' M-tile of the same 16 frames -- NS x 4 x (re, im)
// accumulators of 4 registers, so a lane holds Re and Im of every signal at the same (frame, bin) and an epilogue needs no exchange.
// Per k-step of 4 samples a wave issues 2 NS LDS reads, 8 coalesced 256-byte table reads (prefetched one step ahead) and 8 NS MFMAs.
// Only the staged values enter the arithmetic: the same bits for any batch, stride or alignment around a recording.
//
// stft_half<NS, NY> is the same with NY column tiles per wave, wave w owning the bins 16 NY w .. 16 NY (w + 1) - 1: NY = 4, the default,
// is all 512 bins and what is written above; score_itd.hip needs the bins 0 .. 255 only and runs NY = 2 -- half the table reads, MFMAs
// and accumulators, the same LDS reads.
#pragma once
#include "score_common.h"

namespace m2h {

namespace {

constexpr int STFT_THREADS = 512;
constexpr int STFT_TILE = 16000, STFT_PAD = 511, STFT_HOP = 512, STFT_KSTEPS = 128;
constexpr int STFT_HALF = 16 * STFT_HOP;                    // padded samples between the first frames of the two halves
constexpr int STFT_SPAN = 15 * STFT_HOP + 1024;             // staged positions of a half: 8703 samples and one zero (the partner of n = 0 in the last frame)
constexpr int STFT_ROW = STFT_SPAN + 4 * (STFT_SPAN >> 9);  // with the bank skew: 8772 words >= the largest address 8767 + 1
constexpr int STFT_TABLE_BT = STFT_KSTEPS * 2 * 64;         // table words per 16-bin column tile

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Half h of a tile of n samples (1 .. 16000; the rest of the second is zeros) into smem [NS][STFT_ROW].  load(i, x) reads the tile's
// sample i < n of the NS signals: what a signal is, is the kernel's.  The caller's barrier follows.
template <int NS, class Load>
__device__ __forceinline__ void stft_stage(float* smem, int h, int n, int tid, Load load) {
  static_assert(STFT_SPAN % STFT_THREADS == 0, "a thread stages STFT_SPAN / STFT_THREADS positions of each signal");
  float v[NS][STFT_SPAN / STFT_THREADS];
#pragma unroll
  for (int u = 0; u < STFT_SPAN / STFT_THREADS; ++u) {                   // every load of the half in flight at once: the index of a
    const int q = tid + u * STFT_THREADS;                               // zero is clamped to sample 0, which every tile has
    int i = h * STFT_HALF + q - STFT_PAD;                                // the tile's sample behind padded position h * 8192 + q
    i = i < 0 ? -i : i;
    i = i > STFT_TILE - 1 ? 2 * (STFT_TILE - 1) - i : i;
    const bool ok = q < STFT_SPAN - 1 && i < n;
    i = ok ? i : 0;
    float x[NS];
    load(i, x);
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s][u] = ok ? x[s] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < STFT_SPAN / STFT_THREADS; ++u) {
    const int q = tid + u * STFT_THREADS;
    const int w = q + 4 * (q >> 9);
#pragma unroll
    for (int s = 0; s < NS; ++s) (smem + s * STFT_ROW)[w] = v[s][u];
  }
}

// The staged half's 16 frames x the wave's 16 NY bins: re[s][y], im[s][y] of signal s and column tile y, from zero.  The lane's addresses are
// formed in here (and hoisted out of the caller's loop over the halves): handed in as a struct from a helper, the k-loop comes out scheduled
// differently and score_spectral_kernel 1 % slower (profiles/score_stft_isa.txt).
template <int NS, int NY = 4>
__device__ __forceinline__ void stft_half(const float* smem, const float* dft, int lane, int wave, f32x4 (&re)[NS][NY], f32x4 (&im)[NS][NY]) {
  // A fragment: lane l holds A[frame l & 15][k = l >> 4]; B fragment: B[k = l >> 4][bin l & 15]; C/D: bin l & 15, frame 4 (l >> 4) + reg
  const int m = lane & 15, kq = lane >> 4;
  const int lo0 = STFT_HOP * m + kq + 4 * m;                             // word of sample n = kq of frame m (then + 4 per k-step)
  const int hi0 = STFT_HOP * m + 1023 - kq + 4 * (m + 1);                // word of its partner 1023 - n (then - 4 per k-step)
  const float* tb = dft + (size_t)(NY * wave) * STFT_TABLE_BT + lane;
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int y = 0; y < NY; ++y) re[s][y] = im[s][y] = f32x4{0.f, 0.f, 0.f, 0.f};

  float bc[NY], bs[NY];
#pragma unroll
  for (int y = 0; y < NY; ++y) {
    bc[y] = tb[y * STFT_TABLE_BT];
    bs[y] = tb[y * STFT_TABLE_BT + 64];
  }
#pragma unroll 2
  for (int ks = 0; ks < STFT_KSTEPS; ++ks) {
    const int kn = ks + 1 < STFT_KSTEPS ? ks + 1 : ks;                   // the next step's table fragments, in flight under this step's MFMAs
    float nc[NY], ns[NY];
#pragma unroll
    for (int y = 0; y < NY; ++y) {
      nc[y] = tb[y * STFT_TABLE_BT + kn * 128];
      ns[y] = tb[y * STFT_TABLE_BT + kn * 128 + 64];
    }
    const int lo = lo0 + 4 * ks, hi = hi0 - 4 * ks;
    float as[NS], ad[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float x0 = (smem + s * STFT_ROW)[lo], x1 = (smem + s * STFT_ROW)[hi];
      as[s] = x0 + x1;
      ad[s] = x0 - x1;
    }
#pragma unroll
    for (int y = 0; y < NY; ++y)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        re[s][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[s], bc[y], re[s][y], 0, 0, 0);
        im[s][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[s], bs[y], im[s][y], 0, 0, 0);
      }
#pragma unroll
    for (int y = 0; y < NY; ++y) bc[y] = nc[y], bs[y] = ns[y];
  }
}

// Host.  The checks the two entry points share, in their order; Ls = the scored samples per row, J = its tiles in each of `rows` rows.
inline int check_stft(const char* what, const ScoreSignals& a, const long long* target, int target0, const float* dft, const double* out, int R, int S,
                      int C, long long L, const int* lag, int D, long long rows, long long& Ls, long long& J) {
  if (int rc = check_signals(what, a, true, out, R, S, C, L, D, 0, 1)) return rc;
  M2H_REQUIRE(dft, "%s: null pointer (dft)", what);
  if (int rc = check_lag(what, lag, D)) return rc;
  if (int rc = check_target(what, target, target0, S)) return rc;
  M2H_REQUIRE((reinterpret_cast<size_t>(out) & 7) == 0, "%s: out must be 8-byte aligned", what);
  Ls = L - 2ll * D;
  return check_tiles(what, Ls, STFT_TILE, rows, J);
}

// NS staged rows are more than 64 KB of dynamic LDS: the kernel has to be given leave.
template <int NS, class K>
int reserve_stft_lds(K* kernel, const char* what, size_t& lds) {
  lds = sizeof(float) * NS * STFT_ROW;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail((int)e, "%s: cannot reserve %zu bytes of LDS: %s", what, lds, hipGetErrorString(e));
  return 0;
}

}  // namespace

}  // namespace m2h
