// Waveform-to-waveform separation of long binaural recordings (m2h/separate.py): the HBM-bound glue around the two DFT GEMMs
// (gfx950, fp32, wave64, 16-byte stores, no atomics).
//
// A recording [R][2][L] is cut into S = ceil(L / 16000) one-second segments (the agent's steps; samples at or past L are zero).
// Every segment is transformed on its own with the feeder's semantics (csrc/stft.hip: n_fft 1023, hop 512, periodic Hann,
// centred, reflect padding 511 taken INSIDE the zero-padded segment, 32 frames), goes through the separator networks as one
// batch row, and comes back through the evaluation path's inverse transform (n_fft 1022, length 16000) with the phase of the
// downmix spectrum D = X_left + X_right, carried as the unit phasor D / |D| ((1, 0) where |D| == 0, which is np.angle(0) = 0).
//
// Batch rows are segment-major: row n = sl * R + r for the chunk's local segment sl = s - s0, so that step s of the acoustic
// memory's recurrence is a contiguous batch of R rows.  Fixed geometry below; the entry points check what they are given.
#include "m2h_internal.h"

namespace m2h {

constexpr int SEP_SEG = 16000;    // samples per segment
constexpr int SEP_T = 32;         // frames per segment
constexpr int SEP_NB = 512;       // bins
constexpr int SEP_LD = 1024;      // GEMM row length (K and N of both DFT matrices)
constexpr int SEP_NFFT = 1023;    // forward transform
constexpr int SEP_NIFFT = 1022;   // inverse transform (2 * (bins - 1))
constexpr int SEP_HOP = 512;
constexpr int SEP_KT = 32;        // bins per workgroup of the two transposing kernels

// frames[((sl*R + r)*2 + c)*32 + t][n] = window[n] * seg[t*512 + n - 511] (reflected inside the segment), n < 1023; 0 at n = 1023.
// seg[j] = sample s*hop + j of recording r, channel c, for segment s = s0 + sl: below `end` from the buffer, 0 from `end` on.  Segment s
// starts at sample s * hop: 16000 for the plain path, 16000 / k for overlapped segments.  One thread = four consecutive n = one
// 16-byte store; the source offsets are odd by construction (n - 511), so the reads are scalar and coalesced across the wave.
// The buffer is a window: it holds the absolute samples [origin, origin + stride) of every row, sample g at
// wave[(r*2 + c)*stride + g - origin] (a live feed: m2h/separate.py, SeparatorStream).  The whole recording is the window
// stride = end = L, origin = 0.
__global__ __launch_bounds__(256) void sep_frames_kernel(const float* __restrict__ wave, const float* __restrict__ window /* [1024], [1023] = 0 */,
                                                         float* __restrict__ frames, int R, long long stride, long long origin, long long end, int hop,
                                                         int s0, int nseg) {
  const size_t total = (size_t)nseg * R * 2 * SEP_T * (SEP_LD / 4);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n0 = (int)(i % (SEP_LD / 4)) * 4;
    size_t row = i / (SEP_LD / 4);
    const int t = (int)(row % SEP_T);
    const size_t sig = row / SEP_T;            // (sl*R + r)*2 + c
    const int c = (int)(sig & 1);
    const size_t nrow = sig >> 1;
    const int r = (int)(nrow % R);
    const int sl = (int)(nrow / R);
    const long long base = (long long)(s0 + sl) * hop;
    const float* src = wave + ((size_t)r * 2 + c) * (size_t)stride;
    const float4 w = *reinterpret_cast<const float4*>(window + n0);
    const float wv[4] = {w.x, w.y, w.z, w.w};
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + e;
      float x = 0.f;
      if (n < SEP_NFFT) {
        int j = t * SEP_HOP + n - SEP_NFFT / 2;             // in [-511, 16383]
        if (j < 0) j = -j;                                  // np.pad(mode="reflect"): edge sample not repeated
        if (j >= SEP_SEG) j = 2 * (SEP_SEG - 1) - j;
        const long long g = base + j;
        if (g < end) x = wv[e] * src[g - origin];
      }
      v[e] = x;
    }
    *reinterpret_cast<float4*>(frames + row * SEP_LD + n0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// spec rows [(n*2 + c)*32 + t][1024] = [Re(512) | Im(512)]  ->  mag [n][512][32][2] = log1p|X_c|, phasor [n][512][32][2] = D / |D|
// (re, im), D = X_0 + X_1.  A transpose (rows are k-major, the outputs t-major): one workgroup stages the 64 rows x 32 bins of
// one batch row through LDS with 16-byte loads, and writes 8 KB of each output contiguously with 16-byte stores.
__global__ __launch_bounds__(256) void sep_stft_post_kernel(const float* __restrict__ spec, float* __restrict__ mag, float* __restrict__ phasor, int N) {
  __shared__ __align__(16) float tile[2 * SEP_T][2 * SEP_KT + 4];        // [c*32 + t][part*32 + kk]; row stride 68 floats keeps 16-byte alignment
  const int ktiles = SEP_NB / SEP_KT;
  const int n = blockIdx.x / ktiles;
  const int k0 = (blockIdx.x % ktiles) * SEP_KT;
  if (n >= N) return;
  const float* base = spec + (size_t)n * 2 * SEP_T * SEP_LD;
  // 64 rows x 2 parts x 8 float4 = 1024 loads
  for (int q = threadIdx.x; q < 2 * SEP_T * 2 * (SEP_KT / 4); q += 256) {
    const int v4 = q % (SEP_KT / 4);
    const int part = (q / (SEP_KT / 4)) & 1;
    const int row = q / (2 * (SEP_KT / 4));
    const float4 x = *reinterpret_cast<const float4*>(base + (size_t)row * SEP_LD + part * SEP_NB + k0 + v4 * 4);
    *reinterpret_cast<float4*>(&tile[row][part * SEP_KT + v4 * 4]) = x;
  }
  __syncthreads();
  // 32 bins x 16 frame pairs: each item = (k, t0, t0 + 1) x both channels = one float4 of each output
  for (int q = threadIdx.x; q < SEP_KT * (SEP_T / 2); q += 256) {
    const int tp = q % (SEP_T / 2);
    const int kk = q / (SEP_T / 2);
    float m[4], ph[4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int t = 2 * tp + e;
      const float re0 = tile[t][kk], im0 = tile[t][SEP_KT + kk];
      const float re1 = tile[SEP_T + t][kk], im1 = tile[SEP_T + t][SEP_KT + kk];
      m[2 * e] = log1pf(sqrtf(re0 * re0 + im0 * im0));
      m[2 * e + 1] = log1pf(sqrtf(re1 * re1 + im1 * im1));
      float dr = re0 + re1, di = im0 + im1;
      const float big = fmaxf(fabsf(dr), fabsf(di));
      if (big == 0.f) {                                     // np.angle(0) = 0
        dr = 1.f;
        di = 0.f;
      } else {
        dr /= big;                                          // |D|^2 neither overflows nor flushes to zero
        di /= big;
        const float inv = 1.f / sqrtf(dr * dr + di * di);
        dr *= inv;
        di *= inv;
      }
      ph[2 * e] = dr;
      ph[2 * e + 1] = di;
    }
    const size_t o = (((size_t)n * SEP_NB + k0 + kk) * SEP_T + 2 * tp) * 2;
    *reinterpret_cast<float4*>(mag + o) = make_float4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4*>(phasor + o) = make_float4(ph[0], ph[1], ph[2], ph[3]);
  }
}

// P [n][512][32][1] (log1p magnitude from the networks), phasor [n][512][32][2]  ->  rows [n*32 + t][1024]:
// [k] = expm1(max(P, 0)) * re, [512 + k] = expm1(max(P, 0)) * im.  The transpose of the kernel above, again through LDS.
__global__ __launch_bounds__(256) void sep_istft_pre_kernel(const float* __restrict__ P, const float* __restrict__ phasor, float* __restrict__ rows, int N) {
  __shared__ float tile[2][SEP_KT][SEP_T + 1];              // [part][kk][t]
  const int ktiles = SEP_NB / SEP_KT;
  const int n = blockIdx.x / ktiles;
  const int k0 = (blockIdx.x % ktiles) * SEP_KT;
  if (n >= N) return;
  {
    // 32 bins x 32 frames, contiguous in both inputs: one float4 of P and two of the phasor per thread
    const int q = threadIdx.x;                              // 256 x 4 = 1024 elements
    const size_t e0 = ((size_t)n * SEP_NB + k0) * SEP_T + (size_t)q * 4;
    const float4 p = *reinterpret_cast<const float4*>(P + e0);
    const float4 a = *reinterpret_cast<const float4*>(phasor + e0 * 2);
    const float4 b = *reinterpret_cast<const float4*>(phasor + e0 * 2 + 4);
    const float pv[4] = {p.x, p.y, p.z, p.w};
    const float re[4] = {a.x, a.z, b.x, b.z}, im[4] = {a.y, a.w, b.y, b.w};
    const int kk = (q * 4) / SEP_T, t0 = (q * 4) % SEP_T;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float m = expm1f(fmaxf(pv[e], 0.f));
      tile[0][kk][t0 + e] = m * re[e];
      tile[1][kk][t0 + e] = m * im[e];
    }
  }
  __syncthreads();
  // 32 frames x 2 parts x 8 float4 = 512 stores
  for (int q = threadIdx.x; q < SEP_T * 2 * (SEP_KT / 4); q += 256) {
    const int v4 = q % (SEP_KT / 4);
    const int part = (q / (SEP_KT / 4)) & 1;
    const int t = q / (2 * (SEP_KT / 4));
    const float4 x = make_float4(tile[part][v4 * 4][t], tile[part][v4 * 4 + 1][t], tile[part][v4 * 4 + 2][t], tile[part][v4 * 4 + 3][t]);
    *reinterpret_cast<float4*>(rows + ((size_t)n * SEP_T + t) * SEP_LD + part * SEP_NB + k0 + v4 * 4) = x;
  }
}

// The binaural target (m2h/separate.py, output="binaural"): the mixture's own spectrum of channel c scaled by the clamped mask of the
// first U-Net.  spec rows [(n*2 + c)*32 + t][1024] = [Re | Im], masks BHWC [n][512][32][2]  ->  rows, same shape and row order:
// [k] = max(masks[n][k][t][c], 0) * Re, [512 + k] = max(masks[n][k][t][c], 0) * Im -- the inverse GEMM's operand for 2N signals.
// Masks are bin-major and rows frame-major: the workgroup's 8 KB of masks are read contiguously and transposed through LDS.
// rows == spec is allowed (no __restrict__ on either): a workgroup owns the 64 rows x 2 x 32 columns it reads, all of its loads are
// issued before the barrier and all of its stores after it, and every thread stores to the addresses it loaded from.
__global__ __launch_bounds__(256) void sep_bin_rows_kernel(const float* spec, const float* __restrict__ masks, float* rows, int N) {
  __shared__ float tile[2][SEP_KT][SEP_T + 1];              // [c][kk][t]
  const int ktiles = SEP_NB / SEP_KT;
  const int n = blockIdx.x / ktiles;
  const int k0 = (blockIdx.x % ktiles) * SEP_KT;
  if (n >= N) return;
  const size_t base = (size_t)n * 2 * SEP_T * SEP_LD;
  // 64 rows x 2 parts x 8 float4 = 1024 loads, four per thread, kept in registers across the barrier
  float4 x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = threadIdx.x + i * 256;
    const int v4 = q % (SEP_KT / 4);
    const int part = (q / (SEP_KT / 4)) & 1;
    const int row = q / (2 * (SEP_KT / 4));
    x[i] = *reinterpret_cast<const float4*>(spec + base + (size_t)row * SEP_LD + part * SEP_NB + k0 + v4 * 4);
  }
  // 32 bins x 32 frames x 2 channels, contiguous: two float4 per thread, each = (t, c0), (t, c1), (t + 1, c0), (t + 1, c1) of one bin
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = threadIdx.x + i * 256;
    const float4 m = *reinterpret_cast<const float4*>(masks + (((size_t)n * SEP_NB + k0) * SEP_T * 2 + (size_t)q * 4));
    const int kk = q / (SEP_T / 2), t = (q % (SEP_T / 2)) * 2;
    tile[0][kk][t] = fmaxf(m.x, 0.f);
    tile[1][kk][t] = fmaxf(m.y, 0.f);
    tile[0][kk][t + 1] = fmaxf(m.z, 0.f);
    tile[1][kk][t + 1] = fmaxf(m.w, 0.f);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = threadIdx.x + i * 256;
    const int v4 = q % (SEP_KT / 4);
    const int part = (q / (SEP_KT / 4)) & 1;
    const int row = q / (2 * (SEP_KT / 4));            // c*32 + t
    const int c = row / SEP_T, t = row % SEP_T;
    const float4 y = make_float4(tile[c][v4 * 4][t] * x[i].x, tile[c][v4 * 4 + 1][t] * x[i].y, tile[c][v4 * 4 + 2][t] * x[i].z,
                                 tile[c][v4 * 4 + 3][t] * x[i].w);
    *reinterpret_cast<float4*>(rows + base + (size_t)row * SEP_LD + part * SEP_NB + k0 + v4 * 4) = y;
  }
}

// Sample j of one segment's inverse transform: fr = the segment's 32 rows of the inverse GEMM, at most two frames cover a sample.
__device__ __forceinline__ float sep_ola_sample(const float* __restrict__ fr, const float* __restrict__ window /* [1022] */, int j) {
  const int jj = j + SEP_NIFFT / 2;
  float acc = 0.f, wss = 0.f;
  int t1 = jj / SEP_HOP;
  if (t1 > SEP_T - 1) t1 = SEP_T - 1;
  for (int t = t1; t >= 0; --t) {
    const int n = jj - t * SEP_HOP;
    if (n >= SEP_NIFFT) break;
    const float w = window[n];
    acc += fr[(size_t)t * SEP_LD + n] * w;
    wss += w * w;
  }
  return wss > 1.1754944e-38f ? acc / wss : acc;
}

// Windowed overlap-add as a gather (istft_ola_kernel's arithmetic), every segment written at its offset of y [R][L] and cut at L:
// y[r][(s0 + sl)*16000 + j] = (sum_t frames[(sl*R + r)*32 + t][jj - 512 t] * window[jj - 512 t]) / wss(jj), jj = j + 511.
// One thread = four consecutive j: one 16-byte store where the destination is aligned (always when L % 4 == 0) and inside L.
// y is a window: it holds the absolute samples [origin, origin + stride) of every row, sample n at y[r*stride + n - origin], cut at
// L = the samples received; the whole recording is stride = L, origin = 0.
__global__ __launch_bounds__(256) void sep_istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ window /* [1022] */,
                                                            float* __restrict__ y, int R, long long stride, long long origin, long long L, int s0,
                                                            int nseg) {
  const size_t total = (size_t)nseg * R * (SEP_SEG / 4);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j0 = (int)(i % (SEP_SEG / 4)) * 4;
    const size_t nrow = i / (SEP_SEG / 4);                  // sl*R + r
    const int r = (int)(nrow % R);
    const int sl = (int)(nrow / R);
    const long long g0 = (long long)(s0 + sl) * SEP_SEG + j0;
    if (g0 >= L) continue;
    const float* fr = frames + nrow * SEP_T * SEP_LD;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = sep_ola_sample(fr, window, j0 + e);
    float* dst = y + (size_t)r * (size_t)stride + (g0 - origin);
    if (g0 + 4 <= L && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (g0 + e < L) dst[e] = v[e];
    }
  }
}

// Overlapped segments (segment s covers samples [s*hop, s*hop + 16000), hop = 16000 / k) cross-faded into y [R][L]:
// y[r][n] = sum_s xwin[n - s*hop] * v_s[n - s*hop] / W[n], W[n] = sum_s xwin[n - s*hop] over all segments 0 <= s < S of the recording
// that cover n, v_s = the segment's inverse transform (sep_ola_sample).  A gather: one thread = four consecutive n of the span
// [s0*hop, min(L, (s0 + nseg - 1)*hop + 16000)) the chunk's segments cover; hop % 4 == 0, so the four share their covering segments.
// The chunk's covering segments are added in ascending order onto 0 when the chunk holds the sample's first covering segment and
// onto y[n] otherwise: chunks come in ascending order, y needs no clearing, and the order of the additions is the same for any chunking.
// y is a window: it holds the absolute samples [origin, origin + stride) of every row, sample n at y[r*stride + n - origin]; on a live
// feed the partial sums of the samples that later segments still cover stay there between calls, and L = the samples received so far:
// a sample below it is covered by no segment past S - 1 = ceil(L / hop) - 1 whatever arrives later, so W[n] is final.  The whole
// recording is stride = L, origin = 0.
__global__ __launch_bounds__(256) void sep_istft_xfade_kernel(const float* __restrict__ frames, const float* __restrict__ window /* [1022] */,
                                                              const float* __restrict__ xwin /* [16000] */, float* y, int R, long long stride,
                                                              long long origin, long long L, int hop, int s0, int nseg, long long S) {
  const long long n_first = (long long)s0 * hop;
  long long n_end = (long long)(s0 + nseg - 1) * hop + SEP_SEG;
  if (n_end > L) n_end = L;
  const size_t quads = (size_t)((n_end - n_first + 3) / 4);
  const size_t total = quads * R;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / quads);
    const long long n0 = n_first + (long long)(i % quads) * 4;
    // segments of the recording that cover n0 .. n0 + 3: s*hop <= n < s*hop + 16000
    const long long a = n0 < SEP_SEG ? 0 : (n0 - SEP_SEG) / hop + 1;
    long long b = n0 / hop;
    if (b > S - 1) b = S - 1;
    float W[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long s = a; s <= b; ++s) {
      const float4 w = *reinterpret_cast<const float4*>(xwin + (n0 - s * hop));
      W[0] += w.x;
      W[1] += w.y;
      W[2] += w.z;
      W[3] += w.w;
    }
    float* dst = y + (size_t)r * (size_t)stride + (n0 - origin);
    const bool wide = n0 + 4 <= L && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (a < s0) {                                           // earlier chunks have added their segments already
      if (wide) {
        const float4 p = *reinterpret_cast<const float4*>(dst);
        acc[0] = p.x, acc[1] = p.y, acc[2] = p.z, acc[3] = p.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n0 + e < L) acc[e] = dst[e];
      }
    }
    const int lo = a < s0 ? s0 : (int)a;
    const int hi = b > s0 + nseg - 1 ? s0 + nseg - 1 : (int)b;
    for (int s = lo; s <= hi; ++s) {
      const int j0 = (int)(n0 - (long long)s * hop);        // in [0, 16000), a multiple of 4
      const float* fr = frames + ((size_t)(s - s0) * R + r) * SEP_T * SEP_LD;
      const float4 w = *reinterpret_cast<const float4*>(xwin + j0);
      const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += sep_ola_sample(fr, window, j0 + e) * (wv[e] / W[e]);
    }
    if (wide) {
      *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n0 + e < L) dst[e] = acc[e];
    }
  }
}

static inline unsigned sep_grid(size_t total) {
  size_t g = (total + 255) / 256;
  if (g > 16384) g = 16384;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// hop = 16000 / k for k in {1, 2, 4}
static inline bool sep_hop_ok(int hop) { return hop == SEP_SEG || hop == SEP_SEG / 2 || hop == SEP_SEG / 4; }

// rows [R][cap] hold the absolute samples [origin, origin + cap); `end` samples have been received; segments [s0, s0 + nseg) lie
// inside the ceil(end / hop) segments, batch rows within int range
static inline bool sep_win_ok(int R, long long cap, long long origin, long long end, int hop, int s0, int nseg) {
  if (R <= 0 || cap <= 0 || origin < 0 || end <= 0 || s0 < 0 || nseg <= 0) return false;
  if (end > (1LL << 40) || cap > (1LL << 40) || (long long)R * cap > (1LL << 44)) return false;
  if ((long long)s0 + nseg > (end + hop - 1) / hop) return false;
  return (long long)nseg * R <= (1 << 20);
}

// the samples below `end` that segments [s0, s0 + nseg) cover lie inside the window
static inline bool sep_win_holds(long long cap, long long origin, long long end, int hop, int s0, int nseg) {
  const long long first = (long long)s0 * hop;
  long long stop = (long long)(s0 + nseg - 1) * hop + SEP_SEG;
  if (stop > end) stop = end;
  return first >= origin && stop <= origin + cap;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The runners: the checks, the grid and the launch of one kernel, for the entry point `name` (a string literal: it is the label
// m2h_last_kernel reports).  A whole-recording entry passes cap = end = L, origin = 0.
static int sep_window_check(const char* name, int R, long long cap, long long origin, long long end, int hop, int s0, int nseg) {
  M2H_REQUIRE(sep_hop_ok(hop), "%s: hop must be 16000, 8000 or 4000, got %d", name, hop);
  M2H_REQUIRE(sep_win_ok(R, cap, origin, end, hop, s0, nseg), "%s: bad sizes (R %d, cap %lld, origin %lld, end %lld, hop %d, segments [%d, %d + %d))", name, R, cap,
              origin, end, hop, s0, s0, nseg);
  M2H_REQUIRE(sep_win_holds(cap, origin, end, hop, s0, nseg), "%s: segments [%d, %d + %d) at hop %d leave the window [%lld, %lld + %lld) (end %lld)", name, s0, s0, nseg,
              hop, origin, origin, cap, end);
  return 0;
}

static int sep_frames_run(const char* name, const float* buf, const float* window, float* frames, int R, long long cap, long long origin, long long end, int hop,
                          int s0, int nseg, m2h_stream stream) {
  M2H_REQUIRE(buf && window && frames, "%s: null pointer", name);
  if (const int rc = sep_window_check(name, R, cap, origin, end, hop, s0, nseg)) return rc;
  M2H_REQUIRE(aligned16(window) && aligned16(frames), "%s: window / frames must be 16-byte aligned", name);
  M2H_LAUNCH(sep_frames_kernel, dim3(sep_grid((size_t)nseg * R * 2 * SEP_T * (SEP_LD / 4))), dim3(256), 0, as_stream(stream), buf, window, frames, R, cap, origin,
             end, hop, s0, nseg);
  return launch_status(name);
}

static int sep_istft_ola_run(const char* name, const float* frames, const float* window, float* y, int R, long long cap, long long origin, long long end, int s0,
                             int nseg, m2h_stream stream) {
  M2H_REQUIRE(frames && window && y, "%s: null pointer", name);
  if (const int rc = sep_window_check(name, R, cap, origin, end, SEP_SEG, s0, nseg)) return rc;
  M2H_LAUNCH(sep_istft_ola_kernel, dim3(sep_grid((size_t)nseg * R * (SEP_SEG / 4))), dim3(256), 0, as_stream(stream), frames, window, y, R, cap, origin, end, s0,
             nseg);
  return launch_status(name);
}

static int sep_istft_xfade_run(const char* name, const float* frames, const float* window, const float* xwin, float* y, int R, long long cap, long long origin,
                               long long end, int hop, int s0, int nseg, m2h_stream stream) {
  M2H_REQUIRE(frames && window && xwin && y, "%s: null pointer", name);
  if (const int rc = sep_window_check(name, R, cap, origin, end, hop, s0, nseg)) return rc;
  M2H_REQUIRE(aligned16(xwin), "%s: the cross-fade window must be 16-byte aligned", name);
  const long long S = (end + hop - 1) / hop;
  long long n_end = (long long)(s0 + nseg - 1) * hop + SEP_SEG;
  if (n_end > end) n_end = end;
  const size_t quads = (size_t)((n_end - (long long)s0 * hop + 3) / 4);
  M2H_LAUNCH(sep_istft_xfade_kernel, dim3(sep_grid(quads * R)), dim3(256), 0, as_stream(stream), frames, window, xwin, y, R, cap, origin, end, hop, s0, nseg, S);
  return launch_status(name);
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_sep_frames(const float* wave, const float* window, float* frames, int R, long long L, int s0, int nseg, m2h_stream stream) {
  return sep_frames_run("sep_frames", wave, window, frames, R, L, 0, L, SEP_SEG, s0, nseg, stream);
}

int m2h_sep_stft_post(const float* spec, float* mag, float* phasor, int N, m2h_stream stream) {
  M2H_REQUIRE(spec && mag && phasor, "sep_stft_post: null pointer");
  M2H_REQUIRE(N > 0 && N <= (1 << 20), "sep_stft_post: bad sizes (N %d)", N);
  M2H_REQUIRE(aligned16(spec) && aligned16(mag) && aligned16(phasor), "sep_stft_post: buffers must be 16-byte aligned");
  M2H_LAUNCH(sep_stft_post_kernel, dim3((unsigned)N * (SEP_NB / SEP_KT)), dim3(256), 0, as_stream(stream), spec, mag, phasor, N);
  return launch_status("sep_stft_post");
}

int m2h_sep_istft_pre(const float* P, const float* phasor, float* rows, int N, m2h_stream stream) {
  M2H_REQUIRE(P && phasor && rows, "sep_istft_pre: null pointer");
  M2H_REQUIRE(N > 0 && N <= (1 << 20), "sep_istft_pre: bad sizes (N %d)", N);
  M2H_REQUIRE(aligned16(P) && aligned16(phasor) && aligned16(rows), "sep_istft_pre: buffers must be 16-byte aligned");
  M2H_LAUNCH(sep_istft_pre_kernel, dim3((unsigned)N * (SEP_NB / SEP_KT)), dim3(256), 0, as_stream(stream), P, phasor, rows, N);
  return launch_status("sep_istft_pre");
}

int m2h_sep_bin_rows(const float* spec, const float* masks, float* rows, int N, m2h_stream stream) {
  M2H_REQUIRE(spec && masks && rows, "sep_bin_rows: null pointer");
  M2H_REQUIRE(N > 0 && N <= (1 << 20), "sep_bin_rows: bad sizes (N %d)", N);
  M2H_REQUIRE(aligned16(spec) && aligned16(masks) && aligned16(rows), "sep_bin_rows: buffers must be 16-byte aligned");
  M2H_LAUNCH(sep_bin_rows_kernel, dim3((unsigned)N * (SEP_NB / SEP_KT)), dim3(256), 0, as_stream(stream), spec, masks, rows, N);
  return launch_status("sep_bin_rows");
}

int m2h_sep_istft_ola(const float* frames, const float* window, float* y, int R, long long L, int s0, int nseg, m2h_stream stream) {
  return sep_istft_ola_run("sep_istft_ola", frames, window, y, R, L, 0, L, s0, nseg, stream);
}

int m2h_sep_frames_hop(const float* wave, const float* window, float* frames, int R, long long L, int hop, int s0, int nseg, m2h_stream stream) {
  return sep_frames_run("sep_frames_hop", wave, window, frames, R, L, 0, L, hop, s0, nseg, stream);
}

int m2h_sep_istft_xfade(const float* frames, const float* window, const float* xwin, float* y, int R, long long L, int hop, int s0, int nseg,
                        m2h_stream stream) {
  return sep_istft_xfade_run("sep_istft_xfade", frames, window, xwin, y, R, L, 0, L, hop, s0, nseg, stream);
}

// ---- window forms: a live feed, block by block (m2h/separate.py, SeparatorStream)

int m2h_sep_frames_win(const float* buf, const float* window, float* frames, int R, long long cap, long long origin, long long end, int hop, int s0,
                       int nseg, m2h_stream stream) {
  return sep_frames_run("sep_frames_win", buf, window, frames, R, cap, origin, end, hop, s0, nseg, stream);
}

int m2h_sep_istft_ola_win(const float* frames, const float* window, float* y, int R, long long cap, long long origin, long long end, int s0, int nseg,
                          m2h_stream stream) {
  return sep_istft_ola_run("sep_istft_ola_win", frames, window, y, R, cap, origin, end, s0, nseg, stream);
}

int m2h_sep_istft_xfade_win(const float* frames, const float* window, const float* xwin, float* y, int R, long long cap, long long origin, long long end,
                            int hop, int s0, int nseg, m2h_stream stream) {
  return sep_istft_xfade_run("sep_istft_xfade_win", frames, window, xwin, y, R, cap, origin, end, hop, s0, nseg, stream);
}

}  // extern "C"

