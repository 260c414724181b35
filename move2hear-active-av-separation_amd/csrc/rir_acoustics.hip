// RoomAcoustics (m2h/audio/acoustics.py holds the definition): onset, direct-to-reverberant ratio, decay times, clarity and early IACC of
// a batch of binaural RIRs h [Q][Lr][2] (fp32, the ears interleaved as the Auralizer takes them), in three launches.
//
// m2h_rir_onset: one 1024-thread workgroup per RIR, two passes over the row.  Pass 1: per ear pk_e = max |h| and its first index npk_e.
// Pass 2: per ear the first n with |h| >= 0.1 pk_e (compared in fp64: 0.1 * (double)pk_e, as the reference does), T = sum h^2 and
// D = sum of h^2 over |n - npk_e| <= 40, fp64 with the product taken after widening.  A thread adds its samples in ascending n, the block
// adds the threads in a fixed tree: the same bits on every run.  No atomics.
//
// m2h_rir_band_energy: grid (segment, band, RIR), 1024 threads, the 16384-point complex transform of fft_lds.h in 128 KB of LDS.  Both
// ears ride one transform, z[m] = h[a + m][L] + i h[a + m][R] (zero outside [0, Lr)); the band's mask is real and symmetric, so the real
// and imaginary part of the filtered z ARE the two filtered ears.  Segment g starts at a = n0 - 2064 + 12256 g; the circular convolution
// with the 4097-tap zero-phase filter is wrap-free on the slots [2048, 14336), the samples [n0 - 16 + 12256 g, + 12288): 766 whole bins
// of 16 samples from slot 2064 on, with 16 samples either side for the IACF lags.  Band 0 is h itself and takes no transform.  A bin is
// added by 16 neighbouring lanes, each widening its sample to fp64 and squaring it there, through the xor-8, 4, 2, 1 exchanges.  Segment 0
// also forms the 33 lag products and the two energies of the first 80 ms: wave w owns the sums w, w + 16, w + 32; a lane adds its 20
// terms in ascending t, the wave adds the lanes through the xor-32 .. 1 exchanges.  An ear that m2h_rir_onset found silent (T = 0) is taken as
// zeros after the transform too, whose rounding would otherwise leak the other ear into it.  The bits of an RIR depend on nothing but the RIR.
//
// m2h_rir_decay: one wave per row of bins (q, ear, band).  Total by a first reduce; then the reverse scan EDC[i] = sum_{j >= i} E[j] in
// chunks of 64 bins from the end (a shuffle scan per chunk plus the carry), run twice: the first run finds, per regression range, the
// first and last bin inside it and adds the clarity sums; the second adds the regression sums about the midpoint of that span, so that
// the normal equations are well conditioned.  Nothing is stored but the 7 outputs.
#include "fft_lds.h"

namespace m2h {

namespace {
constexpr int RLOGM = 14;
constexpr int RM = 1 << RLOGM;           // transform points
constexpr int RIR_MAX_TAPS = 256000;
constexpr int RIR_BIN = 16;              // samples of an energy bin (1 ms)
constexpr int RIR_HALF = 2048;           // half length of the band filters: slots [RIR_HALF, RM - RIR_HALF) are wrap-free
constexpr int RIR_LEAD = RIR_HALF + 16;  // slot of sample n0 of segment 0
constexpr int RIR_SEG_BINS = 766;        // (RM - 2 RIR_HALF - 32) / 16
constexpr int RIR_HOP = RIR_SEG_BINS * RIR_BIN;   // 12256
constexpr int RIR_BANDS = 7;
constexpr int RIR_DIRECT = 40;           // +- 2.5 ms about the peak
constexpr int RIR_WIN = 1280;            // 80 ms
constexpr int RIR_MAXLAG = 16;           // +- 1 ms
constexpr int RIR_IACF = 2 * RIR_MAXLAG + 3;      // 33 lag sums, sum L^2, sum R^2
constexpr int RIR_PARAMS = 7;
constexpr int RIR_DECAY_ROWS = 4;        // rows (waves) per workgroup of the decay kernel

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
}  // namespace

__global__ __launch_bounds__(1024) void rir_onset_kernel(const float* __restrict__ h, int Lr, int* __restrict__ onset, int* __restrict__ peak,
                                                         double* __restrict__ sums, double* __restrict__ drr) {
  __shared__ float s_pk[2][1024];
  __shared__ int s_ix[2][1024];
  __shared__ double s_d[4][1024];
  const int tid = threadIdx.x;
  const long long q = blockIdx.x;
  const float* row = h + q * (long long)Lr * 2;

  float pk[2] = {0.f, 0.f};
  int ix[2] = {0, 0};
  for (int n = tid; n < Lr; n += 1024)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float v = fabsf(row[2 * (long long)n + e]);
      if (v > pk[e]) pk[e] = v, ix[e] = n;                  // ascending n: the first index of the thread's maximum
    }
#pragma unroll
  for (int e = 0; e < 2; ++e) s_pk[e][tid] = pk[e], s_ix[e][tid] = ix[e];
  __syncthreads();
  for (int o = 512; o >= 1; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float a = s_pk[e][tid], b = s_pk[e][tid + o];
        const int ia = s_ix[e][tid], ib = s_ix[e][tid + o];
        if (b > a || (b == a && ib < ia)) s_pk[e][tid] = b, s_ix[e][tid] = ib;
      }
    __syncthreads();
  }
  const float pke[2] = {s_pk[0][0], s_pk[1][0]};
  const int npk[2] = {pke[0] > 0.f ? s_ix[0][0] : 0, pke[1] > 0.f ? s_ix[1][0] : 0};
  __syncthreads();

  int first[2] = {Lr, Lr};
  double tot[2] = {0.0, 0.0}, dir[2] = {0.0, 0.0};
  for (int n = tid; n < Lr; n += 1024)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double v = (double)row[2 * (long long)n + e];
      if (pke[e] > 0.f && fabs(v) >= 0.1 * (double)pke[e] && n < first[e]) first[e] = n;
      tot[e] += v * v;
      if (n >= npk[e] - RIR_DIRECT && n <= npk[e] + RIR_DIRECT) dir[e] += v * v;
    }
#pragma unroll
  for (int e = 0; e < 2; ++e) s_ix[e][tid] = first[e], s_d[e][tid] = dir[e], s_d[2 + e][tid] = tot[e];
  __syncthreads();
  for (int o = 512; o >= 1; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int e = 0; e < 2; ++e) s_ix[e][tid] = min(s_ix[e][tid], s_ix[e][tid + o]);
#pragma unroll
      for (int k = 0; k < 4; ++k) s_d[k][tid] += s_d[k][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int n0 = min(s_ix[0][0], s_ix[1][0]);             // a silent ear has no onset (Lr); both silent: 0
    onset[q] = n0 < Lr ? n0 : 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double D = s_d[e][0], T = s_d[2 + e][0];
      peak[2 * q + e] = npk[e];
      sums[4 * q + 2 * e] = D;
      sums[4 * q + 2 * e + 1] = T;
      drr[2 * q + e] = pke[e] > 0.f ? 10.0 * log10(D / (T - D)) : __longlong_as_double(0x7ff8000000000000ll);
    }
  }
}

// grid (segments, 7, Q).  energy [Q][2][7][nbs], nbs = ceil(Lr / 16); iacf [Q][7][35]; iacc [Q][7][2].
__global__ __launch_bounds__(1024) void rir_band_energy_kernel(const float* __restrict__ h, int Lr, const int* __restrict__ onset,
                                                               const double* __restrict__ sums, const float* __restrict__ masks,
                                                               const cf* __restrict__ tws,
                                                               double* __restrict__ energy, double* __restrict__ iacf, double* __restrict__ iacc,
                                                               int nbs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double s_iacf[RIR_IACF];
  cf* z = reinterpret_cast<cf*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, b = blockIdx.y;
  const long long q = blockIdx.z;
  const int n0 = min(max(onset[q], 0), Lr - 1);                // (m2h_rir_onset's value lies there already)
  const long long a = (long long)n0 - RIR_LEAD + (long long)RIR_HOP * g;      // sample of slot 0
  const int bin0 = RIR_SEG_BINS * g;
  double* eL = energy + ((q * 2 + 0) * RIR_BANDS + b) * (long long)nbs;
  double* eR = energy + ((q * 2 + 1) * RIR_BANDS + b) * (long long)nbs;

  if (g > 0 && a + RIR_LEAD >= Lr) {                        // the segment's bins lie past the row (n0 stays on the device): zeros
    for (int i = tid; i < RIR_SEG_BINS; i += 1024)
      if (bin0 + i < nbs) eL[bin0 + i] = 0.0, eR[bin0 + i] = 0.0;
    return;
  }

  const float* row = h + q * (long long)Lr * 2;
#pragma unroll
  for (int i = 0; i < RM / 1024; ++i) {
    const int m = tid + 1024 * i;
    const long long n = a + m;
    const bool in = n >= 0 && n < Lr;
    z[m] = {in ? row[2 * n] : 0.f, in ? row[2 * n + 1] : 0.f};
  }
  __syncthreads();
  float sc = 1.f;
  if (b > 0) {
    fft_dif_fixed<RLOGM, 1024>(z, tws);
    const float* gm = masks + (long long)(b - 1) * RM;
#pragma unroll
    for (int i = 0; i < RM / 1024; ++i) {
      const int m = tid + 1024 * i;
      const float w = gm[bit_rev<RLOGM>(m)];                // slot m holds bin bit_rev(m)
      const cf v = z[m];
      z[m] = {v.x * w, v.y * w};
    }
    __syncthreads();
    ifft_dit_fixed<RLOGM, 1024>(z, tws);
    sc = 1.f / (float)RM;
  }
  // A silent ear (T = 0) stays silent: the ears share a transform, and its rounding would leak the other ear into it.
  const float scl = sums[4 * q + 1] > 0.0 ? sc : 0.f, scr = sums[4 * q + 3] > 0.0 ? sc : 0.f;

  // energy bins: slot RIR_LEAD + 16 i + t, 16 lanes per bin
#pragma unroll
  for (int i = 0; i < (RIR_HOP + 1023) / 1024; ++i) {
    const int u = tid + 1024 * i;                           // < 12288: slot RIR_LEAD + u < RM
    const long long n = a + RIR_LEAD + u;
    const cf v = z[RIR_LEAD + u];
    const bool in = u < RIR_HOP && n < Lr;
    const double l = in ? (double)(v.x * scl) : 0.0, r = in ? (double)(v.y * scr) : 0.0;
    double pl = l * l, pr = r * r;
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) pl += __shfl_xor(pl, o, 64), pr += __shfl_xor(pr, o, 64);
    const int bin = bin0 + (u >> 4);
    if ((u & 15) == 0 && u < RIR_HOP && bin < nbs) eL[bin] = pl, eR[bin] = pr;
  }

  if (g != 0) return;
  // IACF sums over W = [n0, n0 + 1280): slots RIR_LEAD + t; k < 33: lag k - 16; 33: sum L^2; 34: sum R^2
  for (int k = wave; k < RIR_IACF; k += 16) {
    const int tau = k < 2 * RIR_MAXLAG + 1 ? k - RIR_MAXLAG : 0;
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < RIR_WIN / 64; ++j) {
      const int m = RIR_LEAD + lane + 64 * j;
      const cf v = z[m], w = z[m + tau];
      const double l = (double)(v.x * scl), r = (double)(v.y * scr), rt = (double)(w.y * scr);
      acc += k == 33 ? l * l : k == 34 ? r * r : l * rt;
    }
    acc = wave_sum(acc);
    if (lane == 0) s_iacf[k] = acc;
  }
  __syncthreads();
  double* oi = iacf + (q * RIR_BANDS + b) * RIR_IACF;
  if (tid < RIR_IACF) oi[tid] = s_iacf[tid];
  if (tid == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double den = sqrt(s_iacf[33] * s_iacf[34]);
    double best = nan, at = nan;
    if (den > 0.0) {
      best = -1.0;
      for (int k = 0; k < 2 * RIR_MAXLAG + 1; ++k) {
        const double v = fabs(s_iacf[k]) / den;
        if (v > best) best = v, at = (double)(k - RIR_MAXLAG);       // the lowest lag on ties
      }
    }
    iacc[(q * RIR_BANDS + b) * 2] = best;
    iacc[(q * RIR_BANDS + b) * 2 + 1] = at;
  }
}

// bins [rows][nb] fp64 -> out [rows][7]: edt, t20, t30, c50, c80, d50, ts.  One wave per row.
__global__ __launch_bounds__(64 * RIR_DECAY_ROWS) void rir_decay_kernel(const double* __restrict__ bins, long long rows, int nb,
                                                                        double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long rw = (long long)blockIdx.x * RIR_DECAY_ROWS + (threadIdx.x >> 6);
  if (rw >= rows) return;
  const double* E = bins + rw * (long long)nb;
  const int chunks = (nb + 63) / 64;
  const double lo[3] = {0.0, -5.0, -5.0}, hi[3] = {-10.0, -25.0, -35.0};

  double total = 0.0;
  for (int i = lane; i < nb; i += 64) total += E[i];
  total = wave_sum(total);

  // fn(i, E[i], Lv[i]) for every bin, from the last chunk to the first
  auto scan = [&](auto fn) {
    double carry = 0.0;
    for (int c = chunks - 1; c >= 0; --c) {
      const int i = c * 64 + lane;
      const double v = i < nb ? E[i] : 0.0;
      double s = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_down(s, o, 64);
        if (lane + o < 64) s += t;
      }
      const double edc = s + carry;
      const double ratio = edc / total;                     // EDC[i] <= EDC[0]: the two orders of summation may differ in the last bit
      if (i < nb) fn(i, v, 10.0 * log10(ratio > 1.0 ? 1.0 : ratio));
      carry += __shfl(s, 0, 64);
    }
  };

  int first[3] = {nb, nb, nb}, last[3] = {-1, -1, -1};
  double e50 = 0.0, l50 = 0.0, e80 = 0.0, l80 = 0.0, ts = 0.0;
  scan([&](int i, double v, double lv) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (lv <= lo[r] && lv >= hi[r]) first[r] = min(first[r], i), last[r] = max(last[r], i);
    if (i < 50) e50 += v; else l50 += v;
    if (i < 80) e80 += v; else l80 += v;
    ts += ((double)i + 0.5) / 1000.0 * v;
  });
  double pivot[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) first[r] = min(first[r], __shfl_xor(first[r], o, 64)), last[r] = max(last[r], __shfl_xor(last[r], o, 64));
    pivot[r] = 0.5 * ((double)first[r] + (double)last[r]);
  }
  e50 = wave_sum(e50), l50 = wave_sum(l50), e80 = wave_sum(e80), l80 = wave_sum(l80), ts = wave_sum(ts);

  double cnt[3] = {0, 0, 0}, sx[3] = {0, 0, 0}, sy[3] = {0, 0, 0}, sxx[3] = {0, 0, 0}, sxy[3] = {0, 0, 0};
  scan([&](int i, double v, double lv) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (lv <= lo[r] && lv >= hi[r]) {
        const double x = (double)i - pivot[r];
        cnt[r] += 1.0, sx[r] += x, sy[r] += lv, sxx[r] += x * x, sxy[r] += x * lv;
      }
  });
  double* o = out + rw * RIR_PARAMS;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double n = wave_sum(cnt[r]), x = wave_sum(sx[r]), y = wave_sum(sy[r]), xx = wave_sum(sxx[r]), xy = wave_sum(sxy[r]);
    const double slope = (n * xy - x * y) / (n * xx - x * x) * 1000.0;          // dB per second: a bin is 1 ms
    if (lane == 0) o[r] = n >= 2.0 ? -60.0 / slope : nan;
  }
  if (lane == 0) {
    o[3] = 10.0 * log10(e50 / l50);
    o[4] = 10.0 * log10(e80 / l80);
    o[5] = e50 / total;
    o[6] = ts / total;
  }
}

}  // namespace m2h

using namespace m2h;

namespace {
int check_rir(const char* what, int Q, int Lr) {
  M2H_REQUIRE(Lr >= 1 && Lr <= RIR_MAX_TAPS, "%s: Lr = %d taps; 1 .. %d are supported", what, Lr, RIR_MAX_TAPS);
  M2H_REQUIRE(Q >= 1, "%s: Q = %d RIRs; at least one is required", what, Q);
  return 0;
}
}  // namespace

extern "C" int m2h_rir_onset(const float* rirs, int* onset, int* peak, double* sums, double* drr, int Q, int Lr, m2h_stream stream) {
  M2H_REQUIRE(rirs && onset && peak && sums && drr, "rir_onset: null pointer (rirs %p, onset %p, peak %p, sums %p, drr %p)", (const void*)rirs,
              (const void*)onset, (const void*)peak, (const void*)sums, (const void*)drr);
  if (int rc = check_rir("rir_onset", Q, Lr)) return rc;
  M2H_REQUIRE(((reinterpret_cast<size_t>(sums) | reinterpret_cast<size_t>(drr)) & 7) == 0, "rir_onset: sums and drr must be 8-byte aligned");
  M2H_LAUNCH(rir_onset_kernel, dim3((unsigned)Q), dim3(1024), 0, as_stream(stream), rirs, Lr, onset, peak, sums, drr);
  return launch_status("rir_onset");
}

extern "C" int m2h_rir_band_energy(const float* rirs, const int* onset, const double* sums, const float* masks, const float* twiddles, double* energy,
                                   double* iacf, double* iacc, int Q, int Lr, m2h_stream stream) {
  M2H_REQUIRE(rirs && onset && sums && masks && twiddles && energy && iacf && iacc,
              "rir_band_energy: null pointer (rirs %p, onset %p, sums %p, masks %p, twiddles %p, energy %p, iacf %p, iacc %p)", (const void*)rirs,
              (const void*)onset, (const void*)sums, (const void*)masks, (const void*)twiddles, (const void*)energy, (const void*)iacf, (const void*)iacc);
  if (int rc = check_rir("rir_band_energy", Q, Lr)) return rc;
  M2H_REQUIRE(Q <= 65535, "rir_band_energy: Q = %d RIRs exceed the grid's 65535 per launch", Q);
  M2H_REQUIRE(((reinterpret_cast<size_t>(sums) | reinterpret_cast<size_t>(twiddles) | reinterpret_cast<size_t>(energy) | reinterpret_cast<size_t>(iacf) | reinterpret_cast<size_t>(iacc)) & 7) == 0,
              "rir_band_energy: sums, twiddles, energy, iacf and iacc must be 8-byte aligned");
  const int nbs = (Lr + RIR_BIN - 1) / RIR_BIN;
  const int segs = (nbs + RIR_SEG_BINS - 1) / RIR_SEG_BINS;
  if (int rc = reserve_transform_lds<RLOGM>(rir_band_energy_kernel, "rir_band_energy")) return rc;
  M2H_LAUNCH(rir_band_energy_kernel, dim3(segs, RIR_BANDS, Q), dim3(1024), sizeof(cf) << RLOGM, as_stream(stream), rirs, Lr, onset, sums, masks,
             reinterpret_cast<const cf*>(twiddles) + RM, energy, iacf, iacc, nbs);
  return launch_status("rir_band_energy");
}

extern "C" int m2h_rir_decay(const double* bins, double* params, long long rows, int nb, m2h_stream stream) {
  M2H_REQUIRE(bins && params, "rir_decay: null pointer (bins %p, params %p)", (const void*)bins, (const void*)params);
  M2H_REQUIRE(nb >= 1 && nb <= RIR_MAX_TAPS / RIR_BIN, "rir_decay: nb = %d bins; 1 .. %d (Lr <= %d) are supported", nb, RIR_MAX_TAPS / RIR_BIN,
              RIR_MAX_TAPS);
  M2H_REQUIRE(rows >= 1 && (rows + RIR_DECAY_ROWS - 1) / RIR_DECAY_ROWS <= 0x7fffffffLL, "rir_decay: rows = %lld; 1 .. %lld are supported", rows,
              0x7fffffffLL * RIR_DECAY_ROWS);
  M2H_REQUIRE(((reinterpret_cast<size_t>(bins) | reinterpret_cast<size_t>(params)) & 7) == 0, "rir_decay: bins and params must be 8-byte aligned");
  M2H_LAUNCH(rir_decay_kernel, dim3((unsigned)((rows + RIR_DECAY_ROWS - 1) / RIR_DECAY_ROWS)), dim3(64 * RIR_DECAY_ROWS), 0, as_stream(stream), bins,
             rows, nb, params);
  return launch_status("rir_decay");
}
