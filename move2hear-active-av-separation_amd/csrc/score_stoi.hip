// Scorer, STOI and ESTOI (m2h/audio/score.py holds the definition, "STOI"): gfx950, wave64, no atomics, no scratch, every sum in
// a fixed order, no host synchronisation -- the kept-frame count K of a range never leaves the device, every grid is sized for "every
// frame kept" and a workgroup beyond K leaves at once.
//
// m2h_stoi_resample   the three signals of (r, c) -- clean x = the target, the estimate y at its lag, the baseline b -- read in place over
//                     the region [D, L - D) and converted 16 kHz -> 10 kHz: one output per thread, the k = 0 .. 32 fmaf chain of
//                     m2h_resample_poly (same table, same order, zero outside the region), so the bits are Resampler(16000, 10000)'s.
// m2h_stoi_ranges     five launches over a table of ranges [start, end) of the 10 kHz signals (the whole recording and every window):
//   stoi_energy       a wave per frame of the clean signal: 256 fp32 products w x, squared and added in fp64 (4 per lane in order, then
//                     the xor butterfly)
//   stoi_mask         a workgroup per (range, r, c): the largest energy, the keep mask e_f > max - 40 dB, and its exclusive scan (wave
//                     ballots, 256 frames a step) -> the list of kept frames and K
//   stoi_envelope     a workgroup of 128 threads per output frame t < K - 1: the kept frames t - 1, t, t + 1 of each signal are gathered
//                     through the list, windowed and overlap-added (two fp32 products added: the order cannot matter), windowed again,
//                     and transformed as ONE packed 256-point complex transform per signal in LDS (fft_lds.h: the 512-point real
//                     transform of 256 samples and 256 zeros); bins 7 .. 218 are unpacked, |S|^2 converted to fp64 and added band by
//                     band in bin order; sqrt.  No frame, no overlap-added signal and no spectrum goes to memory.
//   stoi_segments     a thread per segment m (30 envelope columns x 15 bands): step 3 of the definition in fp64 for y and for b, every
//                     sum sequential in column / band order
//   stoi_mean         a workgroup per (range, r, c): the segments' values added (thread tid takes segments tid, tid + 256, ... in order,
//                     then a fixed tree), divided by their count; the six numbers
// A range's slots (one per frame) start at its own offset in the work buffers, so that a window of 77 frames does not cost the 46 874
// slots of a ten-minute whole; a workgroup finds its range by bisection of the offsets.  Whatever the table holds, no address leaves a
// buffer: starts, ends, offsets, frame counts, list entries and K are clamped where they are read.
#include "fft_lds.h"
#include "score_common.h"

namespace m2h {

namespace {

constexpr int ST_UP = 5, ST_DOWN = 8, ST_HALF = 80, ST_T = 33;       // 16 kHz -> 10 kHz: m2h.audio.resample.design(16000, 10000)
constexpr int ST_FRAME = 256, ST_HOP = 128, ST_LOGM = 8;             // frames; the packed transform holds 2^8 complex points
constexpr int ST_BANDS = 15, ST_SEG = 30;
constexpr int ST_BIN0 = 7, ST_NBINS = 212;                           // the bands cover the bins 7 .. 218
constexpr int ST_ENV_THREADS = 128, ST_BLOCK = 256;
constexpr double ST_EPS = 2.220446049250313e-16;                     // 2^-52
constexpr double ST_CLIP = 6.623413251903491;                        // 1 + 10^(15 / 20)
constexpr double ST_RANGE_DB = 40.0;
__constant__ int st_edges[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

struct StoiRange { long long start, n, off; int nf; };

// Frames of a range of n samples: starts 0, 128, ... < n - 256 (the end is exclusive).
__device__ __forceinline__ long long frames_of(long long n) { return n > ST_FRAME ? (n - ST_FRAME + ST_HOP - 1) / ST_HOP : 0; }
__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Range q of the table [NR][3] (start, end, slot offset), clamped: [start, start + n) inside [0, L10), nf frames in the slots [off, off + nf)
// inside [0, Ftot).
__device__ __forceinline__ StoiRange stoi_range(const long long* __restrict__ ranges, int q, long long L10, long long Ftot) {
  StoiRange g;
  g.start = clampll(ranges[3 * q], 0, L10);
  g.n = clampll(ranges[3 * q + 1], g.start, L10) - g.start;
  g.off = clampll(ranges[3 * q + 2], 0, Ftot);
  const long long nf = frames_of(g.n);
  g.nf = (int)(nf < Ftot - g.off ? nf : Ftot - g.off);
  return g;
}

// The last range whose offset is <= slot (the offsets ascend; any other table still gives a q in [0, NR)).
__device__ __forceinline__ int stoi_find(const long long* __restrict__ ranges, int NR, long long slot) {
  int lo = 0, hi = NR - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ranges[3 * mid + 2] <= slot) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// K and the "clean signal is silent" flag of (rc, q), K clamped to the range's frames.
__device__ __forceinline__ int stoi_kept(const int* __restrict__ kept, long long rq, int nf, bool& silent) {
  const int k = kept[2 * rq];
  silent = kept[2 * rq + 1] != 0;
  return k < 0 ? 0 : (k > nf ? nf : k);
}

}  // namespace

__global__ __launch_bounds__(ST_BLOCK) void stoi_resample_kernel(ScoreSignals a, const long long* __restrict__ target, int target0, int S,
                                                                 const float* __restrict__ G, float* __restrict__ out, int C, long long Ls,
                                                                 long long L10, const int* __restrict__ lag, int D) {
  __shared__ float tab[ST_UP * ST_T];
  for (int i = threadIdx.x; i < ST_UP * ST_T; i += ST_BLOCK) tab[i] = G[i];
  __syncthreads();
  const long long n = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
  if (n >= L10) return;
  const int sig = blockIdx.y;
  const long long rc = blockIdx.z, c = rc % C, r = rc / C;
  const float* p0;
  long long other = 0;                                                   // the second mixture channel of the mono baseline
  if (sig == 0) p0 = row(a.refs, r, score_target(target, target0, r, S), c) + D;
  else if (sig == 1) p0 = row(a.est, r, c) + D + score_lag(lag, rc, D);
  else {
    p0 = row(a.mix, r, 0) + (C == 2 ? c * a.mix.sc : 0) + D;
    other = C == 2 ? 0 : a.mix.sc;
  }
  const bool mean2 = sig == 2 && C == 1;
  const long long t = n * ST_DOWN + ST_HALF, j0 = t / ST_UP;
  const float* g = tab + (int)(t - j0 * ST_UP) * ST_T;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < ST_T; ++k) {
    const long long j = j0 - k;
    const bool ok = j >= 0 && j < Ls;
    const long long jc = ok ? j : 0;                                     // (row sample 0 always exists: Ls >= 1)
    float v = p0[jc];
    if (mean2) v = 0.5f * (v + p0[jc + other]);
    acc = fmaf(g[k], ok ? v : 0.f, acc);
  }
  out[(rc * 3 + sig) * L10 + n] = acc;
}

__global__ __launch_bounds__(ST_BLOCK) void stoi_energy_kernel(const float* __restrict__ x10, long long ld, const float* __restrict__ win,
                                                               const long long* __restrict__ ranges, double* __restrict__ energy, long long L10,
                                                               int NR, long long Ftot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long slot = (long long)blockIdx.x * (ST_BLOCK / 64) + wave, rc = blockIdx.y;
  if (slot >= Ftot) return;
  const StoiRange g = stoi_range(ranges, stoi_find(ranges, NR, slot), L10, Ftot);
  const long long f = slot - g.off;
  if (f < 0 || f >= g.nf) return;
  const float* x = x10 + rc * 3 * ld + g.start + f * ST_HOP;              // the clean signal's frame f
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float p = __fmul_rn(win[4 * lane + u], x[4 * lane + u]);
    s += (double)p * (double)p;
  }
  s = wave_sum(s);
  if (lane == 0) energy[rc * Ftot + slot] = s;
}

__global__ __launch_bounds__(ST_BLOCK) void stoi_mask_kernel(const long long* __restrict__ ranges, const double* __restrict__ energy,
                                                             int* __restrict__ list, int* __restrict__ kept, long long L10, int NR, long long Ftot) {
  __shared__ double red[ST_BLOCK / 64];
  __shared__ int cnt[ST_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const long long rc = blockIdx.y;
  const StoiRange g = stoi_range(ranges, q, L10, Ftot);
  const double* e = energy + rc * Ftot + g.off;
  int* lst = list + rc * Ftot + g.off;
  double mx = 0.0;                                                       // (a maximum does not depend on the order it is taken in)
  for (int f = tid; f < g.nf; f += ST_BLOCK) mx = fmax(mx, e[f]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const double floor_db = 20.0 * log10(sqrt(mx) + ST_EPS) - ST_RANGE_DB;
  int base = 0;
  for (int f0 = 0; f0 < g.nf; f0 += ST_BLOCK) {
    const int f = f0 + tid;
    const bool keep = f < g.nf && 20.0 * log10(sqrt(e[f]) + ST_EPS) > floor_db;
    const unsigned long long m = __ballot(keep);
    __syncthreads();                                                     // the last step's counts have been read
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    int before = base;
    for (int w = 0; w < wave; ++w) before += cnt[w];
    if (keep) lst[before + __popcll(m & ((1ull << lane) - 1ull))] = f;
    base += cnt[0] + cnt[1] + cnt[2] + cnt[3];
  }
  if (tid == 0) {
    kept[2 * (rc * NR + q)] = base;
    kept[2 * (rc * NR + q) + 1] = g.nf > 0 && !(mx > 0.0) ? 1 : 0;     // (a range without a frame is not silent: it is too short)
  }
}

__global__ __launch_bounds__(ST_ENV_THREADS) void stoi_envelope_kernel(const float* __restrict__ x10, long long ld, const float* __restrict__ win,
                                                                       const cf* __restrict__ tw, const long long* __restrict__ ranges,
                                                                       const int* __restrict__ list, const int* __restrict__ kept,
                                                                       double* __restrict__ env, long long L10, int NR, long long Ftot) {
  __shared__ cf z[3][1 << ST_LOGM];
  __shared__ double pw[3][ST_NBINS];
  const int tid = threadIdx.x;
  const long long slot = blockIdx.x, rc = blockIdx.y;
  const int q = stoi_find(ranges, NR, slot);
  const StoiRange g = stoi_range(ranges, q, L10, Ftot);
  const long long t = slot - g.off;
  bool silent;
  const int K = stoi_kept(kept, rc * NR + q, g.nf, silent);
  if (t < 0 || t >= K - 1) return;                                       // K - 1 envelope frames
  const int* lst = list + rc * Ftot + g.off;
  long long src[3];                                                      // the kept frames t - 1, t, t + 1 (t + 1 <= K - 1 exists)
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const long long k = t - 1 + u < 0 ? 0 : t - 1 + u;
    src[u] = clampll(lst[k], 0, g.nf - 1) * ST_HOP;
  }
  const float wa = win[tid], wb = win[tid + ST_HOP];
  const cf* tws = tw + (1 << ST_LOGM);                                   // the stage-ordered copy
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const float* x = x10 + (rc * 3 + s) * ld + g.start;
    // sample tid of the frame: the second half of kept frame t - 1 (none at t = 0) plus the first half of frame t; sample tid + 128: the
    // second half of frame t plus the first half of frame t + 1
    const float prev = t > 0 ? __fmul_rn(wb, x[src[0] + tid + ST_HOP]) : 0.f;
    const float lo = __fadd_rn(prev, __fmul_rn(wa, x[src[1] + tid]));
    const float hi = __fadd_rn(__fmul_rn(wb, x[src[1] + tid + ST_HOP]), __fmul_rn(wa, x[src[2] + tid]));
    float* zf = reinterpret_cast<float*>(z[s]);                          // z[m] = {v[2 m], v[2 m + 1]}: the samples in their order
    zf[tid] = __fmul_rn(wa, lo);
    zf[tid + ST_HOP] = __fmul_rn(wb, hi);
    zf[tid + 2 * ST_HOP] = 0.f;
    zf[tid + 3 * ST_HOP] = 0.f;
  }
  __syncthreads();
  for (int st = 0; st < ST_LOGM; ++st) {
#pragma unroll
    for (int s = 0; s < 3; ++s) dif_butterfly<ST_LOGM>(z[s], tws, st, tid);
    __syncthreads();
  }
  for (int i = tid; i < 3 * ST_NBINS; i += ST_ENV_THREADS) {
    const int s = i / ST_NBINS, k = ST_BIN0 + i - s * ST_NBINS;
    cf e, to;
    rfft_unpack(tw[k], z[s][bit_rev<ST_LOGM>(k)], z[s][bit_rev<ST_LOGM>((1 << ST_LOGM) - k)], e, to);
    const float re = __fadd_rn(e.x, to.x), im = __fadd_rn(e.y, to.y);
    pw[s][k - ST_BIN0] = (double)re * (double)re + (double)im * (double)im;
  }
  __syncthreads();
  if (tid < 3 * ST_BANDS) {
    const int s = tid / ST_BANDS, j = tid - s * ST_BANDS;
    double sum = 0.0;
    for (int k = st_edges[j]; k < st_edges[j + 1]; ++k) sum += pw[s][k - ST_BIN0];
    env[((rc * 3 + s) * ST_BANDS + j) * Ftot + slot] = sqrt(sum);
  }
}

namespace {

// d_m of STOI and of ESTOI for the clean block X and the processed block P, rows of 30 columns `stride` apart.
// rows: this thread's column of [4][15][64] doubles of LDS -- the rows' means and centred norms, which ESTOI's column pass reads again
// (in registers they cost 120 VGPRs next to a column's 60 and the kernel spills).  Loops over the 30 columns are kept rolled.
__device__ __forceinline__ void stoi_segment(const double* __restrict__ X, const double* __restrict__ P, long long stride, double* rows,
                                             double& d_stoi, double& d_estoi) {
  double d = 0.0;
#pragma unroll 1
  for (int j = 0; j < ST_BANDS; ++j) {
    const double* x = X + j * stride;
    const double* p = P + j * stride;
    double sx = 0.0, sp = 0.0, sxx = 0.0, spp = 0.0;
#pragma unroll 1
    for (int i = 0; i < ST_SEG; ++i) {
      const double xv = x[i], pv = p[i];
      sx += xv, sp += pv, sxx += xv * xv, spp += pv * pv;
    }
    const double alpha = sqrt(sxx) / (sqrt(spp) + ST_EPS);
    double sc = 0.0;                                                     // the clipped row's mean
#pragma unroll 1
    for (int i = 0; i < ST_SEG; ++i) sc += fmin(alpha * p[i], ST_CLIP * x[i]);
    const double mux = sx / ST_SEG, mup = sp / ST_SEG, muc = sc / ST_SEG;
    double cxx = 0.0, cpp = 0.0, ccc = 0.0;
#pragma unroll 1
    for (int i = 0; i < ST_SEG; ++i) {
      const double xv = x[i] - mux, pv = p[i] - mup, cv = fmin(alpha * p[i], ST_CLIP * x[i]) - muc;
      cxx += xv * xv, cpp += pv * pv, ccc += cv * cv;
    }
    const double dx = sqrt(cxx) + ST_EPS, dc = sqrt(ccc) + ST_EPS;
    double row = 0.0;
#pragma unroll 1
    for (int i = 0; i < ST_SEG; ++i) row += ((x[i] - mux) / dx) * ((fmin(alpha * p[i], ST_CLIP * x[i]) - muc) / dc);
    d += row;
    rows[(0 * ST_BANDS + j) * 64] = mux, rows[(1 * ST_BANDS + j) * 64] = dx;
    rows[(2 * ST_BANDS + j) * 64] = mup, rows[(3 * ST_BANDS + j) * 64] = sqrt(cpp) + ST_EPS;
  }
  d_stoi = d / ST_BANDS;
  double de = 0.0;
#pragma unroll 1
  for (int i = 0; i < ST_SEG; ++i) {
    double xr[ST_BANDS], pr[ST_BANDS];
    double sx = 0.0, sp = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
      xr[j] = (X[j * stride + i] - rows[(0 * ST_BANDS + j) * 64]) / rows[(1 * ST_BANDS + j) * 64];
      pr[j] = (P[j * stride + i] - rows[(2 * ST_BANDS + j) * 64]) / rows[(3 * ST_BANDS + j) * 64];
      sx += xr[j], sp += pr[j];
    }
    const double mux = sx / ST_BANDS, mup = sp / ST_BANDS;
    double cxx = 0.0, cpp = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
      xr[j] -= mux, pr[j] -= mup;
      cxx += xr[j] * xr[j], cpp += pr[j] * pr[j];
    }
    const double dx = sqrt(cxx) + ST_EPS, dp = sqrt(cpp) + ST_EPS;
    double col = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) col += (xr[j] / dx) * (pr[j] / dp);
    de += col;
  }
  d_estoi = de / ST_SEG;
}

}  // namespace

__global__ __launch_bounds__(64) void stoi_segments_kernel(const double* __restrict__ env, const long long* __restrict__ ranges,
                                                           const int* __restrict__ kept, double* __restrict__ dseg, long long L10, int NR,
                                                           long long Ftot) {
  __shared__ double rows[4 * ST_BANDS * 64];
  const long long slot = (long long)blockIdx.x * 64 + threadIdx.x, rc = blockIdx.y;
  if (slot >= Ftot) return;
  const int q = stoi_find(ranges, NR, slot);
  const StoiRange g = stoi_range(ranges, q, L10, Ftot);
  const long long i = slot - g.off;                                      // segment i: the envelope columns [i, i + 30), m = i + 30
  bool silent;
  const int K = stoi_kept(kept, rc * NR + q, g.nf, silent);
  if (i < 0 || i + ST_SEG > K - 1) return;
  const double* X = env + rc * 3 * ST_BANDS * Ftot + slot;
  double* out = dseg + rc * 4 * Ftot + slot;
#pragma unroll 1
  for (int s = 1; s < 3; ++s) {
    double a, b;
    stoi_segment(X, X + s * ST_BANDS * Ftot, Ftot, rows + threadIdx.x, a, b);
    out[(2 * s - 2) * Ftot] = a;
    out[(2 * s - 1) * Ftot] = b;
  }
}

__global__ __launch_bounds__(ST_BLOCK) void stoi_mean_kernel(const double* __restrict__ dseg, const long long* __restrict__ ranges,
                                                             const int* __restrict__ kept, double* __restrict__ out, long long L10, int NR,
                                                             long long Ftot) {
  __shared__ double part[4][ST_BLOCK];
  const int tid = threadIdx.x, q = blockIdx.x;
  const long long rc = blockIdx.y;
  const StoiRange g = stoi_range(ranges, q, L10, Ftot);
  bool silent;
  const int K = stoi_kept(kept, rc * NR + q, g.nf, silent);
  const int nseg = K - ST_SEG;                                           // m = 30 .. K - 1
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const double* d = dseg + (rc * 4 + v) * Ftot + g.off;
    double s = 0.0;
    for (int i = tid; i < nseg; i += ST_BLOCK) s += d[i];
    part[v][tid] = s;
  }
  __syncthreads();
  for (int h = ST_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int v = 0; v < 4; ++v) part[v][tid] += part[v][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = out + (rc * NR + q) * 6;
    const bool none = nseg < 1 || silent;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double m[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) m[v] = none ? nan : part[v][0] / (double)nseg;
    o[0] = m[0], o[1] = m[1], o[2] = m[2], o[3] = m[3], o[4] = m[0] - m[2], o[5] = m[1] - m[3];
  }
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_stoi_resample(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr,
                                 long long est_sc, const float* mix, long long mix_sr, long long mix_sc, const long long* target, int target0,
                                 const float* G, float* out, int R, int S, int C, long long L, const int* lag, int D, m2h_stream stream) {
  const char* what = "stoi_resample";
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {mix, mix_sr, mix_sc}};
  if (int rc = check_signals(what, a, true, out, R, S, C, L, D, 0, 1, 65535 / 2)) return rc;
  M2H_REQUIRE(G, "%s: null pointer (G)", what);
  if (int rc = check_lag(what, lag, D)) return rc;
  if (int rc = check_target(what, target, target0, S)) return rc;
  M2H_REQUIRE((reinterpret_cast<size_t>(out) & 3) == 0, "%s: out must be 4-byte aligned", what);
  const long long Ls = L - 2ll * D, L10 = (Ls * ST_UP + ST_DOWN - 1) / ST_DOWN;
  long long J;
  if (int rc = check_tiles(what, L10, ST_BLOCK, 1, J)) return rc;
  M2H_LAUNCH(stoi_resample_kernel, dim3((unsigned)J, 3, (unsigned)(R * C)), dim3(ST_BLOCK), 0, as_stream(stream), a, target, target0, S, G, out, C, Ls,
             L10, lag, D);
  return launch_status(what);
}

extern "C" int m2h_stoi_ranges(const float* x10, long long ld, long long L10, const float* window, const float* twiddles, const long long* ranges,
                               int NR, long long Ftot, int RC, double* energy, int* list, int* kept, double* env, double* dseg, double* out,
                               m2h_stream stream) {
  const char* what = "stoi_ranges";
  M2H_REQUIRE(x10 && window && twiddles && ranges && energy && list && kept && env && dseg && out,
              "%s: null pointer (x10 %p, window %p, twiddles %p, ranges %p, energy %p, list %p, kept %p, env %p, dseg %p, out %p)", what, (const void*)x10,
              (const void*)window, (const void*)twiddles, (const void*)ranges, (void*)energy, (void*)list, (void*)kept, (void*)env, (void*)dseg, (void*)out);
  M2H_REQUIRE(RC >= 1 && RC <= 65535, "%s: RC = %d rows of three signals; 1 .. 65535 are supported", what, RC);
  M2H_REQUIRE(NR >= 1 && NR <= 0x7fffffff / 3, "%s: NR = %d ranges; at least 1 is required", what, NR);
  M2H_REQUIRE(L10 >= 1 && ld >= L10, "%s: L10 = %lld samples in rows %lld apart; 1 <= L10 <= ld is required", what, L10, ld);
  M2H_REQUIRE(Ftot >= 1 && Ftot <= 0x7fffffffLL, "%s: Ftot = %lld frame slots; 1 .. 2^31 - 1 are supported (more exceed a grid of 2^31 - 1 workgroups)", what,
              Ftot);
  M2H_REQUIRE(((reinterpret_cast<size_t>(energy) | reinterpret_cast<size_t>(env) | reinterpret_cast<size_t>(dseg) | reinterpret_cast<size_t>(out) |
                reinterpret_cast<size_t>(ranges)) & 7) == 0,
              "%s: energy, env, dseg, out and ranges must be 8-byte aligned", what);
  M2H_REQUIRE(((reinterpret_cast<size_t>(x10) | reinterpret_cast<size_t>(window) | reinterpret_cast<size_t>(list) | reinterpret_cast<size_t>(kept)) & 3) == 0 &&
                  (reinterpret_cast<size_t>(twiddles) & 7) == 0,
              "%s: x10, window, list and kept must be 4-byte aligned, twiddles 8-byte aligned", what);
  hipStream_t s = as_stream(stream);
  const cf* tw = reinterpret_cast<const cf*>(twiddles);
  M2H_LAUNCH(stoi_energy_kernel, dim3((unsigned)((Ftot + 3) / 4), (unsigned)RC), dim3(ST_BLOCK), 0, s, x10, ld, window, ranges, energy, L10, NR, Ftot);
  M2H_LAUNCH(stoi_mask_kernel, dim3((unsigned)NR, (unsigned)RC), dim3(ST_BLOCK), 0, s, ranges, energy, list, kept, L10, NR, Ftot);
  M2H_LAUNCH(stoi_envelope_kernel, dim3((unsigned)Ftot, (unsigned)RC), dim3(ST_ENV_THREADS), 0, s, x10, ld, window, tw, ranges, list, kept, env, L10, NR,
             Ftot);
  M2H_LAUNCH(stoi_segments_kernel, dim3((unsigned)((Ftot + 63) / 64), (unsigned)RC), dim3(64), 0, s, env, ranges, kept, dseg, L10, NR, Ftot);
  M2H_LAUNCH(stoi_mean_kernel, dim3((unsigned)NR, (unsigned)RC), dim3(ST_BLOCK), 0, s, dseg, ranges, kept, out, L10, NR, Ftot);
  return launch_status(what);
}
