// Scorer, time alignment (m2h/audio/score.py holds the definition): the cross-correlation of the target and the estimate of one
// (recording, channel, tile) at every lag d in -D .. D, by one 32 768-point circular correlation in LDS.
//
//   region   : the reference samples [D, L - D), Lr = L - 2 D of them, cut into tiles of `tile` samples, J = ceil(Lr / tile)
//   s segment: s[D + j tile + t],        t < n = min(tile, Lr - j tile), zero-padded
//   x segment: x[j tile + q],            q < n + 2 D <= 32 768 (it ends at or before L)
//   ct[r][c][j][d + D] = sum_t s[D + j tile + t] x[D + j tile + t + d] = sum_t sseg[t] xseg[t + (d + D)] = IFFT(conj(S) X)[d + D]
//
// t + (d + D) < n + 2 D <= 32 768: no wrap-around reaches the outputs 0 .. 2 D.
//
// One 1024-thread workgroup per (tile, channel, recording) on the packed 16 384-point complex transform of fft_lds.h in 128 KB of LDS,
// as render.hip runs it.  Two real spectra do not fit into the CU's 160 KB together, so the s segment is transformed first and the
// thread's 8 pairs (k, M-k) of its spectrum are unpacked into registers (16 complex values; thread 0 also holds k = M/2); the x segment
// is then loaded into the same LDS and transformed, and conj(S) X is formed pair by pair and re-packed IN PLACE: the slots br(k) and
// br(M-k) of a pair are read and written by the one thread that owns the pair, so no barrier stands between the unpack and the re-pack.
// Inverse transform, scale by 1 / M, the first 2 D + 1 outputs stored as doubles.  No atomics: the same bits on every run.  Samples are
// loaded one 4-byte word at a time, so the alignment of a row plays no role.
#include "fft_lds.h"
#include "score_common.h"

namespace m2h {

namespace {
constexpr int ALOGM = 14;              // packed transform: 2^14 complex points = 32 768 real points
constexpr int AM = 1 << ALOGM;
constexpr int ANFFT = 2 * AM;
constexpr int APAIRS = AM / 2 / 1024;  // pairs (k, M-k) per thread
}  // namespace

// grid (J, C, R).  target: [R] reference indices on the device (clamped to [0, S)), or null: target0 for every recording.  a.mix is not read.
__global__ __launch_bounds__(1024) void align_corr_kernel(ScoreSignals a, const long long* __restrict__ target, int target0, int S,
                                                          const cf* __restrict__ tw, double* __restrict__ out, long long L, int tile, int D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  const int tid = threadIdx.x;
  const long long j = blockIdx.x, c = blockIdx.y, r = blockIdx.z;
  const long long Lr = L - 2ll * D;
  const long long left = Lr - j * tile;                    // >= 1: J = ceil(Lr / tile)
  const int n = left < tile ? (int)left : tile;
  const float* s = row(a.refs, r, score_target(target, target0, r, S), c) + D + j * tile;
  const float* x = row(a.est, r, c) + j * tile;             // the x segment [j tile, j tile + n + 2 D) ends at or before L

  load_packed<ALOGM, 1024>(z, s, n);
  __syncthreads();
  fft_dif_fixed<ALOGM, 1024>(z, tw + AM);                  // (the table's second half: the same twiddles in stage order)
  cf sk[APAIRS], smc[APAIRS];                              // S[k], conj(S[M-k]); k = 0: {S[0], S[M]}, both real
  cf sh = {0.f, 0.f};                                      // S[M/2] (thread 0)
  auto spectrum = [&](int k, cf& yk, cf& ymc) {            // -> Y[k], conj(Y[M-k]) of the real signal whose packed transform z holds now
    cf e, to;
    rfft_unpack(tw[k], z[bit_rev<ALOGM>(k)], z[bit_rev<ALOGM>(AM - k)], e, to);
    yk = cadd(e, to);
    ymc = csub(e, to);
  };
  rfft_own_pairs<ALOGM, 1024>(
      [&](int i) {
        const cf z0 = z[0];
        sk[i] = {z0.x + z0.y, z0.x - z0.y};
        smc[i] = {0.f, 0.f};
      },
      [&](int i, int k) { spectrum(k, sk[i], smc[i]); },
      [&] {
        cf ignored;
        spectrum(AM / 2, sh, ignored);
      });
  __syncthreads();                                         // every thread has read its pairs of S

  load_packed<ALOGM, 1024>(z, x, n + 2 * D);
  __syncthreads();
  fft_dif_fixed<ALOGM, 1024>(z, tw + AM);
  rfft_own_pairs<ALOGM, 1024>(
      [&](int i) {
        const cf z0 = z[0];
        z[0] = rfft_repack_dc(sk[i].x * (z0.x + z0.y), sk[i].y * (z0.x - z0.y));      // S[0] X[0], S[M] X[M]: real
      },
      [&](int i, int k) {
        cf xk, xmc, zk, zm;                                // X[k], conj(X[M-k])
        spectrum(k, xk, xmc);
        // Y[k] = conj(S[k]) X[k];  conj(Y[M-k]) = S[M-k] conj(X[M-k]) = conj(smc) xmc
        rfft_repack(tw[k], cmulc(xk, sk[i]), cmulc(xmc, smc[i]), zk, zm);
        z[bit_rev<ALOGM>(k)] = zk;
        z[bit_rev<ALOGM>(AM - k)] = zm;
      },
      [&] {
        cf xh, ignored, zk, zm;
        spectrum(AM / 2, xh, ignored);
        const cf yh = cmulc(xh, sh);
        rfft_repack(tw[AM / 2], yh, conj(yh), zk, zm);
        z[bit_rev<ALOGM>(AM / 2)] = zk;
      });
  __syncthreads();
  ifft_dit_fixed<ALOGM, 1024>(z, tw + AM);
  const int K = 2 * D + 1;
  double* o = out + (((size_t)r * gridDim.y + c) * gridDim.x + j) * K;
  const float sc = 1.f / (float)AM;
  for (int m = tid; m <= D; m += 1024) {                   // outputs 2m and 2m + 1 <= 2 D
    const cf v = z[m];
    o[2 * m] = (double)(v.x * sc);
    if (2 * m + 1 < K) o[2 * m + 1] = (double)(v.y * sc);
  }
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_align_corr(const float* refs, long long refs_sr, long long refs_ss, long long refs_sc, const float* est, long long est_sr,
                              long long est_sc, const long long* target, int target0, const float* twiddles, double* out, int R, int S, int C,
                              long long L, int tile, int D, m2h_stream stream) {
  const ScoreSignals a{{refs, refs_sr, refs_ss, refs_sc}, {est, est_sr, est_sc}, {nullptr, 0, 0}};
  long long J;
  if (int rc = check_signals("align_corr", a, false, out, R, S, C, L, D, 1, 2, 65535)) return rc;   // (R is the grid's z)
  M2H_REQUIRE(twiddles, "align_corr: null pointer (twiddles)");
  M2H_REQUIRE((long long)tile + 2ll * D <= ANFFT, "align_corr: tile + 2 D = %d + 2 * %d exceeds the transform's %d points", tile, D, ANFFT);
  if (int rc = check_target("align_corr", target, target0, S)) return rc;
  M2H_REQUIRE((reinterpret_cast<size_t>(twiddles) & 7) == 0 && (reinterpret_cast<size_t>(out) & 7) == 0, "align_corr: twiddles and out must be 8-byte aligned");
  if (int rc = check_tiles("align_corr", L - 2ll * D, tile, 1, J)) return rc;           // (J alone is the grid's x)
  if (int rc = reserve_transform_lds<ALOGM>(align_corr_kernel, "align_corr")) return rc;
  M2H_LAUNCH(align_corr_kernel, dim3((unsigned)J, C, R), dim3(1024), sizeof(cf) << ALOGM, as_stream(stream), a, target, target0, S,
             reinterpret_cast<const cf*>(twiddles), out, L, tile, D);
  return launch_status("align_corr");
}
