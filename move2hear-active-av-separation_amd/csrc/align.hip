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
#include "m2h_internal.h"
#include "fft_lds.h"

namespace m2h {

namespace {
constexpr int ALOGM = 14;              // packed transform: 2^14 complex points = 32 768 real points
constexpr int AM = 1 << ALOGM;
constexpr int ANFFT = 2 * AM;
constexpr int AMAXD = 8192;
constexpr int APAIRS = AM / 2 / 1024;  // pairs (k, M-k) per thread

__device__ __forceinline__ int abr14(int k) { return (int)(__brev((unsigned)k) >> (32 - ALOGM)); }

// z[m] = {src[2m], src[2m+1]}, zero from sample n on
__device__ __forceinline__ void load_segment(cf* z, const float* __restrict__ src, int n) {
  for (int m = threadIdx.x; m < AM; m += 1024) z[m] = {2 * m < n ? src[2 * m] : 0.f, 2 * m + 1 < n ? src[2 * m + 1] : 0.f};
}
}  // namespace

// grid (J, C, R).  target: [R] reference indices on the device (clamped to [0, S): device data never becomes an address out of bounds),
// or null: target0 for every recording.
__global__ __launch_bounds__(1024) void align_corr_kernel(const float* __restrict__ refs, long long refs_sr, long long refs_ss, long long refs_sc,
                                                          const float* __restrict__ est, long long est_sr, long long est_sc,
                                                          const long long* __restrict__ target, int target0, int S, const cf* __restrict__ tw,
                                                          double* __restrict__ out, long long L, int tile, int D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  const int tid = threadIdx.x;
  const long long j = blockIdx.x, c = blockIdx.y, r = blockIdx.z;
  const long long Lr = L - 2ll * D;
  const long long left = Lr - j * tile;                    // >= 1: J = ceil(Lr / tile)
  const int n = left < tile ? (int)left : tile;
  long long t = target ? target[r] : (long long)target0;
  t = t < 0 ? 0 : (t > S - 1 ? S - 1 : t);
  const float* s = refs + r * refs_sr + t * refs_ss + c * refs_sc + D + j * tile;
  const float* x = est + r * est_sr + c * est_sc + j * tile;            // the x segment [j tile, j tile + n + 2 D) ends at or before L

  load_segment(z, s, n);
  __syncthreads();
  fft_dif_fixed<ALOGM, 1024>(z, tw + AM);                  // (the table's second half: the same twiddles in stage order)
  cf sk[APAIRS], smc[APAIRS];                              // S[k], conj(S[M-k]); k = 0: {S[0], S[M]}, both real
#pragma unroll
  for (int i = 0; i < APAIRS; ++i) {
    const int k = tid + 1024 * i;
    if (k == 0) {
      const cf z0 = z[0];
      sk[i] = {z0.x + z0.y, z0.x - z0.y};
      smc[i] = {0.f, 0.f};
    } else {
      cf e, to;
      rfft_unpack(tw[k], z[abr14(k)], z[abr14(AM - k)], e, to);
      sk[i] = cadd(e, to);
      smc[i] = csub(e, to);
    }
  }
  cf sh = {0.f, 0.f};                                      // S[M/2] (thread 0)
  if (tid == 0) {
    cf e, to;
    const cf zh = z[abr14(AM / 2)];
    rfft_unpack(tw[AM / 2], zh, zh, e, to);
    sh = cadd(e, to);
  }
  __syncthreads();                                         // every thread has read its pairs of S

  load_segment(z, x, n + 2 * D);
  __syncthreads();
  fft_dif_fixed<ALOGM, 1024>(z, tw + AM);
#pragma unroll
  for (int i = 0; i < APAIRS; ++i) {
    const int k = tid + 1024 * i;
    if (k == 0) {
      const cf z0 = z[0];
      z[0] = rfft_repack_dc(sk[i].x * (z0.x + z0.y), sk[i].y * (z0.x - z0.y));      // S[0] X[0], S[M] X[M]: real
    } else {
      const int bk = abr14(k), bm = abr14(AM - k);
      cf e, to, zk, zm;
      rfft_unpack(tw[k], z[bk], z[bm], e, to);
      const cf xk = cadd(e, to), xmc = csub(e, to);        // X[k], conj(X[M-k])
      // Y[k] = conj(S[k]) X[k];  conj(Y[M-k]) = S[M-k] conj(X[M-k]) = conj(smc) xmc
      rfft_repack(tw[k], cmulc(xk, sk[i]), cmulc(xmc, smc[i]), zk, zm);
      z[bk] = zk;
      z[bm] = zm;
    }
  }
  if (tid == 0) {
    const int bh = abr14(AM / 2);
    cf e, to, zk, zm;
    const cf zh = z[bh];
    rfft_unpack(tw[AM / 2], zh, zh, e, to);
    const cf yh = cmulc(cadd(e, to), sh);
    rfft_repack(tw[AM / 2], yh, conj(yh), zk, zm);
    z[bh] = zk;
  }
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
  M2H_REQUIRE(refs && est && twiddles && out, "align_corr: null pointer (refs %p, est %p, twiddles %p, out %p)", (const void*)refs, (const void*)est,
              (const void*)twiddles, (void*)out);
  M2H_REQUIRE(S >= 1 && S <= 6, "align_corr: S = %d reference sources; 1 .. 6 are supported", S);
  M2H_REQUIRE(C == 1 || C == 2, "align_corr: C = %d channels; 1 or 2 are supported", C);
  M2H_REQUIRE(R >= 1 && R <= 65535, "align_corr: R = %d recordings; 1 .. 65535 are supported", R);
  M2H_REQUIRE(D >= 1 && D <= AMAXD, "align_corr: D = %d samples; 1 .. %d are supported", D, AMAXD);
  M2H_REQUIRE(tile >= 1, "align_corr: tile = %d samples; at least 1 is required", tile);
  M2H_REQUIRE((long long)tile + 2ll * D <= ANFFT, "align_corr: tile + 2 D = %d + 2 * %d exceeds the transform's %d points", tile, D, ANFFT);
  M2H_REQUIRE(L >= 2ll * D + 2, "align_corr: L = %lld samples; at least 2 D + 2 = %lld are required", L, 2ll * D + 2);
  M2H_REQUIRE(target || (target0 >= 0 && target0 < S), "align_corr: target = %d is not one of the S = %d references", target0, S);
  M2H_REQUIRE((reinterpret_cast<size_t>(twiddles) & 7) == 0 && (reinterpret_cast<size_t>(out) & 7) == 0, "align_corr: twiddles and out must be 8-byte aligned");
  const long long J = (L - 2ll * D + tile - 1) / tile;
  M2H_REQUIRE(J <= 0x7fffffffLL, "align_corr: ceil((L - 2 D) / tile) = %lld workgroups exceed a grid of 2^31 - 1", J);
  const size_t lds = sizeof(cf) << ALOGM;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(align_corr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail((int)e, "align_corr: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
  M2H_LAUNCH(align_corr_kernel, dim3((unsigned)J, C, R), dim3(1024), lds, as_stream(stream), refs, refs_sr, refs_ss, refs_sc, est, est_sr, est_sc, target,
             target0, S, reinterpret_cast<const cf*>(twiddles), out, L, tile, D);
  return launch_status("align_corr");
}
