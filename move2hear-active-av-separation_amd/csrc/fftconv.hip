// RIR convolution of the audio feeder (gfx950): scipy.signal.fftconvolve(mono, rir[:, ear]) for both ears of one (clip, source)
// pair per workgroup (pretrain/datasets/dataset.py:180, habitat_audio/simulator_train.py:419), as hand-written FFTs in LDS.
//
// The linear convolution needs N >= L + Lr - 1 points (32 768 for one-second clips and RIRs).  A real N-point transform is one
// complex M = N/2-point transform of z[m] = x[2m] + i x[2m+1] plus an O(N) unpack; M = 16 384 complex fp32 values are 128 KB,
// so the whole transform lives in the CU's 160 KB of LDS: 1024 threads, radix-2, 14 stages, one barrier per stage.
//   forward : decimation in frequency, natural order in -> bit-reversed order out (no reordering pass);
//   spectrum: the pair (k, M-k) is all that the unpack of X, H, the product Y = X H and the re-pack for the inverse need, so
//             each thread turns Z_h[k], Z_h[M-k] (LDS) and Z_x[k], Z_x[M-k] (global scratch, written once per source) into
//             Z'[k], Z'[M-k] in place -- still in bit-reversed slots;
//   inverse : the same butterfly network run backwards with conjugate twiddles: bit-reversed in -> natural order out.
// Twiddles exp(-2 pi i k / N) come from a table built on the host in float64 (setup data, like the DFT matrices of the STFT).
// Arithmetic fp32 throughout, like the library transform it replaces (rocFFT through torch.fft in round 1).
#include "m2h_internal.h"
#include "fft_lds.h"   // cf, fft_dif / ifft_dit, the pair-wise unpack and re-pack, the packed load, bit_rev, the LDS reservation

namespace m2h {

template <int LOGM>
__global__ __launch_bounds__(1024) void fftconv_kernel(const float* __restrict__ mono, const float* __restrict__ rirs, const cf* __restrict__ tw,
                                                       cf* __restrict__ xspec, float* __restrict__ full, int L, int Lr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  constexpr int M = 1 << LOGM, N = 2 * M;
  const int cs = blockIdx.x, tid = threadIdx.x;
  const int ear0 = blockIdx.y;   // one workgroup per (clip, source, ear): 2 x CS workgroups fill the chip at the feeder's batch (64 x 2
                                 // sources); each redoes the clip's own transform (3 transforms per workgroup instead of 5 in one)

  // ---- spectrum of the mono clip (packed, bit-reversed), kept in global scratch for the two ears ----
  load_packed<LOGM, 1024>(z, mono + (size_t)cs * L, L);
  __syncthreads();
  fft_dif<LOGM>(z, tw);
  cf* zx = xspec + ((size_t)cs * 2 + ear0) * M;
  for (int m = tid; m < M; m += 1024) zx[m] = z[m];
  __threadfence();   // the block reads zx back below (other threads' elements): stores drained to L2 before the barrier
  __syncthreads();

  for (int ear = ear0; ear <= ear0; ++ear) {
    load_packed<LOGM, 1024>(z, rirs + (size_t)cs * Lr * 2 + ear, Lr, 2);
    __syncthreads();
    fft_dif<LOGM>(z, tw);
    // ---- per pair (k, M-k): unpack X and H, multiply, re-pack for the inverse; in place, bit-reversed slots ----
    for (int k = tid; k <= M / 2; k += 1024) {
      if (k == 0) {
        const cf zh = z[0], zxx = zx[0];
        const float y0 = (zxx.x + zxx.y) * (zh.x + zh.y), ym = (zxx.x - zxx.y) * (zh.x - zh.y);   // X[0] H[0], X[M] H[M] (all real)
        z[0] = rfft_repack_dc(y0, ym);
        continue;
      }
      const int ik = bit_rev<LOGM>(k), im = bit_rev<LOGM>(M - k);
      const cf t = tw[k];
      const cf zhk = z[ik], zhm = z[im], zxk = zx[ik], zxm = zx[im];
      cf ex, ox, eh, oh, zk, zm;
      rfft_unpack(t, zxk, zxm, ex, ox);
      rfft_unpack(t, zhk, zhm, eh, oh);
      const cf yk = cmul(cadd(ex, ox), cadd(eh, oh));                  // Y[k]
      const cf ymc = cmul(csub(ex, ox), csub(eh, oh));                 // conj(Y[M-k])
      rfft_repack(t, yk, ymc, zk, zm);
      z[ik] = zk;
      if (im != ik) z[im] = zm;
    }
    __syncthreads();
    ifft_dit<LOGM>(z, tw);
    float* out = full + ((size_t)cs * 2 + ear) * N;
    const float sc = 1.f / (float)M;
    for (int m = tid; m < M; m += 1024) {
      const cf v = z[m];
      *reinterpret_cast<float2*>(out + 2 * m) = make_float2(v.x * sc, v.y * sc);
    }
    __syncthreads();
  }
}

template <int LOGM>
static int launch_fftconv(const float* mono, const float* rirs, const float* tw, float* xspec, float* full, int CS, int L, int Lr, hipStream_t st) {
  const size_t lds = sizeof(cf) << LOGM;
  auto kern = fftconv_kernel<LOGM>;
  if (lds > 64 * 1024)
    if (int rc = reserve_transform_lds<LOGM>(kern, "fftconv_same")) return rc;
  M2H_LAUNCH(kern, dim3(CS, 2), dim3(1024), lds, st, mono, rirs, reinterpret_cast<const cf*>(tw), reinterpret_cast<cf*>(xspec), full, L, Lr);
  return launch_status("fftconv_same");
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_fftconv_full(const float* mono, const float* rirs, const float* twiddles, float* xspec, float* full, int CS, int L, int Lr,
                                int log2n, m2h_stream stream) {
  M2H_REQUIRE(mono && rirs && twiddles && xspec && full && CS > 0 && L > 0 && Lr > 0, "fftconv_full: bad arguments");
  M2H_REQUIRE(log2n >= 11 && log2n <= 15, "fftconv_full: transform length 2^%d outside 2^11 .. 2^15 (the packed transform must fit 128 KB of LDS)", log2n);
  M2H_REQUIRE((long)L + Lr - 1 <= (1L << log2n), "fftconv_full: 2^%d points cannot hold a %d + %d - 1 point linear convolution", log2n, L, Lr);
  hipStream_t st = as_stream(stream);
  switch (log2n) {
    case 11: return launch_fftconv<10>(mono, rirs, twiddles, xspec, full, CS, L, Lr, st);
    case 12: return launch_fftconv<11>(mono, rirs, twiddles, xspec, full, CS, L, Lr, st);
    case 13: return launch_fftconv<12>(mono, rirs, twiddles, xspec, full, CS, L, Lr, st);
    case 14: return launch_fftconv<13>(mono, rirs, twiddles, xspec, full, CS, L, Lr, st);
    default: return launch_fftconv<14>(mono, rirs, twiddles, xspec, full, CS, L, Lr, st);
  }
}
