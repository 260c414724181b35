// In-LDS radix-2 complex transforms, the packed-real-transform pair algebra and what stands around them (the packed load, the
// bit-reversed slot of a bin, the walk over a thread's pairs, the LDS reservation), shared by three units:
//   fftconv.hip  the feeder's one-second convolution: bit_rev, load_packed, reserve_transform_lds; the any-block-size fft_dif / ifft_dit on
//                the natural-order table and a strided pair loop of its own (at LOGM = 10 a block has more threads than pairs)
//   render.hip   the partitioned renderer: the unrolled transforms; render_spectra_kernel all of the helpers, render_frames_kernel
//                bit_rev under its own grouped product loop
//   align.hip    the Scorer's cross-correlation: the unrolled transforms and all of the helpers, twice each
//
// A real N-point transform is one complex M = N/2-point transform of z[m] = x[2m] + i x[2m+1] plus an O(N) unpack; the pair
// (k, M-k) is all that the unpack, a spectrum product and the re-pack for the inverse need:
//   forward : decimation in frequency, natural order in -> bit-reversed order out (no reordering pass);
//   inverse : the same butterfly network run backwards with conjugate twiddles: bit-reversed in -> natural order out.
// Twiddles tw[k] = exp(-2 pi i k / (2M)), k < M, come from a table built on the host in float64.  Arithmetic fp32 throughout.
#pragma once
#include "m2h_internal.h"

namespace m2h {

namespace {
struct cf {
  float x, y;
};
__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cf cmulc(cf a, cf b) { return {a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }   // a * conj(b)
__device__ __forceinline__ cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cf conj(cf a) { return {a.x, -a.y}; }

// Unpack of the pair (k, M-k) of a packed transform Z, t = tw[k]:  E = (Zk + conj Zm)/2, T O = T * (-i/2)(Zk - conj Zm);
// the real signal's spectrum is S[k] = E + T O, S[M-k] = conj(E - T O).
__device__ __forceinline__ void rfft_unpack(cf t, cf zk, cf zm, cf& e, cf& to) {
  e = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
  const cf d = {0.5f * (zk.x - zm.x), 0.5f * (zk.y + zm.y)};   // (Zk - conj Zm)/2
  to = cmul(t, cf{d.y, -d.x});                                   // * (-i)
}

// Re-pack of Y[k] and conj(Y[M-k]) for the inverse packed transform: Z'[k] = E' + i O', Z'[M-k] = conj(E') + i conj(O').
__device__ __forceinline__ void rfft_repack(cf t, cf yk, cf ymc, cf& zk, cf& zm) {
  const cf e2 = {0.5f * (yk.x + ymc.x), 0.5f * (yk.y + ymc.y)};    // E' = (Y[k] + conj Y[M-k]) / 2
  const cf w2 = {0.5f * (yk.x - ymc.x), 0.5f * (yk.y - ymc.y)};
  const cf o2 = cmulc(w2, t);                                      // O' = conj(T) (Y[k] - conj Y[M-k]) / 2
  zk = {e2.x - o2.y, e2.y + o2.x};
  zm = {e2.x + o2.y, -e2.y + o2.x};
}

// Slot 0 of a packed transform holds the two real bins: S[0] = Z0.x + Z0.y, S[M] = Z0.x - Z0.y; and back.
__device__ __forceinline__ cf rfft_repack_dc(float y0, float ym) { return {0.5f * (y0 + ym), 0.5f * (y0 - ym)}; }

// The forward transform leaves bin k of M = 2^LOGM in slot bit_rev(k), and the inverse reads it there.
template <int LOGM>
__device__ __forceinline__ int bit_rev(int k) { return (int)(__brev((unsigned)k) >> (32 - LOGM)); }

// z[m] = {src[2m], src[2m+1]} at element stride es, zero from sample n on; a block of NT threads.
template <int LOGM, int NT>
__device__ __forceinline__ void load_packed(cf* z, const float* __restrict__ src, int n, int es = 1) {
  for (int m = threadIdx.x; m < 1 << LOGM; m += NT)
    z[m] = {2 * m < n ? src[(size_t)(2 * m) * es] : 0.f, 2 * m + 1 < n ? src[(size_t)(2 * m + 1) * es] : 0.f};
}

// The pairs (k, M-k) a thread of a block of NT owns: k = tid + NT i < M/2, unrolled -- dc(i) for k = 0 (slot 0 and its two real bins),
// pair(i, k) for every other k -- and on thread 0 half() for k = M/2, its own partner.
template <int LOGM, int NT, class DC, class Pair, class Half>
__device__ __forceinline__ void rfft_own_pairs(DC dc, Pair pair, Half half) {
  static_assert((1 << LOGM) / 2 % NT == 0, "whole pairs per thread");
#pragma unroll
  for (int i = 0; i < (1 << LOGM) / 2 / NT; ++i) {
    const int k = (int)threadIdx.x + NT * i;
    if (k == 0) dc(i);
    else pair(i, k);
  }
  if (threadIdx.x == 0) half();
}

// Host: a kernel that holds the whole transform in dynamic LDS (128 KB at LOGM = 14) has to be given leave for more than 64 KB.
template <int LOGM, class K>
int reserve_transform_lds(K* kernel, const char* what) {
  const size_t lds = sizeof(cf) << LOGM;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail((int)e, "%s: cannot reserve %zu bytes of LDS: %s", what, lds, hipGetErrorString(e));
  return 0;
}
}  // namespace

// z: M complex values in LDS.  tw[k] = exp(-2 pi i k / (2M)), k < M.
// Butterfly j of stage s (half = M >> (s + 1)), as written out in the loops of fft_dif / ifft_dit below, with its twiddle read from
// the STAGE-ORDERED copy of the table: tws[M - (M >> s) + pos] = tw[(pos << s) * 2], pos < half -- the same values, each stage's
// contiguous.  (In tw itself the twiddles of consecutive butterflies of stage s lie 16 << s bytes apart: from the fifth stage on every
// lane of a wave reads another cache line, and the transform is bound by the L1's lines per clock.)
template <int LOGM>
__device__ __forceinline__ void dif_butterfly(cf* z, const cf* __restrict__ tws, int s, int j) {
  const int half = (1 << LOGM) >> (s + 1);
  const int g = j >> (LOGM - 1 - s), pos = j & (half - 1);       // j / half and j % half as a shift and a mask: half is a power of two
  const int i0 = g * 2 * half + pos, i1 = i0 + half;
  const cf a = z[i0], b = z[i1];
  z[i0] = cadd(a, b);
  z[i1] = cmul(csub(a, b), tws[(1 << LOGM) - ((1 << LOGM) >> s) + pos]);
}

template <int LOGM>
__device__ __forceinline__ void dit_butterfly(cf* z, const cf* __restrict__ tws, int s, int j) {
  const int half = (1 << LOGM) >> (s + 1);
  const int g = j >> (LOGM - 1 - s), pos = j & (half - 1);       // j / half and j % half as a shift and a mask: half is a power of two
  const int i0 = g * 2 * half + pos, i1 = i0 + half;
  const cf a = z[i0], b = cmulc(z[i1], tws[(1 << LOGM) - ((1 << LOGM) >> s) + pos]);
  z[i0] = cadd(a, b);
  z[i1] = csub(a, b);
}

// Any block size: the butterflies of a stage walked at stride blockDim.x (the loops as the feeder's kernel has always had them).
template <int LOGM>
__device__ __forceinline__ void fft_dif(cf* z, const cf* __restrict__ tw) {
  constexpr int M = 1 << LOGM;
  for (int s = 0; s < LOGM; ++s) {
    const int half = M >> (s + 1);
    for (int j = threadIdx.x; j < M / 2; j += blockDim.x) {
      const int g = j / half, pos = j - g * half;
      const int i0 = g * 2 * half + pos, i1 = i0 + half;
      const cf a = z[i0], b = z[i1];
      z[i0] = cadd(a, b);
      z[i1] = cmul(csub(a, b), tw[(pos << s) * 2]);
    }
    __syncthreads();
  }
}

template <int LOGM>
__device__ __forceinline__ void ifft_dit(cf* z, const cf* __restrict__ tw) {
  constexpr int M = 1 << LOGM;
  for (int s = LOGM - 1; s >= 0; --s) {
    const int half = M >> (s + 1);
    for (int j = threadIdx.x; j < M / 2; j += blockDim.x) {
      const int g = j / half, pos = j - g * half;
      const int i0 = g * 2 * half + pos, i1 = i0 + half;
      const cf a = z[i0], b = cmulc(z[i1], tw[(pos << s) * 2]);
      z[i0] = cadd(a, b);
      z[i1] = csub(a, b);
    }
    __syncthreads();
  }
}

// The same transforms for a block of exactly NT threads: the walk's trip count is a constant and the loop is unrolled, so a thread's
// M / (2 NT) LDS reads and twiddle loads of a stage are in flight together instead of one after the other.  The butterflies, their
// operands and every element's order of operations are those of the forms above; tws is the stage-ordered table.
template <int LOGM, int NT>
__device__ __forceinline__ void fft_dif_fixed(cf* z, const cf* __restrict__ tws) {
  constexpr int M = 1 << LOGM;
  static_assert(M / 2 % NT == 0, "whole butterflies per thread");
  for (int s = 0; s < LOGM; ++s) {
#pragma unroll
    for (int i = 0; i < M / 2 / NT; ++i) dif_butterfly<LOGM>(z, tws, s, (int)threadIdx.x + i * NT);
    __syncthreads();
  }
}

template <int LOGM, int NT>
__device__ __forceinline__ void ifft_dit_fixed(cf* z, const cf* __restrict__ tws) {
  constexpr int M = 1 << LOGM;
  static_assert(M / 2 % NT == 0, "whole butterflies per thread");
  for (int s = LOGM - 1; s >= 0; --s) {
#pragma unroll
    for (int i = 0; i < M / 2 / NT; ++i) dit_butterfly<LOGM>(z, tws, s, (int)threadIdx.x + i * NT);
    __syncthreads();
  }
}

}  // namespace m2h
