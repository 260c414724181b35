// In-LDS radix-2 complex transforms and the packed-real-transform pair algebra, shared by the feeder's one-second convolution
// (fftconv.hip) and the partitioned renderer (render.hip).
//
// A real N-point transform is one complex M = N/2-point transform of z[m] = x[2m] + i x[2m+1] plus an O(N) unpack; the pair
// (k, M-k) is all that the unpack, a spectrum product and the re-pack for the inverse need:
//   forward : decimation in frequency, natural order in -> bit-reversed order out (no reordering pass);
//   inverse : the same butterfly network run backwards with conjugate twiddles: bit-reversed in -> natural order out.
// Twiddles tw[k] = exp(-2 pi i k / (2M)), k < M, come from a table built on the host in float64.  Arithmetic fp32 throughout.
#pragma once
#include <hip/hip_runtime.h>

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
