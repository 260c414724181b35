// What the Scorer's launches share (score.hip, align.hip, score_spectral.hip, score_spatial.hip, score_itd.hip): the description of the signals, the two rules that keep
// device data from becoming an address out of bounds, and the argument checks of the entry points.
#pragma once
#include "m2h_internal.h"

namespace m2h {

constexpr int SCORE_MAXD = 8192;       // the largest lag of the alignment, in samples

// refs [R][S][C][L], est [R][C][L], mix [R][2][L] (a null pointer for a launch that reads no mixture): strides in elements, the last one 1.
// Field for field the ten arguments of the C ABI, in their order.
struct ScoreRefs { const float* p; long long sr, ss, sc; };
struct ScoreRows { const float* p; long long sr, sc; };
struct ScoreSignals { ScoreRefs refs; ScoreRows est, mix; };

namespace {
// The row of (recording r, source s, channel c).  A helper takes the tensor it reads and takes it by value: handed the whole description,
// or a reference to any of it, the kernels keep their arithmetic but their scalar code comes out different, some with more SGPRs.
__device__ __forceinline__ const float* row(ScoreRefs a, long long r, long long s, long long c) { return a.p + r * a.sr + s * a.ss + c * a.sc; }
__device__ __forceinline__ const float* row(ScoreRows a, long long r, long long c) { return a.p + r * a.sr + c * a.sc; }

// Device data never becomes an address out of bounds.  The target of recording r: target[r] from device memory clamped to [0, S), or,
// with a null table, target0 (checked by the entry point) ...
__device__ __forceinline__ long long score_target(const long long* target, int target0, long long r, int S) {
  const long long t = target ? target[r] : (long long)target0;
  return t < 0 ? 0 : (t > S - 1 ? S - 1 : t);
}

// ... and the lag of (recording, channel) rc: lag[rc] from device memory clamped to [-D, D]; 0 with a null table.
__device__ __forceinline__ long long score_lag(const int* lag, long long rc, int D) {
  if (!lag) return 0;
  const int v = lag[rc];
  return v < -D ? -D : (v > D ? D : v);
}

// The sum of a double over the 64 lanes of a wave, in every lane: the xor butterfly, a fixed order.
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// The entry points' argument checks.  Each returns 0 or, with the message set, the library's error code; `what` is the entry's name.
// The signals, the output and the scored region [D, L - D) of every row: min_D <= D, and at least `least` samples beyond the 2 D.
inline int check_signals(const char* what, const ScoreSignals& a, bool with_mix, const void* out, int R, int S, int C, long long L, int D, int min_D,
                         int least, int max_R = 0x7fffffff) {
  M2H_REQUIRE(a.refs.p && a.est.p && (a.mix.p || !with_mix) && out, "%s: null pointer (refs %p, est %p, mix %p, out %p)", what, (const void*)a.refs.p,
              (const void*)a.est.p, (const void*)a.mix.p, out);
  M2H_REQUIRE(S >= 1 && S <= 6, "%s: S = %d reference sources; 1 .. 6 are supported", what, S);
  M2H_REQUIRE(C == 1 || C == 2, "%s: C = %d channels; 1 or 2 are supported", what, C);
  M2H_REQUIRE(R >= 1 && R <= max_R, "%s: R = %d recordings; 1 .. %d are supported", what, R, max_R);
  M2H_REQUIRE(D >= min_D && D <= SCORE_MAXD, "%s: D = %d samples; %d .. %d are supported", what, D, min_D, SCORE_MAXD);
  M2H_REQUIRE(L >= 2ll * D + least, "%s: L = %lld samples; at least 2 D + %d = %lld are required", what, L, least, 2ll * D + least);
  return 0;
}

inline int check_lag(const char* what, const int* lag, int D) {
  M2H_REQUIRE(lag ? D >= 1 : D == 0, "%s: lag %p with D = %d; a lag table needs D >= 1, a null pointer needs D = 0", what, (const void*)lag, D);
  return 0;
}

inline int check_target(const char* what, const long long* target, int target0, int S) {
  M2H_REQUIRE(target || (target0 >= 0 && target0 < S), "%s: target = %d is not one of the S = %d references", what, target0, S);
  return 0;
}

// J = ceil(n / tile) tiles in each of `rows` rows of one grid dimension.
inline int check_tiles(const char* what, long long n, int tile, long long rows, long long& J) {
  M2H_REQUIRE(tile >= 1, "%s: tile = %d samples; at least 1 is required", what, tile);
  J = (n + tile - 1) / tile;
  M2H_REQUIRE(J <= 0x7fffffffLL / rows, "%s: %lld rows * ceil(%lld / %d) = %lld tiles of each exceed a grid of 2^31 - 1 workgroups", what, rows, n, tile, J);
  return 0;
}
}  // namespace

}  // namespace m2h
