// Rational-rate conversion of recordings (m2h/audio/resample.py): a polyphase FIR, gfx950, fp32, wave64, one launch for all rows,
// no atomics, no scratch, deterministic.
//
// Definition (include/m2h.h): half = 10 * max(up, down), N = 2 * half + 1 taps h (designed on the host), L_out = ceil(L_in * up / down),
//   y[n] = sum_j x[j] * h[n * down - j * up + half],   x zero outside [0, L_in);
// polyphase form: t = n * down + half, p = t mod up, j0 = t div up, y[n] = sum_{k < T} G[p][k] * x[j0 - k], G[p][k] = h[p + k * up]
// (zero past the end), T = ceil(N / up).
//
// resample_tile_kernel<NPT, UP1>: a workgroup of 256 threads owns 256 * NPT consecutive outputs of one row.
//   1. The input span those outputs need, x[j0(first) - T + 1 .. j0(last)] -- about tile * down / up + T samples -- is staged into LDS
//      with 16-byte loads on the 16-byte grid of the address space: a row base is unaligned whenever L_in % 4 != 0, so the first slot
//      starts up to three samples early and the compute phase adds that shift.  A slot that leaves the buffer is loaded from a clamped
//      address and the samples outside [0, L_in) of THIS row are replaced by zero with a select: the zero extension at both ends and
//      the isolation of neighbouring rows are the same select.
//   2. The table is copied to LDS transposed, tab[k * upS + p] with upS odd: the copy reads G in memory order and its LDS writes step by
//      the odd stride (no bank conflict); the compute phase reads one k for all lanes, so the bank is p mod 32 -- distinct over 32
//      consecutive outputs whenever up is a multiple of 32 and down is odd (44.1 k -> 16 k, 22.05 k -> 16 k), a broadcast when up is
//      small (16 k -> 48 k), and unstructured for 16 k -> 44.1 k.  UP1 (48 k -> 16 k: one phase) skips the table: the tap index is
//      uniform over the wave and the taps come through the scalar cache.
//   3. Thread tid computes outputs tid + 256 * i: consecutive lanes read x at a stride of down / up samples (conflict-free for an
//      odd integer stride, a broadcast when up > down; a fractional stride wraps the banks: DESIGN 8.1 has the counters).  p and
//      j0 are derived once per output, tile-relative in 32 bits from one 64-bit block-uniform base: n * down passes 2^31 from
//      110 s of 44.1 kHz input.
//   4. The tile leaves through LDS: a scalar head up to the first 16-byte boundary of the destination, 16-byte stores, a scalar tail.
// resample_direct_kernel: the same sum straight from memory, one output per thread, for the ratios whose table and span do not fit
// into 64 KB of LDS (max(up, down) above a few hundred).
//
// Window form (m2h_resample_poly_win; m2h.audio.resample.ResamplerStream): both kernels take the input as a window -- row r holds the
// absolute samples [origin, origin + stride_in) at x[r * stride_in + j - origin], samples below 0 and at or past `end` are zero -- and
// produce the outputs [n_first, n_stop) of the definition into y[r * stride_out + n - n_first].  The whole recording is the window
// stride_in = end = L_in, origin = 0, n_first = 0, n_stop = stride_out = L_out.  The tile size depends on the ratio alone and an
// output's sum on its own n alone (the same p, j0 and k = 0 .. T-1 fmaf chain wherever its tile starts; fmaf(g, 0, acc) is exact), so
// a recording converted window by window equals the one-call result bit for bit.
#include "m2h_internal.h"

#include <cstdint>

namespace m2h {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_RATIO = 1024;              // max(up, down)
constexpr int RS_LDS_BYTES = 64 * 1024;

// floats of LDS a tile of `tile` outputs needs: (table, span) -- the host's upper bounds of what the kernel derives per block
static inline long long rs_table_floats(int up, int T) { return up == 1 ? 0 : (long long)T * (up | 1); }
static inline long long rs_span_floats(int tile, int up, int down, int T) {
  const long long span = ((long long)(tile - 1) * down + up - 1) / up + T;      // j0(last) - j0(first) + T at most
  return (span + 3 + 3) / 4 * 4;                                               // + the alignment shift, in whole 16-byte slots
}

template <int NPT, bool UP1>
__global__ __launch_bounds__(RS_THREADS) void resample_tile_kernel(const float* __restrict__ x, const float* __restrict__ G, float* __restrict__ y,
                                                                   long long stride_in, long long origin, long long end, long long n_first,
                                                                   long long n_stop, long long stride_out, int up, int down, int T, int half,
                                                                   long long total_in, unsigned tiles_per_row, int table_floats) {
  extern __shared__ __align__(16) float rs_lds[];
  constexpr int TILE = RS_THREADS * NPT;
  float* tab = rs_lds;                          // [T][upS]
  float* xs = rs_lds + table_floats;            // the staged span; table_floats % 4 == 0
  const int tid = threadIdx.x;
  const long long row = blockIdx.x / tiles_per_row;
  const long long n0 = n_first + (long long)(blockIdx.x % tiles_per_row) * TILE;
  const int cnt = (int)(n_stop - n0 < TILE ? n_stop - n0 : TILE);
  const long long t0 = n0 * down + half;
  const long long jb = t0 / up;                 // j0 of the tile's first output
  const int pb = (int)(t0 - jb * up);
  const long long jlo = jb - (T - 1);
  const int span = (int)((pb + (long long)(cnt - 1) * down) / up) + T;

  // ---- 1. the span, on the 16-byte grid of the address space
  const long long xa4 = (long long)(reinterpret_cast<uintptr_t>(x) >> 2);
  const long long rowA = xa4 + row * stride_in - origin;   // absolute float index of the row's sample 0 (outside the window when origin > 0)
  const long long A0 = rowA + jlo;
  const int shift = (int)(A0 & 3);
  const long long F0 = A0 >> 2;
  const long long Fmin = (xa4 + 3) >> 2, Fmax = ((xa4 + total_in) >> 2) - 1;   // the slots that lie inside the buffer
  const bool have_wide = Fmin <= Fmax;
  const int nslots = (shift + span + 3) >> 2;
  for (int q = tid; q < nslots; q += RS_THREADS) {
    const long long F = F0 + q;
    const long long Fc = F < Fmin ? Fmin : (F > Fmax ? Fmax : F);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (have_wide) v = *reinterpret_cast<const float4*>(static_cast<uintptr_t>(Fc) << 4);
    float e[4] = {v.x, v.y, v.z, v.w};
    const long long j = (F << 2) - rowA;        // sample index, in its row, of the slot's first sample
    if (F != Fc || !have_wide) {                // the first or last slot of the whole buffer: sample by sample, clamped
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        long long jj = j + u - origin;
        jj = jj < 0 ? 0 : (jj >= stride_in ? stride_in - 1 : jj);
        e[u] = x[row * stride_in + jj];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = (j + u >= 0 && j + u >= origin && j + u < end && j + u < origin + stride_in) ? e[u] : 0.f;
    *reinterpret_cast<float4*>(xs + 4 * q) = make_float4(e[0], e[1], e[2], e[3]);
  }
  // ---- 2. the table, transposed
  const int upS = up | 1;
  if (!UP1) {
    const int ntab = up * T;
    for (int i = tid; i < ntab; i += RS_THREADS) {
      const int p = i / T, k = i - p * T;
      tab[k * upS + p] = G[i];
    }
  }
  __syncthreads();

  // ---- 3. the sums
  int xb[NPT], ph[NPT];
  float acc[NPT];
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    int m = tid + RS_THREADS * i;
    m = m < cnt ? m : cnt - 1;                  // past the row's end: a valid output's addresses, never stored
    const int tr = pb + m * down;               // below 2048 * 1024 + 1024
    const int jr = tr / up;
    ph[i] = tr - jr * up;
    xb[i] = jr + (T - 1) + shift;               // LDS index of x[j0]
    acc[i] = 0.f;
  }
  if (UP1) {
    for (int k = 0; k < T; ++k) {
      const float g = G[k];
#pragma unroll
      for (int i = 0; i < NPT; ++i) acc[i] = fmaf(g, xs[xb[i] - k], acc[i]);
    }
  } else {
    for (int k = 0; k < T; ++k) {
      const float* tk = tab + k * upS;
#pragma unroll
      for (int i = 0; i < NPT; ++i) acc[i] = fmaf(tk[ph[i]], xs[xb[i] - k], acc[i]);
    }
  }
  __syncthreads();                              // every wave is done with the span and the table: the tile takes their place

  // ---- 4. the tile
  float* ot = rs_lds;
#pragma unroll
  for (int i = 0; i < NPT; ++i) ot[tid + RS_THREADS * i] = acc[i];
  __syncthreads();
  float* yr = y + row * stride_out + (n0 - n_first);
  int lead = (int)((4 - ((reinterpret_cast<uintptr_t>(yr) >> 2) & 3)) & 3);
  lead = lead < cnt ? lead : cnt;
  const int nfull = (cnt - lead) >> 2;
  if (tid < lead) yr[tid] = ot[tid];
  for (int q = tid; q < nfull; q += RS_THREADS) {
    const float* s = ot + lead + 4 * q;
    *reinterpret_cast<float4*>(yr + lead + 4 * q) = make_float4(s[0], s[1], s[2], s[3]);
  }
  const int done = lead + 4 * nfull;
  if (tid < cnt - done) yr[done + tid] = ot[done + tid];
}

__global__ __launch_bounds__(RS_THREADS) void resample_direct_kernel(const float* __restrict__ x, const float* __restrict__ G, float* __restrict__ y,
                                                                     long long stride_in, long long origin, long long end, long long n_first,
                                                                     long long n_stop, long long stride_out, int up, int down, int T, int half,
                                                                     unsigned tiles_per_row) {
  const long long row = blockIdx.x / tiles_per_row;
  const long long n = n_first + (long long)(blockIdx.x % tiles_per_row) * RS_THREADS + threadIdx.x;
  if (n >= n_stop) return;
  const long long t = n * down + half;
  const long long j0 = t / up;
  const float* g = G + (size_t)(t - j0 * up) * T;
  const float* xr = x + row * stride_in;
  float acc = 0.f;
  for (int k = 0; k < T; ++k) {
    const long long j = j0 - k;
    const long long jr = j - origin;
    const long long jc = jr < 0 ? 0 : (jr >= stride_in ? stride_in - 1 : jr);
    const float v = xr[jc];
    acc = fmaf(g[k], (j >= 0 && jr >= 0 && j < end && jr < stride_in) ? v : 0.f, acc);
  }
  y[row * stride_out + (n - n_first)] = acc;
}

template <int NPT>
static void rs_launch_tile(bool up1, unsigned grid, size_t lds, hipStream_t s, const float* x, const float* G, float* y, long long stride_in,
                           long long origin, long long end, long long n_first, long long n_stop, long long stride_out, int up, int down, int T, int half,
                           long long total_in, unsigned tiles_per_row, int table_floats) {
  if (up1)
    M2H_LAUNCH((resample_tile_kernel<NPT, true>), dim3(grid), dim3(RS_THREADS), lds, s, x, G, y, stride_in, origin, end, n_first, n_stop, stride_out, up,
               down, T, half, total_in, tiles_per_row, table_floats);
  else
    M2H_LAUNCH((resample_tile_kernel<NPT, false>), dim3(grid), dim3(RS_THREADS), lds, s, x, G, y, stride_in, origin, end, n_first, n_stop, stride_out, up,
               down, T, half, total_in, tiles_per_row, table_floats);
}

// The tile-or-direct choice of a ratio and the launch of outputs [n_first, n_stop) from the window (x, stride_in, origin, end); every
// argument has been checked.  Returns false when the grid would not fit.
static bool rs_run(const float* x, const float* G, float* y, int rows, long long stride_in, long long origin, long long end, long long n_first,
                   long long n_stop, long long stride_out, int up, int down, int T, int half, hipStream_t s, bool* direct) {
  const long long table = rs_table_floats(up, T);
  const int table_floats = (int)((table + 3) / 4 * 4);
  int npt = 0;
  size_t lds = 0;
  for (int c = 8; c >= 1 && !npt; c >>= 1) {
    const int tile = RS_THREADS * c;
    long long f = table_floats + rs_span_floats(tile, up, down, T);
    if (f < tile) f = tile;
    if (f * 4 <= RS_LDS_BYTES) {
      npt = c;
      lds = (size_t)f * 4;
    }
  }
  const long long tile = RS_THREADS * (npt ? npt : 1);
  const long long tiles_per_row = (n_stop - n_first + tile - 1) / tile;
  if (tiles_per_row * rows >= (1LL << 31)) return false;
  const unsigned grid = (unsigned)(tiles_per_row * rows);
  const long long total_in = (long long)rows * stride_in;
  const unsigned tpr = (unsigned)tiles_per_row;
  switch (npt) {
    case 8: rs_launch_tile<8>(up == 1, grid, lds, s, x, G, y, stride_in, origin, end, n_first, n_stop, stride_out, up, down, T, half, total_in, tpr, table_floats); break;
    case 4: rs_launch_tile<4>(up == 1, grid, lds, s, x, G, y, stride_in, origin, end, n_first, n_stop, stride_out, up, down, T, half, total_in, tpr, table_floats); break;
    case 2: rs_launch_tile<2>(up == 1, grid, lds, s, x, G, y, stride_in, origin, end, n_first, n_stop, stride_out, up, down, T, half, total_in, tpr, table_floats); break;
    case 1: rs_launch_tile<1>(up == 1, grid, lds, s, x, G, y, stride_in, origin, end, n_first, n_stop, stride_out, up, down, T, half, total_in, tpr, table_floats); break;
    default:
      M2H_LAUNCH(resample_direct_kernel, dim3(grid), dim3(RS_THREADS), 0, s, x, G, y, stride_in, origin, end, n_first, n_stop, stride_out, up, down, T, half, tpr);
  }
  *direct = npt == 0;
  return true;
}

// The checks and the launch of both entry points: outputs [n_first, n_first + count) from the window (x [rows][cap], origin, end) for
// the entry point `name` (`name` and `name_direct` are string literals: the labels m2h_last_kernel reports).  The whole recording is
// cap = end = L_in, origin = 0, n_first = 0, count = L_out (`whole`: the count must then be every output, not just few enough).
static int rs_window_run(const char* name, const char* name_direct, bool whole, const float* x, const float* G, float* y, int rows, long long cap, long long origin,
                         long long end, long long n_first, long long count, int up, int down, int T, m2h_stream stream) {
  M2H_REQUIRE(x && G && y, "%s: null pointer", name);
  M2H_REQUIRE(rows > 0 && cap > 0 && origin >= 0 && end > 0 && n_first >= 0 && up > 0 && down > 0 && T > 0,
              "%s: bad sizes (rows %d, cap %lld, origin %lld, end %lld, n_first %lld, up %d, down %d, T %d)", name, rows, cap, origin, end, n_first, up, down, T);
  M2H_REQUIRE(count > 0, "%s: count must be positive, got %lld", name, count);
  M2H_REQUIRE(up <= RS_MAX_RATIO && down <= RS_MAX_RATIO, "%s: ratio %d/%d is over the limit (max(up, down) <= %d)", name, up, down, RS_MAX_RATIO);
  M2H_REQUIRE(end <= (1LL << 40) && cap <= (1LL << 40) && count <= (1LL << 40) && (long long)rows * (cap > count ? cap : count) <= (1LL << 44),
              "%s: bad sizes (rows %d x cap %lld / count %lld is too long)", name, rows, cap, count);
  M2H_REQUIRE(!whole || count == (end * up + down - 1) / down, "%s: L_out %lld is not ceil(L_in * up / down) = %lld", name, count, (end * up + down - 1) / down);
  M2H_REQUIRE(n_first + count <= (end * up + down - 1) / down, "%s: outputs [%lld, %lld + %lld) pass ceil(end * up / down) = %lld", name, n_first, n_first, count,
              (end * up + down - 1) / down);
  const int half = 10 * (up > down ? up : down);
  M2H_REQUIRE((long long)T * up >= 2 * half + 1 && T <= 2 * half + 1, "%s: a table of T %d x up %d does not hold the %d taps of this ratio", name, T, up, 2 * half + 1);
  M2H_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0 && (reinterpret_cast<uintptr_t>(G) & 3) == 0,
              "%s: buffers must be 4-byte aligned", name);
  // the samples inside [0, end) that the outputs read: x[j0(n_first) - T + 1 .. j0(n_first + count - 1)]
  long long jlo = (n_first * down + half) / up - (T - 1);
  long long jhi = ((n_first + count - 1) * down + half) / up + 1;
  if (jlo < 0) jlo = 0;
  if (jhi > end) jhi = end;
  M2H_REQUIRE(jlo >= jhi || (jlo >= origin && jhi <= origin + cap), "%s: outputs [%lld, %lld + %lld) read samples [%lld, %lld), outside the window [%lld, %lld + %lld)", name,
              n_first, n_first, count, jlo, jhi, origin, origin, cap);
  bool direct = false;
  M2H_REQUIRE(rs_run(x, G, y, rows, cap, origin, end, n_first, n_first + count, count, up, down, T, half, as_stream(stream), &direct), "%s: bad sizes (too many tiles)",
              name);
  return launch_status(direct ? name_direct : name);
}

}  // namespace m2h

using namespace m2h;

extern "C" {

int m2h_resample_poly(const float* x, const float* G, float* y, int rows, long long L_in, long long L_out, int up, int down, int T, m2h_stream stream) {
  return rs_window_run("resample_poly", "resample_poly_direct", true, x, G, y, rows, L_in, 0, L_in, 0, L_out, up, down, T, stream);
}

int m2h_resample_poly_win(const float* x, const float* G, float* y, int rows, long long cap, long long origin, long long end, long long n_first,
                          long long count, int up, int down, int T, m2h_stream stream) {
  return rs_window_run("resample_poly_win", "resample_poly_win_direct", false, x, G, y, rows, cap, origin, end, n_first, count, up, down, T, stream);
}

}  // extern "C"

