// RoomSimulator (m2h/audio/room.py holds the definition): binaural RIRs of shoebox rooms by the image-source method, one launch.
//
// params [Q][16] fp64 per RIR: room Lx Ly Lz, beta x0 x1 y0 y1 z0 z1, source x y z, listener x y z, yaw.  out [Q][taps][2] fp32.
//
// m2h_room_sim: grid (time tiles, RIRs), 512 threads; the workgroup owns ROOM_TILE = 512 output samples of both ears of one RIR, wave w
// the 64 samples from 64 w on, a lane one sample (two accumulators, one per ear).  Tile ntiles - 1 - blockIdx.x: the image count of a tile
// grows with the square of its time, so the expensive tiles start first.
//   1. Enumeration.  An image reaches the tile if the delay to one ear lies in [t0 - 41, t0 + 512 + 40); the ears lie HEAD_RADIUS from the
//      head centre, so the head-centre distance lies in the shell [r_lo, r_hi] (widened by 1 mm against rounding; a superset is allowed,
//      the tap test in step 3 is exact in integers).  Threads take the (p_x, m_x, p_y, m_y) pairs of the square around the disc of radius
//      r_hi, 512 at a time; a thread solves r_lo^2 <= X^2 + Y^2 + Z^2 <= r_hi^2 for Z = (1 - 2 p_z) s_z + 2 m_z L_z - l_z: up to four
//      runs of consecutive m_z (p_z = 0, 1; Z < 0, Z > 0), clipped to the orders max_order leaves.  A block prefix scan over the run
//      lengths gives every thread its place in the list: no counter, no atomics, the list order is the enumeration order.
//   2. Records, ROOM_CHUNK images of the list at a time, a thread per image: d, tau = d RATE / C, k = floor(tau), kr = round(tau) and
//      fr = tau - kr in fp64 with no contraction (the bits of numpy's float64), then per ear in fp32: fr, sp = -A sin(pi fr) / pi,
//      cos and sin of pi fr / 82, A.  G = exp2 of the fp64 sum of exponent x log2(beta), its integer part applied by ldexp.
//   3. Taps.  Every wave walks the chunk 64 images at a time: a lane fetches one image's records, a ballot names the image ears that reach
//      the wave's 64 samples, and only those are visited, their records broadcast by v_readlane.  A lane with j = n - kr: x = j - fr, sin(pi x) = -(-1)^j sin(pi fr), cos(pi x / 82) by the addition theorem from an LDS table over j:
//      the tap A sinc(x) cos^2(pi x / 82) keeps its relative accuracy next to the zeros of the sinc and at the window's end.
//   4. Every sample of the tile is stored exactly once, both ears in one 8-byte store; empty tiles store zeros.
// A lane adds the taps of its sample over the 64 images of a batch in list order and the batch sums in list order: the bits of an RIR depend on its 16 parameters, taps and max_order alone.
// Parameters are not validated on the host (that would wait for it): a row with a value that is not finite, a room side outside
// [ROOM_MIN_SIDE, ROOM_MAX_COORD] or a source or head centre outside the room is stored as NaN; nothing is enumerated for it.
#include "m2h_internal.h"

namespace m2h {

namespace {
constexpr int ROOM_TILE = 512;
constexpr int ROOM_THREADS = 512;
constexpr int ROOM_CHUNK = 1024;          // images of a list chunk in LDS
constexpr int ROOM_HALF_WIDTH = 41;
constexpr int ROOM_MAX_TAPS = 256000;
constexpr int ROOM_PARAMS = 16;
constexpr int ROOM_MAX_BATCH = 65535;
constexpr double ROOM_RATE = 16000.0;
constexpr double ROOM_C = 343.0;
constexpr double ROOM_HEAD_RADIUS = 0.0875;
constexpr double ROOM_EAR_PATTERN = 0.3;
constexpr double ROOM_MIN_SIDE = 0.5;
constexpr double ROOM_MAX_COORD = 1.0e5;
constexpr double ROOM_SHELL_MARGIN = 1.0e-3;
constexpr double ROOM_PI = 3.14159265358979323846;
constexpr int ROOM_FAR = 1 << 29;         // "no bound" of an m range

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }
}  // namespace

__global__ __launch_bounds__(ROOM_THREADS) void room_sim_kernel(const double* __restrict__ params, float* __restrict__ out, int taps, int max_order,
                                                                int ntiles) {
  __shared__ int s_kk[2][ROOM_CHUNK];                    // 2 k + (kr - k) per ear
  __shared__ float s_fr[2][ROOM_CHUNK], s_sp[2][ROOM_CHUNK], s_cf[2][ROOM_CHUNK], s_sf[2][ROOM_CHUNK], s_am[2][ROOM_CHUNK];
  __shared__ int s_dx[ROOM_CHUNK], s_dy[ROOM_CHUNK], s_dz[ROOM_CHUNK];          // 2 m + p per axis
  __shared__ double s_par[24];                           // the 16 parameters, log2(beta) x 6, -sin yaw, cos yaw
  __shared__ float2 s_win[2 * ROOM_HALF_WIDTH + 1];      // cos, sin of pi j / 82, j = -41 .. 41
  __shared__ int s_wsum[ROOM_THREADS / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long q = blockIdx.y;
  const int t0 = (ntiles - 1 - (int)blockIdx.x) * ROOM_TILE;
  const int tend = min(t0 + ROOM_TILE, taps);
  float2* row = reinterpret_cast<float2*>(out) + q * (long long)taps;

  if (tid < ROOM_PARAMS) s_par[tid] = params[q * ROOM_PARAMS + tid];
  if (tid < 2 * ROOM_HALF_WIDTH + 1) {
    const double a = (double)(tid - ROOM_HALF_WIDTH) / (2.0 * ROOM_HALF_WIDTH);
    s_win[tid] = make_float2((float)cospi(a), (float)sinpi(a));
  }
  __syncthreads();
  if (tid >= 64 && tid < 70) s_par[16 + tid - 64] = fmax(log2(s_par[3 + tid - 64]), -1.0e6);       // beta = 0: any exponent > 0 gives G = 0, 0 gives 1
  if (tid == 70) s_par[22] = -sin(s_par[15]);
  if (tid == 71) s_par[23] = cos(s_par[15]);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < ROOM_PARAMS; ++i) {
    const double v = s_par[i];
    ok = ok && fabs(v) <= ROOM_MAX_COORD;                                  // (false for NaN and infinity)
    if (i < 3) ok = ok && v >= ROOM_MIN_SIDE;
    if (i >= 9 && i < 15) ok = ok && v >= 0.0 && v <= s_par[(i - 9) % 3];  // source and head centre inside the room: that bounds the enumeration
  }
  __syncthreads();
  const int n = t0 + tid;
  if (!ok) {
    if (n < tend) row[n] = make_float2(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000));
    return;
  }

  const double Lx = s_par[0], Ly = s_par[1], Lz = s_par[2];
  const double sx = s_par[9], sy = s_par[10], sz = s_par[11], lx = s_par[12], ly = s_par[13], lz = s_par[14];
  const double r_hi = (double)(tend + ROOM_HALF_WIDTH - 1) * (ROOM_C / ROOM_RATE) + ROOM_HEAD_RADIUS + ROOM_SHELL_MARGIN;
  const double r_lo = fmax((double)(t0 - ROOM_HALF_WIDTH) * (ROOM_C / ROOM_RATE) - ROOM_HEAD_RADIUS - ROOM_SHELL_MARGIN, 0.0);
  const int mcap = max_order >= 0 ? max_order / 2 + 1 : ROOM_FAR;
  const int mxlo = max((int)floor((lx - r_hi - fabs(sx)) / (2.0 * Lx)), -mcap), mxhi = min((int)ceil((lx + r_hi + fabs(sx)) / (2.0 * Lx)), mcap);
  const int mylo = max((int)floor((ly - r_hi - fabs(sy)) / (2.0 * Ly)), -mcap), myhi = min((int)ceil((ly + r_hi + fabs(sy)) / (2.0 * Ly)), mcap);
  const int NX = max(2 * (mxhi - mxlo + 1), 0), NY = max(2 * (myhi - mylo + 1), 0);
  const long long npairs = (long long)NX * NY;

  float acc0 = 0.f, acc1 = 0.f;
  for (long long pb = 0; pb < npairs; pb += ROOM_THREADS) {
    // 1. the runs of m_z of this thread's pair
    int cnt[4] = {0, 0, 0, 0}, first[4] = {0, 0, 0, 0}, dxc = 0, dyc = 0;
    const long long pid = pb + tid;
    if (pid < npairs) {
      const int ix = (int)(pid % NX), iy = (int)(pid / NX);
      const int px = ix & 1, mx = mxlo + (ix >> 1), py = iy & 1, my = mylo + (iy >> 1);
      dxc = mx * 2 + px, dyc = my * 2 + py;
      const double X = (double)(1 - 2 * px) * sx + (double)(2 * mx) * Lx - lx, Y = (double)(1 - 2 * py) * sy + (double)(2 * my) * Ly - ly;
      const int oxy = iabs(mx - px) + iabs(mx) + iabs(my - py) + iabs(my);
      const double rem_hi = r_hi * r_hi - X * X - Y * Y, rem_lo = r_lo * r_lo - X * X - Y * Y;
      if (rem_hi >= 0.0 && (max_order < 0 || oxy <= max_order)) {
        const double zhi = sqrt(rem_hi);
        const bool split = rem_lo > 1.0e-12;               // a hole about Z = 0; below that the two runs are taken as one
        const double zlo = split ? sqrt(rem_lo) : 0.0;
        const int left = max_order - oxy;                  // the orders left for the z walls
#pragma unroll
        for (int pz = 0; pz < 2; ++pz) {
          const double a = (double)(1 - 2 * pz) * sz - lz;
          int olo = -ROOM_FAR, ohi = ROOM_FAR;
          if (max_order >= 0) {
            if (pz == 0) olo = -(left / 2), ohi = left / 2;                          // 2 |m| <= left
            else olo = left >= 1 ? -((left - 1) / 2) : 1, ohi = (left + 1) / 2;      // |m - 1| + |m| <= left
          }
          const double inv = 1.0 / (2.0 * Lz);
          const int a_lo = max((int)ceil((-zhi - a) * inv), olo), a_hi = min((int)floor(((split ? -zlo : zhi) - a) * inv), ohi);
          first[2 * pz] = a_lo, cnt[2 * pz] = max(a_hi - a_lo + 1, 0);
          if (split) {
            const int b_lo = max((int)ceil((zlo - a) * inv), olo), b_hi = min((int)floor((zhi - a) * inv), ohi);
            first[2 * pz + 1] = b_lo, cnt[2 * pz + 1] = max(b_hi - b_lo + 1, 0);
          }
        }
      }
    }
    const int mine = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int off = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < ROOM_THREADS / 64; ++w) {
      const int v = s_wsum[w];
      if (w < wave) off += v;
      total += v;
    }
    __syncthreads();

    for (int w0 = 0; w0 < total; w0 += ROOM_CHUNK) {
      const int nimg = min(ROOM_CHUNK, total - w0);
      // the thread's images that fall into this chunk of the list
      {
        const int lo = max(off, w0), hi = min(off + mine, w0 + ROOM_CHUNK);
        int base = off;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          for (int i = max(base, lo); i < min(base + cnt[r], hi); ++i) {
            s_dx[i - w0] = dxc, s_dy[i - w0] = dyc;
            s_dz[i - w0] = (first[r] + (i - base)) * 2 + (r >> 1);
          }
          base += cnt[r];
        }
      }
      __syncthreads();
      // 2. records
      for (int i = tid; i < nimg; i += ROOM_THREADS) {
#pragma clang fp contract(off)
        const int cx = s_dx[i], cy = s_dy[i], cz = s_dz[i];
        const int px = cx & 1, mx = cx >> 1, py = cy & 1, my = cy >> 1, pz = cz & 1, mz = cz >> 1;
        const double gx = (double)(1 - 2 * px) * sx + (double)(2 * mx) * Lx;
        const double gy = (double)(1 - 2 * py) * sy + (double)(2 * my) * Ly;
        const double gz = (double)(1 - 2 * pz) * sz + (double)(2 * mz) * Lz;
        const double arg = (double)iabs(mx - px) * s_par[16] + (double)iabs(mx) * s_par[17] + (double)iabs(my - py) * s_par[18] +
                           (double)iabs(my) * s_par[19] + (double)iabs(mz - pz) * s_par[20] + (double)iabs(mz) * s_par[21];
        const double ai = floor(arg);
        const float G = ldexpf(exp2f((float)(arg - ai)), (int)fmin(fmax(ai, -400.0), 400.0));
        const double ux = s_par[22], uy = s_par[23];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const double axx = e ? -ux : ux, axy = e ? -uy : uy;
          const double ex = e ? lx - ROOM_HEAD_RADIUS * ux : lx + ROOM_HEAD_RADIUS * ux, ey = e ? ly - ROOM_HEAD_RADIUS * uy : ly + ROOM_HEAD_RADIUS * uy;
          const double vx = gx - ex, vy = gy - ey, vz = gz - lz;
          const double d = sqrt(vx * vx + vy * vy + vz * vz);
          const double cs = d > 0.0 ? (vx * axx + vy * axy) / d : 1.0;
          const float A = (float)(((1.0 - ROOM_EAR_PATTERN) + ROOM_EAR_PATTERN * cs) / (4.0 * ROOM_PI * fmax(d, ROOM_HEAD_RADIUS))) * G;
          const double tau = d * ROOM_RATE / ROOM_C;
          const double k = floor(tau), kr = floor(tau + 0.5);
          const float fr = (float)(tau - kr);
          s_kk[e][i] = 2 * (int)k + (int)(kr - k);
          s_fr[e][i] = fr;
          s_sp[e][i] = -(A * sinf((float)ROOM_PI * fr)) / (float)ROOM_PI;
          s_cf[e][i] = cosf((float)(ROOM_PI / (2.0 * ROOM_HALF_WIDTH)) * fr);
          s_sf[e][i] = sinf((float)(ROOM_PI / (2.0 * ROOM_HALF_WIDTH)) * fr);
          s_am[e][i] = A;
        }
      }
      __syncthreads();
      // 3. taps: the wave's samples are [nw, nw + 64).  A lane fetches the record of one image; the ballot names the image ears whose
      // taps k - 40 .. k + 41 meet the wave's samples, and only those are visited, in list order, their records broadcast from the lane.
      const int nw = t0 + wave * 64;
      for (int i0 = 0; i0 < nimg; i0 += 64) {
        const int i = i0 + lane;                           // < ROOM_CHUNK; past nimg the slots hold stale records that kk masks out
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int kk = i < nimg ? s_kk[e][i] : -(1 << 30);
          const float fr = s_fr[e][i], sp = s_sp[e][i], cf = s_cf[e][i], sf = s_sf[e][i], am = s_am[e][i];
          const int k = kk >> 1;
          unsigned long long hits = __ballot(k + ROOM_HALF_WIDTH >= nw && k - (ROOM_HALF_WIDTH - 1) <= nw + 63);
          float acc = 0.f;
          while (hits) {
            const int b = __builtin_ctzll(hits);
            hits &= hits - 1;
            const int kkb = __builtin_amdgcn_readlane(kk, b);
            const float frb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fr), b));
            const float spb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sp), b));
            const float cfb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cf), b));
            const float sfb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sf), b));
            const float amb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(am), b));
            const int j = n - (kkb >> 1);
            if (j >= -(ROOM_HALF_WIDTH - 1) && j <= ROOM_HALF_WIDTH) {
              const int jr = j - (kkb & 1);                // -41 .. 41
              const float x = (float)jr - frb;
              const float2 cw = s_win[jr + ROOM_HALF_WIDTH];
              const float c = cw.x * cfb + cw.y * sfb;
              const float v = x == 0.f ? amb : ((jr & 1) ? -spb : spb) * __builtin_amdgcn_rcpf(x);
              acc += v * c * c;
            }
          }
          if (e == 0) acc0 += acc; else acc1 += acc;
        }
      }
      __syncthreads();
    }
  }
  // 4. every sample of the tile, once
  if (n < tend) row[n] = make_float2(acc0, acc1);
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_room_sim(const double* params, float* rirs, int Q, int taps, int max_order, m2h_stream stream) {
  M2H_REQUIRE(params && rirs, "room_sim: null pointer (params %p, rirs %p)", (const void*)params, (const void*)rirs);
  M2H_REQUIRE(taps >= 1 && taps <= ROOM_MAX_TAPS, "room_sim: taps = %d; 1 .. %d are supported", taps, ROOM_MAX_TAPS);
  M2H_REQUIRE(Q >= 1 && Q <= ROOM_MAX_BATCH, "room_sim: Q = %d RIRs; one launch takes 1 .. %d", Q, ROOM_MAX_BATCH);
  M2H_REQUIRE(max_order >= -1, "room_sim: max_order = %d; an order >= 0, or -1 for every order, is required", max_order);
  M2H_REQUIRE(((reinterpret_cast<size_t>(params) | reinterpret_cast<size_t>(rirs)) & 7) == 0, "room_sim: params and rirs must be 8-byte aligned");
  const int ntiles = (taps + ROOM_TILE - 1) / ROOM_TILE;
  M2H_LAUNCH(room_sim_kernel, dim3((unsigned)ntiles, (unsigned)Q), dim3(ROOM_THREADS), 0, as_stream(stream), params, rirs, taps, max_order, ntiles);
  return launch_status("room_sim");
}
