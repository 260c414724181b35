// Auralizer (gfx950): binaural recordings of any length from sources and RIRs (m2h/audio/render.py holds the definition).
//
// Uniformly partitioned overlap-add: the source is cut into blocks of B = 16 000 samples, the RIR into partitions of B taps, and
// every block x partition product is a 32 768-point circular convolution (B + B - 1 = 31 999 points: no aliasing) -- the packed
// 16 384-point complex transform in 128 KB of LDS of the feeder's fftconv_kernel<14> (fft_lds.h).
//
//   frame_m = IFFT( sum over p ascending, 0 <= m - p < J, of X_{m-p} (.) H_{kappa(m-p), p} )       m = 0 .. J + Pn - 2
//   image[m B + i] = frame_m[i] + frame_{m-1}[B + i]                                               i < B
//
// Three launches:
//   render_spectra : one workgroup per row of at most B samples (a source block at element stride 1, one ear of an RIR partition at
//                    stride 2): forward transform in LDS, then the pair-wise unpack, ONCE per spectrum, and the real signal's
//                    spectrum S written to global memory in natural order: slot k <= M/2 holds S[k], slot M - k holds conj(S[M-k]),
//                    slot 0 the two real bins {S[0], S[M]}.  (The feeder's kernel keeps the packed, bit-reversed transform and unpacks
//                    inside its one product; here a spectrum enters up to Pn products of up to Pn + 1 frames, and a bit-reversed slot
//                    order would turn every load of the product loop into 64 cache lines per wave.  The values multiplied are the same.)
//   render_frames  : one workgroup per (r, s, m, ear): the Pn products of a thread's 8 pairs (k, M-k) are accumulated in registers
//                    straight from the global spectra (coalesced 8-byte loads, 16 in flight together, p ascending,
//                    no atomics), re-packed into bit-reversed LDS slots, inverse transform, the frame's first 2 B samples written with
//                    16-byte stores.
//   Both transform kernels run blocks of exactly 1024 threads and use the unrolled transforms of fft_lds.h, which read the twiddles
//   from a stage-ordered copy of the table (twiddles: [2][M] complex: the feeder's table, then that copy).
//   render_mix     : per output sample the two frames that cover it, for every source in order (an fmaf chain), cut at L_out.
#include "m2h_internal.h"
#include "fft_lds.h"

namespace m2h {

namespace {
constexpr int RB = 16000;              // block = partition length: one second, the Separator's segment
constexpr int RLOGM = 14;              // packed transform: 2^14 complex points = 32 768 real points
constexpr int RM = 1 << RLOGM;
constexpr int RFRAME = 2 * RB;         // samples of a frame that are kept (index 31 999 is the circular result's first zero)
constexpr int RMAXP = 16;              // RIR partitions: Lr <= 256 000
}  // namespace

// grid (nblk, n_mid * n_inner, n_outer).  Row (o, c, i) starts at x + o * outer_stride + c * mid_stride + i * inner_stride and has row_len
// samples at element stride es; block b holds its samples [(first_block + b) B, +B), zero past the row's end.
__global__ __launch_bounds__(1024) void render_spectra_kernel(const float* __restrict__ x, const cf* __restrict__ tw, cf* __restrict__ spec,
                                                              int n_inner, long long outer_stride, long long mid_stride, long long inner_stride,
                                                              long long row_len, int es, int first_block) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  const int mid = (int)blockIdx.y / n_inner, inner = (int)blockIdx.y - mid * n_inner;
  const float* row = x + (size_t)blockIdx.z * outer_stride + (size_t)mid * mid_stride + (size_t)inner * inner_stride;
  const long long a = (long long)(first_block + (int)blockIdx.x) * RB;
  const long long left = row_len - a;                      // samples of the row from the block's start on (>= 1: checked by the entry point)
  const int n = left < RB ? (int)left : RB;
  load_packed<RLOGM, 1024>(z, row + (size_t)a * es, n, es);
  __syncthreads();
  fft_dif_fixed<RLOGM, 1024>(z, tw + RM);                  // (the table's second half: the same twiddles in stage order)
  cf* out = spec + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * RM;
  auto pair = [&](int, int k) {
    cf e, to;
    rfft_unpack(tw[k], z[bit_rev<RLOGM>(k)], z[bit_rev<RLOGM>(RM - k)], e, to);
    out[k] = cadd(e, to);                                  // S[k]
    if (k != RM / 2) out[RM - k] = csub(e, to);            // conj(S[M-k])
  };
  auto dc = [&](int) {
    const cf z0 = z[0];
    out[0] = {z0.x + z0.y, z0.x - z0.y};                   // S[0], S[M]: both real
  };
  rfft_own_pairs<RLOGM, 1024>(dc, pair, [&] { pair(0, RM / 2); });
}

// grid (nm, RS, 2 ears).  xspec [RS][nx][M] holds the source blocks jx0 .. jx0 + nx - 1; hspec [RS][nh][2][Pn][M] the RIRs
// kh0 .. kh0 + nh - 1 (nh = 1, kh0 = 0 for a static scene); frames [RS][nm][2][2 B] the frames m0 .. m0 + nm - 1.
__global__ __launch_bounds__(1024) void render_frames_kernel(const cf* __restrict__ xspec, const cf* __restrict__ hspec, const cf* __restrict__ tw,
                                                             float* __restrict__ frames, int J, int Pn, int moving, int m0, int jx0, int nx, int kh0,
                                                             int nh) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  const int tid = threadIdx.x, rs = blockIdx.y, ear = blockIdx.z, nm = gridDim.x;
  const int m = m0 + (int)blockIdx.x;
  const int p_lo = m - (J - 1) > 0 ? m - (J - 1) : 0, p_hi = m < Pn - 1 ? m : Pn - 1;      // 0 <= m - p < J
  const cf* xs = xspec + (size_t)rs * nx * RM;
  const cf* hs = hspec + (size_t)rs * nh * 2 * Pn * RM;
  // The pairs (k, M-k), k = tid + 1024 i < M/2, 8 per thread, in two groups of NP = 4: a group's 16 loads of a partition are in flight
  // together and its 16 accumulator values stay in registers.  Thread 0 also has k = M/2, its own partner.
  constexpr int NP = 4;
  auto spectra_of = [&](int p, const cf*& X, const cf*& H) {
    const int j = m - p;
    X = xs + (size_t)(j - jx0) * RM;
    H = hs + (((size_t)(moving ? j - kh0 : 0) * 2 + ear) * Pn + p) * RM;
  };
#pragma unroll 1
  for (int grp = 0; grp < RM / 2 / 1024 / NP; ++grp) {
    const int k0 = tid + 1024 * NP * grp;
    cf yk[NP], ymc[NP];                                    // Y[k], conj(Y[M-k])
#pragma unroll
    for (int i = 0; i < NP; ++i) yk[i] = ymc[i] = {0.f, 0.f};
    for (int p = p_lo; p <= p_hi; ++p) {
      const cf *X, *H;
      spectra_of(p, X, H);
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int k = k0 + 1024 * i, km = (RM - k) & (RM - 1);          // (k = 0: slot 0 holds the two real bins)
        const cf xk = X[k], hk = H[k], xm = X[km], hm = H[km];
        if (k == 0) {
          yk[i].x = fmaf(xk.x, hk.x, yk[i].x);             // S[0]: real
          yk[i].y = fmaf(xk.y, hk.y, yk[i].y);             // S[M]: real
        } else {
          yk[i] = cadd(yk[i], cmul(xk, hk));
          ymc[i] = cadd(ymc[i], cmul(xm, hm));
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int k = k0 + 1024 * i;
      if (k == 0) {
        z[0] = rfft_repack_dc(yk[i].x, yk[i].y);
      } else {
        cf zk, zm;
        rfft_repack(tw[k], yk[i], ymc[i], zk, zm);
        z[bit_rev<RLOGM>(k)] = zk;
        z[bit_rev<RLOGM>(RM - k)] = zm;
      }
    }
  }
  if (tid == 0) {
    cf yh = {0.f, 0.f}, zk, zm;
    for (int p = p_lo; p <= p_hi; ++p) {
      const cf *X, *H;
      spectra_of(p, X, H);
      yh = cadd(yh, cmul(X[RM / 2], H[RM / 2]));
    }
    rfft_repack(tw[RM / 2], yh, conj(yh), zk, zm);
    z[bit_rev<RLOGM>(RM / 2)] = zk;
  }
  __syncthreads();
  ifft_dit_fixed<RLOGM, 1024>(z, tw + RM);
  float* out = frames + (((size_t)rs * nm + blockIdx.x) * 2 + ear) * RFRAME;
  const float sc = 1.f / (float)RM;
  for (int q = tid; q < RFRAME / 4; q += 1024) {
    const cf v0 = z[2 * q], v1 = z[2 * q + 1];
    *reinterpret_cast<float4*>(out + 4 * q) = make_float4(v0.x * sc, v0.y * sc, v1.x * sc, v1.y * sc);
  }
}

// grid (ceil((o1 - o0) B / 4 / 256), 2 ears, R), 256 threads, four consecutive samples per thread.  Output block o = n / B reads
// frame o (where o < F) and frame o - 1 (where o >= 1); frames [R S][nm][2][2 B] holds the frames m0 .. m0 + nm - 1.
__global__ __launch_bounds__(256) void render_mix_kernel(const float* __restrict__ frames, const float* __restrict__ gains, float* __restrict__ mix,
                                                         float* __restrict__ images, int S, int m0, int nm, int F, int o0, int o1, long long L_out) {
  const long long n = (long long)o0 * RB + 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
  if (n >= (long long)o1 * RB || n >= L_out) return;
  const int ear = blockIdx.y, r = blockIdx.z;
  const int o = (int)(n / RB), i = (int)(n - (long long)o * RB);      // B is a multiple of 4: the four samples share a block
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int left = L_out - n < 4 ? (int)(L_out - n) : 4;
  auto put = [&](float* row, float4 v) {
    float* dst = row + n;
    if (left == 4 && (reinterpret_cast<size_t>(dst) & 15) == 0) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x;
      if (left > 1) dst[1] = v.y;
      if (left > 2) dst[2] = v.z;
      if (left > 3) dst[3] = v.w;
    }
  };
  for (int s = 0; s < S; ++s) {
    const float* f = frames + (((size_t)(r * S + s) * nm) * 2 + ear) * RFRAME;        // frame m0 of (r, s, ear); a frame pair is 2 * RFRAME floats on
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < F) v = *reinterpret_cast<const float4*>(f + (size_t)(o - m0) * 2 * RFRAME + i);
    if (o >= 1) {
      const float4 t = *reinterpret_cast<const float4*>(f + (size_t)(o - 1 - m0) * 2 * RFRAME + RB + i);
      v = make_float4(v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w);
    }
    if (images) put(images + ((size_t)(r * S + s) * 2 + ear) * L_out, v);
    const float g = gains[r * S + s];
    acc = make_float4(fmaf(g, v.x, acc.x), fmaf(g, v.y, acc.y), fmaf(g, v.z, acc.z), fmaf(g, v.w, acc.w));
  }
  put(mix + ((size_t)r * 2 + ear) * L_out, acc);
}

}  // namespace m2h

using namespace m2h;

extern "C" int m2h_render_spectra(const float* x, const float* twiddles, float* spec, int n_outer, int n_mid, int n_inner, long long outer_stride,
                                  long long mid_stride, long long inner_stride, long long row_len, int elem_stride, int first_block, int nblk,
                                  m2h_stream stream) {
  M2H_REQUIRE(x && twiddles && spec, "render_spectra: null pointer");
  M2H_REQUIRE(n_outer > 0 && n_mid > 0 && n_inner > 0 && (long long)n_mid * n_inner <= 65535 && n_outer <= 65535 && nblk > 0 && row_len > 0 &&
                  outer_stride >= 0 && mid_stride >= 0 && inner_stride >= 0 && (elem_stride == 1 || elem_stride == 2),
              "render_spectra: bad sizes (rows %d x %d x %d, %d blocks, row length %lld, element stride %d)", n_outer, n_mid, n_inner, nblk, row_len,
              elem_stride);
  M2H_REQUIRE(first_block >= 0 && ((long long)first_block + nblk - 1) * RB < row_len,
              "render_spectra: window: blocks [%d, %d) of %d samples do not all start inside a row of %lld samples", first_block, first_block + nblk, RB,
              row_len);
  M2H_REQUIRE((reinterpret_cast<size_t>(spec) & 7) == 0 && (reinterpret_cast<size_t>(twiddles) & 7) == 0, "render_spectra: buffers must be 8-byte aligned");
  if (int rc = reserve_transform_lds<RLOGM>(render_spectra_kernel, "render_spectra")) return rc;
  M2H_LAUNCH(render_spectra_kernel, dim3(nblk, n_mid * n_inner, n_outer), dim3(1024), sizeof(cf) << RLOGM, as_stream(stream), x,
             reinterpret_cast<const cf*>(twiddles), reinterpret_cast<cf*>(spec), n_inner, outer_stride, mid_stride, inner_stride, row_len, elem_stride,
             first_block);
  return launch_status("render_spectra");
}

extern "C" int m2h_render_frames(const float* xspec, const float* hspec, const float* twiddles, float* frames, int RS, int J, int Pn, int K, int m0,
                                 int nm, int jx0, int nx, int kh0, int nh, m2h_stream stream) {
  M2H_REQUIRE(xspec && hspec && twiddles && frames, "render_frames: null pointer");
  M2H_REQUIRE(RS > 0 && RS <= 65535 && J > 0 && Pn > 0 && nm > 0 && nx > 0 && nh > 0, "render_frames: bad sizes (RS %d, J %d, Pn %d, %d frames)", RS, J, Pn, nm);
  M2H_REQUIRE(Pn <= RMAXP, "render_frames: %d RIR partitions; the limit is %d (an RIR of at most %d taps)", Pn, RMAXP, RMAXP * RB);
  M2H_REQUIRE(K == 1 || K == J, "render_frames: K = %d RIRs per source; 1 or J = %d is required", K, J);
  M2H_REQUIRE(m0 >= 0 && (long long)m0 + nm <= (long long)J + Pn - 1, "render_frames: window: frames [%d, %lld) outside [0, J + Pn - 1 = %lld)", m0,
              (long long)m0 + nm, (long long)J + Pn - 1);
  const int j_lo = m0 - (Pn - 1) > 0 ? m0 - (Pn - 1) : 0, j_hi = m0 + nm - 1 < J - 1 ? m0 + nm - 1 : J - 1;     // the source blocks these frames read
  M2H_REQUIRE(jx0 >= 0 && jx0 <= j_lo && j_hi < (long long)jx0 + nx, "render_frames: window: the frames read source blocks [%d, %d], the spectra hold [%d, %lld)",
              j_lo, j_hi, jx0, (long long)jx0 + nx);
  const int moving = K != 1;
  if (moving)
    M2H_REQUIRE(kh0 >= 0 && kh0 <= j_lo && j_hi < (long long)kh0 + nh, "render_frames: window: the frames read RIRs [%d, %d], the spectra hold [%d, %lld)", j_lo,
                j_hi, kh0, (long long)kh0 + nh);
  else
    M2H_REQUIRE(kh0 == 0 && nh == 1, "render_frames: window: a static scene has one RIR (kh0 = 0, nh = 1), got kh0 = %d, nh = %d", kh0, nh);
  M2H_REQUIRE((reinterpret_cast<size_t>(frames) & 15) == 0 && (reinterpret_cast<size_t>(xspec) & 7) == 0 && (reinterpret_cast<size_t>(hspec) & 7) == 0 &&
                  (reinterpret_cast<size_t>(twiddles) & 7) == 0,
              "render_frames: buffers: frames must be 16-byte aligned, spectra and twiddles 8-byte aligned");
  if (int rc = reserve_transform_lds<RLOGM>(render_frames_kernel, "render_frames")) return rc;
  M2H_LAUNCH(render_frames_kernel, dim3(nm, RS, 2), dim3(1024), sizeof(cf) << RLOGM, as_stream(stream), reinterpret_cast<const cf*>(xspec),
             reinterpret_cast<const cf*>(hspec), reinterpret_cast<const cf*>(twiddles), frames, J, Pn, moving, m0, jx0, nx, kh0, nh);
  return launch_status("render_frames");
}

extern "C" int m2h_render_mix(const float* frames, const float* gains, float* mix, float* images, int R, int S, int m0, int nm, int F, int o0, int o1,
                              long long L_out, m2h_stream stream) {
  M2H_REQUIRE(frames && gains && mix, "render_mix: null pointer");
  M2H_REQUIRE(R > 0 && R <= 65535 && S > 0 && nm > 0 && F > 0 && L_out > 0 && (long long)R * S <= 0x7fffffffll, "render_mix: bad sizes (R %d, S %d, %d frames of %d, L_out %lld)",
              R, S, nm, F, L_out);
  M2H_REQUIRE(o0 >= 0 && o1 > o0 && (long long)o0 * RB < L_out && (long long)(o1 - 1) * RB < L_out && o1 - 1 <= F,
              "render_mix: window: output blocks [%d, %d) outside a recording of %lld samples and %d frames", o0, o1, L_out, F);
  const int f_lo = o0 >= 1 ? o0 - 1 : 0, f_hi = o1 - 1 < F - 1 ? o1 - 1 : F - 1;                                // the frames these blocks read
  M2H_REQUIRE(m0 >= 0 && m0 <= f_lo && f_hi < (long long)m0 + nm, "render_mix: window: the blocks read frames [%d, %d], the buffer holds [%d, %lld)", f_lo, f_hi,
              m0, (long long)m0 + nm);
  M2H_REQUIRE((reinterpret_cast<size_t>(frames) & 15) == 0 && (reinterpret_cast<size_t>(mix) & 3) == 0 && (reinterpret_cast<size_t>(images) & 3) == 0,
              "render_mix: buffers: frames must be 16-byte aligned");
  const long long quads = ((long long)(o1 - o0) * RB) / 4;
  M2H_LAUNCH(render_mix_kernel, dim3((unsigned)((quads + 255) / 256), 2, R), dim3(256), 0, as_stream(stream), frames, gains, mix, images, S, m0, nm, F, o0, o1,
             L_out);
  return launch_status("render_mix");
}
