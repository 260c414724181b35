// Implicit-GEMM convolution for gfx950 (MI355X), fp32 in / fp32 accumulate on the matrix cores: the register-staged engine, the
// last of the forward dispatch's engines (conv_dispatch.hip; the others live in units of their own, igemm_common.h) and the home of
// the split-K rule and reduce they share.
//
// Replaces, in the reference, every Conv2d / ConvTranspose2d (+BatchNorm2d(eval) + activation) of the
// separator U-Nets (audio_separation/rl/models/separator_cnn.py:5-24,46-52,128-135) and, through the same
// engine, the 3x3 convs of AcousticMem (rl/models/memory_nets.py:11-16).
//
// GEMM view:  D[m][n] = sum_k A[m][k] * W[n][k]
//   m = (b, q, r) over the output pixel grid of one sub-pixel phase, n = output channel,
//   k = (th, tw, ci): kernel tap x input channel, input channels being the concatenation of two NHWC
//   sources (the U-Net skip concat is read in place, never materialised).
// A is gathered on the fly from NHWC activations (channel-contiguous 16-byte segments, zero outside the
// image); W is pre-packed [n][k] (m2h_pack_conv*_weight).  Both are staged global -> VGPR -> LDS with a
// register double buffer (one barrier per 32-deep k-tile), LDS rows padded 32 -> 36 floats so that the
// ds_read_b128 fragment reads are bank-conflict free.  Each wave owns a (TM x TN) sub-tile as FM x FN
// v_mfma_f32_32x32x2_f32 accumulators: one 16-byte LDS read feeds four MFMAs (lane (i, h) holds
// k = 8g + 4h + {0..3} of row i; MFMA j of the group contracts k = 8g + j and 8g + 4 + j).  The f32 MFMA
// is a k-ordered fp32 FMA chain, so results match an fp32 CPU convolution to rounding.
//
// Epilogue (fused): optional target-class plane (border-aware bias), BatchNorm(eval) scale/shift,
// LeakyReLU/ReLU, and the store either NHWC or de-sliced straight into the reference's BHWC layout.
//
// Block -> tile map: n-tiles of one m-tile are consecutive on one XCD (blocks b and b+8 share an XCD's
// L2), so the gathered A panel is fetched from HBM once and re-read from L2 by its sibling n-tiles.
#include <string>

#include "igemm_common.h"

#ifndef M2H_SCHED
#define M2H_SCHED 0  // instruction-interleave experiment selector for the k-loop (0 = compiler default)
#endif

namespace m2h {

#ifdef M2H_CLOCK_DIAG
// Diagnostic build only (tools/clock_diag.py): shader-clock vs 100 MHz real-time stamps around the k-loop of each block, to read
// the clock the chip holds under this kernel (MI355X_MICROARCH.md, DVFS give-back item 6).  Never compiled into libm2h.so.
__device__ unsigned long long g_clock_dbg[8192][6];
#endif

// FR = MFMA fragment edge: 32 (v_mfma_f32_32x32x2_f32, 8 k per 16-byte LDS read) or 16 (v_mfma_f32_16x16x4_f32, 16 k per read;
// used for N <= 16 so that a 16-channel layer does not pay for a half-empty 32-wide tile).  Same FLOP rate per cycle.
//
// FAST = 1 (both sources' channel counts multiples of the 32-deep k-tile, operands < 4 GiB): every k-tile lies inside one
// (tap, source) segment, so the whole k decode is SCALAR (SGPR) work and a load's address is `uniform base + per-lane 32-bit
// offset` with the per-lane part recomputed only when the segment changes (every C/32 tiles).  The generic path decodes k per
// lane (any C % 4 == 0) and costs ~250 vector instructions per k-tile, which made the k-loop issue-bound beside 64 MFMAs.
//
// SPLIT = 1 | 2 ("bf16x3" math; 2 = both operands already arrive in the split32 layout, no conversion in the loop): fp32 operands are split on their way into LDS into bf16 high and low parts (x = hi + lo to 2^-17
// relative) and each product a*b is formed as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the bf16 matrix pipe with fp32 accumulation
// (the dropped a_lo*b_lo term is 2^-16 of the dropped precision again): three bf16 MFMAs replace sixteen (32x32) or eight
// (16x16) fp32 MFMAs per fragment and 32-deep k-tile -- the bf16 pipe is 16x the fp32 one -- at ~16 mantissa bits per product
// instead of 24.  Tensors in HBM stay fp32; the LDS row keeps its 144-byte stride ([hi 64 B | lo 64 B | pad]) and the fragment
// reads are byte-for-byte those of the fp32 path.  Measured end to end on the U-Net pair: rel-L1 1e-5 vs the fp32 reference
// (plain bf16 operands: 4e-3..6e-3, outside the 1e-3 contract).
template <int BM, int BN, int WM, int WN, int NSTAGE, int FR = 32, int FAST = 0, int SPLIT = 0>
__global__ __launch_bounds__(64 * WM * WN, (SPLIT && WM * WN == 4) ? 2 : 1) void igemm_f32_kernel(const IGemmP p) {
  static_assert(WM * WN == 4 || WM * WN == 8, "4 or 8 waves per block");
  constexpr int NT = 64 * WM * WN;           // threads per block
  constexpr int RPP = NT / 8;                // tile rows staged per pass (a row = 8 threads x 16 bytes)
  constexpr int TM = BM / WM, TN = BN / WN;  // wave tile
  constexpr int FM = TM / FR, FN = TN / FR;  // MFMA fragments per wave
  constexpr int BNS = BN < RPP ? RPP : BN;   // staged weight rows (a pass stages RPP rows)
  constexpr int AR = BM / RPP, BR = BNS / RPP; // staged rows per thread
  constexpr int GK = FR == 32 ? 8 : 16;      // k covered by one fragment group (one 16-byte read per lane)
  constexpr int NG = BK / GK;                // fragment groups per k-tile
  constexpr int NE = FR == 32 ? 16 : 4;      // accumulator elements per lane
  using AccT = typename std::conditional<FR == 32, f32x16, f32x4>::type;
  static_assert(FM >= 1 && FN >= 1, "wave tile must hold at least one fragment");

  __shared__ __attribute__((aligned(16))) float As[NSTAGE][BM * LDK];
  __shared__ __attribute__((aligned(16))) float Bs[NSTAGE][BNS * LDK];
  __shared__ int ri_qh[BM], ri_rw[BM], ri_bpix[BM], ri_out[BM], ri_bc[BM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int seg = tid & 7;    // 16-byte segment inside the 128-byte k-tile row
  const int srow = tid >> 3;  // 0..RPP-1

  // ---- block -> (m-tile, n-tile): siblings (same m-tile) run back to back on one XCD ----
  const int L = blockIdx.x;
  const int xcd = L & 7;
  int idx = L >> 3;
  // transposed conv: the four sub-pixel phases of one m-tile read the same 3x3 input neighbourhood; with pmaj they are
  // consecutive blocks of one XCD (input tile served by that XCD's L2) instead of four passes over the whole input
  int phase = 0;
  if (p.convT) {
    if (p.pmaj) {
      phase = idx & 3;
      idx >>= 2;
    } else {
      phase = blockIdx.z;
    }
  }
  const int mt = (idx / p.NT) * 8 + xcd;
  const int nt = idx - (idx / p.NT) * p.NT;
  if (mt >= p.MT) return;  // whole block leaves before any barrier
  const int m0 = mt * BM;
  const int n0 = nt * BN;

  int mulh = p.mulh, offh = p.offh, mulw = p.mulw, offw = p.offw, ph = p.ph, pw = p.pw;
  const float* wbase = p.w;
  if (p.convT) {
    ph = phase >> 1;
    pw = phase & 1;
    mulh = 2 * ph - 1;
    mulw = 2 * pw - 1;
    offh = 0;
    offw = 0;
    wbase += (size_t)phase * p.N * p.K;
  }

  // ---- per-row (output pixel) bookkeeping, once per block ----
  for (int r = threadIdx.x; r < BM; r += NT) {
    const int m = m0 + r;
    int qh = -(1 << 24), rw = -(1 << 24), bpix = 0, out = -1, bc = 0;
    if (m < p.M) {
      int q, rr, b;
      decode_row(p, m, ph, pw, q, rr, b, out, bc);
      qh = q * p.stride + offh;
      rw = rr * p.stride + offw;
      bpix = b * p.Hi * p.Wi;
    }
    ri_qh[r] = qh;
    ri_rw[r] = rw;
    ri_bpix[r] = bpix;
    ri_out[r] = out;
    ri_bc[r] = bc;
  }
  __syncthreads();

  int a_qh[AR], a_rw[AR], a_bpix[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    a_qh[i] = ri_qh[srow + RPP * i];
    a_rw[i] = ri_rw[srow + RPP * i];
    a_bpix[i] = ri_bpix[srow + RPP * i];
  }

  AccT acc[FM][FN];
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[mi][ni][e] = 0.f;
  // accumulator element e of this lane -> fragment row (C/D layout of the two MFMA shapes); column = lane & (FR-1)
  auto row_of = [&](int e) { return FR == 32 ? (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) : (lane >> 4) * 4 + e; };

  // Two register sets for the staged tile: the loads of k-tile t+2 are issued at the top of tile t's MFMA phase and are not
  // consumed (LDS write) until the end of tile t+1, so a loaded-chip HBM/L2 round trip (several microseconds) has a whole
  // tile of MFMAs (>= 4096 cycles on the 128x128 tile) to land instead of the tail of the current one.
  f32x4 ra[2][AR], rb[2][BR];
  unsigned okmask[2] = {0u, 0u};
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const int nk_all = ((FAST ? p.Kw : p.K) + BK - 1) / BK;
  const int split = blockIdx.y;
  const int kt0 = (int)(((long)nk_all * split) / p.S);
  const int kt1 = (int)(((long)nk_all * (split + 1)) / p.S);
  const int k_end = min(p.K, kt1 * BK);  // loads past this block's k-range are masked (they re-read element 0: a cache hit)

  // ---- loader state for the tile being loaded (advanced incrementally, one k-tile at a time) ----
  // generic: per-lane k = kt*BK + seg*4 -> (th, tw, ci)
  int ld_k, ld_th, ld_tw, ld_ci;
  bool t_kok;
  int t_dh, t_dw, t_Cs, t_c;
  const float* t_src;
  // FAST: uniform tile index / tap / channel offset; per-lane byte offsets of the staged rows inside the current segment
  int u_kt, u_th, u_tw, u_ci;
  unsigned voffA[AR], voffB[BR], okA = 0;

  auto seek_generic = [&](int kt) {
    ld_k = kt * BK + seg * 4;
    int tap = 0;
    ld_ci = ld_k;
    if (p.ntap > 1) {
      tap = (unsigned)ld_k / (unsigned)p.Ctot;
      ld_ci = ld_k - tap * p.Ctot;
    }
    ld_th = (unsigned)tap / (unsigned)p.ntw;
    ld_tw = tap - ld_th * p.ntw;
  };
  // FAST: per-lane row offsets for the current (tap, source) segment
  auto segment_rows = [&]() {
    const int dh = u_th * mulh, dw = u_tw * mulw;
    const int Cs = (u_ci >= p.C0 && p.src1 != nullptr) ? p.C1 : p.C0;
    okA = 0;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int ih = a_qh[i] + dh, iw = a_rw[i] + dw;
      const bool ok = (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
      voffA[i] = ok ? ((unsigned)(a_bpix[i] + ih * p.Wi + iw) * (unsigned)Cs + (unsigned)(seg * 4)) * 4u : 0u;
      okA |= ok ? (1u << i) : 0u;
    }
  };
  auto loader_seek = [&](int kt) {
    if constexpr (FAST) {
      u_kt = kt;
      const int k0 = kt * BK;
      const int tap = p.ntap > 1 ? k0 / p.Ctot : 0;   // index inside the tap window
      u_ci = k0 - tap * p.Ctot;
      u_th = p.th0 + tap / p.twn;
      u_tw = p.tw0 + tap % p.twn;
      segment_rows();
#pragma unroll
      for (int j = 0; j < BR; ++j)  // rows past N re-read row N-1 (their products are never stored): no mask on the weight side
        voffB[j] = ((unsigned)min(n0 + srow + RPP * j, p.N - 1) * (unsigned)p.K + (unsigned)(seg * 4)) * 4u;
    } else {
      seek_generic(kt);
    }
  };
  auto loader_next = [&]() {
    if constexpr (FAST) {
      if (u_kt + 1 < kt1) {  // past this block's k-range the loader stays on the last tile (a harmless cached re-read)
        ++u_kt;
        u_ci += BK;
        bool reseg = u_ci == p.C0 && p.src1 != nullptr;
        if (u_ci == p.Ctot) {
          u_ci = 0;
          reseg = true;
          if (++u_tw == p.tw0 + p.twn) {
            u_tw = p.tw0;
            ++u_th;
          }
        }
        if (reseg) segment_rows();  // wave-uniform branch
      }
    } else {
      if (p.Ctot >= BK) {  // at most one wrap per 32-deep step; selects, not branches (the wrap differs per lane)
        ld_k += BK;
        ld_ci += BK;
        const bool wrap = ld_ci >= p.Ctot;
        ld_ci -= wrap ? p.Ctot : 0;
        ld_tw += wrap ? 1 : 0;
        const bool wrap2 = ld_tw == p.ntw;
        ld_tw = wrap2 ? 0 : ld_tw;
        ld_th += wrap2 ? 1 : 0;
      } else {
        seek_generic(ld_k / BK + 1);
      }
    }
  };
  // Generic loads are unconditional (clamped to element 0 of the source when masked) and zeroed by a select afterwards: no
  // divergent branches in the k-loop, so the loads can be scheduled into the MFMA shadows.
  // The loaded value is NOT touched until store_tile (a select right after the load would force a vmcnt(0) wait there);
  // the validity bits travel in a mask.
  auto load_a = [&](int set, int i) {
    const int ih = a_qh[i] + t_dh, iw = a_rw[i] + t_dw;
    const bool ok = t_kok && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
    const unsigned off = ok ? (unsigned)(a_bpix[i] + ih * p.Wi + iw) * (unsigned)t_Cs + (unsigned)t_c : 0u;
    ra[set][i] = *reinterpret_cast<const f32x4*>(t_src + off);
    okmask[set] = ok ? (okmask[set] | (1u << i)) : (okmask[set] & ~(1u << i));
  };
  auto load_b = [&](int set, int j) {
    const int n = n0 + srow + RPP * j;
    const bool ok = t_kok && n < p.N;
    const unsigned off = ok ? (unsigned)n * (unsigned)p.K + (unsigned)ld_k : 0u;
    rb[set][j] = *reinterpret_cast<const f32x4*>(wbase + off);
    okmask[set] = ok ? (okmask[set] | (1u << (8 + j))) : (okmask[set] & ~(1u << (8 + j)));
  };
  auto load_tile = [&](int set) {
    if constexpr (FAST) {
      const bool second = u_ci >= p.C0 && p.src1 != nullptr;
      const char* baseA = reinterpret_cast<const char*>(second ? p.src1 + (u_ci - p.C0) : p.src0 + u_ci);  // uniform
      const char* baseB = reinterpret_cast<const char*>(wbase + (size_t)(u_th * p.ntw + u_tw) * p.Ctot + u_ci);  // uniform
#pragma unroll
      for (int i = 0; i < AR; ++i) ra[set][i] = *reinterpret_cast<const f32x4*>(baseA + voffA[i]);
#pragma unroll
      for (int j = 0; j < BR; ++j) rb[set][j] = *reinterpret_cast<const f32x4*>(baseB + voffB[j]);
      okmask[set] = okA;
    } else {
      t_kok = ld_k < k_end;
      t_dh = ld_th * mulh;
      t_dw = ld_tw * mulw;
      t_src = p.src0;
      t_Cs = p.C0;
      t_c = ld_ci;
      if (ld_ci >= p.C0 && p.src1 != nullptr) {  // second source; beyond-K padding tiles of a single-source conv keep src0
        t_src = p.src1;
        t_Cs = p.C1;
        t_c = ld_ci - p.C0;
      }
#pragma unroll
      for (int i = 0; i < AR; ++i) load_a(set, i);
#pragma unroll
      for (int j = 0; j < BR; ++j) load_b(set, j);
    }
  };
  // SPLIT: [hi bf16 x 32 | lo bf16 x 32] per row; this thread's four k-values land at byte seg*8 of each half
  auto store_split = [&](float* rowp, f32x4 v) {
    const bf16x4 hi = __builtin_convertvector(v, bf16x4);
    const f32x4 hf = __builtin_convertvector(hi, f32x4);
    const bf16x4 lo = __builtin_convertvector(v - hf, bf16x4);
    char* base = reinterpret_cast<char*>(rowp) + seg * 8;
    *reinterpret_cast<bf16x4*>(base) = hi;
    *reinterpret_cast<bf16x4*>(base + 64) = lo;
  };
  auto store_tile = [&](int set, int buf) {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const f32x4 v = (okmask[set] & (1u << i)) ? ra[set][i] : zero4;
      if constexpr (SPLIT == 1)
        store_split(&As[buf][(srow + RPP * i) * LDK], v);
      else
        *reinterpret_cast<f32x4*>(&As[buf][(srow + RPP * i) * LDK + seg * 4]) = v;
    }
#pragma unroll
    for (int j = 0; j < BR; ++j) {
      const f32x4 v = (FAST || (okmask[set] & (1u << (8 + j)))) ? rb[set][j] : zero4;
      if constexpr (SPLIT == 1)
        store_split(&Bs[buf][(srow + RPP * j) * LDK], v);
      else
        *reinterpret_cast<f32x4*>(&Bs[buf][(srow + RPP * j) * LDK + seg * 4]) = v;
    }
  };

  const int frow = lane & (FR - 1);  // fragment row (A: pixel, B: channel)
  const int fk = (lane / FR) * 4;    // k offset of this lane group inside a GK-deep fragment group

  f32x4 fa[2][FM], fb[2][FN];  // fragment double buffer: group g+1 is read from LDS while group g's MFMAs run
  auto read_frags = [&](int buf, int g, int slot) {
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
      fa[slot][mi] = *reinterpret_cast<const f32x4*>(&As[buf][(wm * TM + mi * FR + frow) * LDK + g * GK + fk]);
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
      fb[slot][ni] = *reinterpret_cast<const f32x4*>(&Bs[buf][(wn * TN + ni * FR + frow) * LDK + g * GK + fk]);
  };
  auto mfma_group = [&](int slot) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
          if constexpr (FR == 32)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[slot][mi][j], fb[slot][ni][j], acc[mi][ni], 0, 0, 0);
          else
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[slot][mi][j], fb[slot][ni][j], acc[mi][ni], 0, 0, 0);
  };
  // SPLIT: the 16-byte fragment reads are the same four (FR 32) / two (FR 16) groups; group g < NG/2 holds the hi parts of
  // k-step g, group g + NG/2 the lo parts.  Per step: hi*hi + hi*lo + lo*hi (small terms first).
  auto mfma_bf16 = [&](const f32x4& a, const f32x4& b, AccT& c) {
    if constexpr (FR == 32)
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  };
  auto mfma_tile = [&](int buf) {
    if constexpr (SPLIT) {
      constexpr int NSTEP = NG / 2;
#pragma unroll
      for (int st = 0; st < NSTEP; ++st) {
        read_frags(buf, st, 0);            // hi
        read_frags(buf, st + NSTEP, 1);    // lo
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
          for (int ni = 0; ni < FN; ++ni) {
            mfma_bf16(fa[1][mi], fb[0][ni], acc[mi][ni]);
            mfma_bf16(fa[0][mi], fb[1][ni], acc[mi][ni]);
            mfma_bf16(fa[0][mi], fb[0][ni], acc[mi][ni]);
          }
      }
    } else {
      read_frags(buf, 0, 0);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) read_frags(buf, g + 1, (g + 1) & 1);
        mfma_group(g & 1);
      }
    }
  };
  // One k-tile t (straight-line, no conditionals): issue the loads of tile t+2 into register set `par`, run tile t's MFMAs
  // from LDS stage `rd`, then write tile t+1 (register set par^1, loaded during tile t-1) to stage `wr`.
  auto tile_step = [&](int par, int rd, int wr) {
    loader_next();
    load_tile(par);
    mfma_tile(rd);
    if constexpr (NSTAGE == 1) __syncthreads();  // single stage: everyone is done reading before it is overwritten
    store_tile(par ^ 1, wr);
    __syncthreads();
  };

  // prologue: tile 0 -> LDS stage 0; tile 1 in flight in register set 1
  loader_seek(kt0);
  load_tile(0);
  store_tile(0, 0);
  if (kt1 - kt0 > 1) {
    loader_next();
    load_tile(1);
  }
  __syncthreads();
#ifdef M2H_CLOCK_DIAG
  const unsigned long long dbg_t0 = __builtin_amdgcn_s_memtime(), dbg_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  {
    // all but the last tile; unrolled by two so that register sets and LDS stages are compile-time
    const int nfull = kt1 - kt0 - 1;
    int t = 0;
    for (; t + 1 < nfull; t += 2) {
      tile_step(0, 0, NSTAGE == 2 ? 1 : 0);
      tile_step(1, NSTAGE == 2 ? 1 : 0, 0);
    }
    if (t < nfull) {
      tile_step(0, 0, NSTAGE == 2 ? 1 : 0);
      mfma_tile(NSTAGE == 2 ? 1 : 0);
    } else {
      mfma_tile(0);
    }
  }
#ifdef M2H_CLOCK_DIAG
  if (tid == 0 && blockIdx.y == 0) {
    const unsigned bi = blockIdx.x + gridDim.x * blockIdx.z;
    if (bi < 8192) {
      g_clock_dbg[bi][0] = __builtin_amdgcn_s_memtime() - dbg_t0;
      const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
      g_clock_dbg[bi][1] = r1 - dbg_r0;
      g_clock_dbg[bi][2] = dbg_r0;
      g_clock_dbg[bi][3] = r1;
      unsigned hwid, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      g_clock_dbg[bi][4] = hwid;
      g_clock_dbg[bi][5] = xcc;
    }
  }
#endif

  if (p.S > 1) {
    // split-K: raw partial sums to the slab [phase][split][M][N]; BN/activation/store happen in the reduce kernel
    float* slab = p.ws + ((size_t)(phase * p.S + split) * p.M) * p.N;
    const int col = lane & (FR - 1);
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int m = m0 + wm * TM + mi * FR + row_of(e);
        if (m >= p.M) continue;
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          const int n = n0 + wn * TN + ni * FR + col;
          if (n < p.N) slab[(size_t)m * p.N + n] = acc[mi][ni][e];
        }
      }
    return;
  }

  // ---- fused epilogue ----
  fused_epilogue<BM, BN, WM, WN, FR, AccT, NSTAGE * BM * LDK * 4>(p, acc, &As[0][0], &Bs[0][0], ri_out, ri_bc, n0, tid);
}

// Split-K epilogue: sums the S partial slabs of one output element in a fixed order (deterministic) and applies the
// same fused epilogue as the main kernel.  One thread = one GEMM row x 4 consecutive channels.
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const IGemmP p) {
  const int N4 = p.N >> 2;
  const long total = (long)p.M * N4;
  const int phase = blockIdx.y;
  const int ph = p.convT ? (phase >> 1) : p.ph, pw = p.convT ? (phase & 1) : p.pw;
  const size_t plane = (size_t)p.Ho * p.Wo;
  const int Cc = p.N >> 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / N4);
    const int n = (int)(i - (long)m * N4) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < p.S; ++s) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p.ws + ((size_t)(phase * p.S + s) * p.M + m) * p.N + n);
      v += t;
    }
    int q, rr, b, out, bc;
    decode_row(p, m, ph, pw, q, rr, b, out, bc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x = v[j];
      if (p.cls_table != nullptr) x += p.cls_val[bc >> 4] * p.cls_table[(size_t)(bc & 15) * p.N + n + j];
      const float sc = p.scale != nullptr ? p.scale[n + j] : 1.f;
      const float sh = p.shift != nullptr ? p.shift[n + j] : 0.f;
      x = x * sc + sh;
      v[j] = x > 0.f ? x : x * p.slope;
    }
    if (p.out_mode == M2H_OUT_NHWC) {
      if (p.dst_split) {
        const bf16x4 hi = __builtin_convertvector(v, bf16x4);
        const f32x4 hf = __builtin_convertvector(hi, f32x4);
        const bf16x4 lo = __builtin_convertvector(v - hf, bf16x4);
        char* base = reinterpret_cast<char*>(p.dst + (size_t)out * p.ldc + (n & ~31)) + ((n & 31) >> 2) * 8;
        *reinterpret_cast<bf16x4*>(base) = hi;
        *reinterpret_cast<bf16x4*>(base + 64) = lo;
      } else {
        *reinterpret_cast<f32x4*>(p.dst + (size_t)out * p.ldc + n) = v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (n + j) >> 4, s = (n + j) & 15;
        p.dst[((size_t)out + (size_t)s * plane) * Cc + c] = v[j];
      }
    }
  }
}

// The same reduce for the headline's deep stages (m2h_tuning_set 42: -1 = the kernel above everywhere).  The kernel above keeps one
// 16-byte load in flight per thread (run-time S: every load waits behind the previous add) and decodes its row per item.  Here
//   - S is a template parameter (2, 3, 4, 8; 0 = run-time loop): all S slab loads of an item are issued before the first add;
//   - an item is VEC = 8 consecutive channels where N % 8 == 0 (two f32x4 loads per slab; split32: ONE 16-byte hi and ONE 16-byte lo
//     store), VEC = 4 otherwise;
//   - a block owns 256 >> tsh whole rows (1 << tsh threads per row, the power of two at or above min(N / VEC, 256)): threads
//     0 .. rows - 1 decode one row each into LDS while the first item's loads are in flight.
// Sum order (0 + s0 + s1 + ...), class plane, scale / shift, activation and the hi / lo split are those of the kernel above, bit for bit.
template <int SC, int VEC>
__global__ __launch_bounds__(256) void splitk_reduce_rows_kernel(const IGemmP p, const int tsh) {
  constexpr int Q = VEC / 4;
  constexpr int SMAX = SC > 0 ? SC : 1;
  __shared__ int r_out[256], r_bc[256];
  const int tid = threadIdx.x;
  const int tpr = 1 << tsh, rows = 256 >> tsh;
  const int ipr = p.N / VEC;
  const int phase = blockIdx.y;
  const int ph = p.convT ? (phase >> 1) : p.ph, pw = p.convT ? (phase & 1) : p.pw;
  const int r = tid >> tsh, c0 = tid & (tpr - 1);
  const int m = blockIdx.x * rows + r;
  const bool live = m < p.M;
  const size_t slab = (size_t)p.M * p.N;   // floats per slab
  const float* src = p.ws + ((size_t)phase * p.S * p.M + (live ? m : 0)) * p.N;
  auto ld = [&](const float* q) { return *reinterpret_cast<const f32x4*>(q); };
  f32x4 t[SMAX][Q], sc[Q], sh[Q];
  // an item's loads, all issued before anything waits: the S slab pieces and the channels' scale / shift as vectors (the kernel above
  // loads them channel by channel behind a test of the pointer each, one memory round trip per channel)
  auto load_item = [&](int c) {
    if constexpr (SC > 0) {
#pragma unroll
      for (int s = 0; s < SC; ++s)
#pragma unroll
        for (int h = 0; h < Q; ++h) t[s][h] = ld(src + (size_t)s * slab + c * VEC + 4 * h);
    }
    // (no scale / no shift: the loads re-read the item's first slab piece and a select at the use drops them -- no branch around a load)
    const float* scp = p.scale != nullptr ? p.scale + c * VEC : src + c * VEC;
    const float* shp = p.shift != nullptr ? p.shift + c * VEC : src + c * VEC;
#pragma unroll
    for (int h = 0; h < Q; ++h) {
      sc[h] = *reinterpret_cast<const f32x4*>(scp + 4 * h);
      sh[h] = *reinterpret_cast<const f32x4*>(shp + 4 * h);
    }
  };
  const bool first = live && c0 < ipr;
  if (first) load_item(c0);
  if (tid < rows) {
    const int mr = blockIdx.x * rows + tid;
    int q, rr, b, out = -1, bc = 0;
    if (mr < p.M) decode_row(p, mr, ph, pw, q, rr, b, out, bc);
    r_out[tid] = out;
    r_bc[tid] = bc;
  }
  __syncthreads();
  if (!live) return;
  const int out = r_out[r], bc = r_bc[r];
  const size_t plane = (size_t)p.Ho * p.Wo;
  const int Cc = p.N >> 4;
  for (int c = c0; c < ipr; c += tpr) {
    if (c != c0) load_item(c);
    const int n0 = c * VEC;
    f32x4 v[Q];
#pragma unroll
    for (int h = 0; h < Q; ++h) v[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (SC > 0) {
#pragma unroll
      for (int s = 0; s < SC; ++s)
#pragma unroll
        for (int h = 0; h < Q; ++h) v[h] += t[s][h];
    } else {
      for (int s = 0; s < p.S; ++s)
#pragma unroll
        for (int h = 0; h < Q; ++h) v[h] += ld(src + (size_t)s * slab + n0 + 4 * h);
    }
    if (p.cls_table != nullptr) {
      const float cv = p.cls_val[bc >> 4];
      f32x4 ct[Q];
#pragma unroll
      for (int h = 0; h < Q; ++h) ct[h] = *reinterpret_cast<const f32x4*>(p.cls_table + (size_t)(bc & 15) * p.N + n0 + 4 * h);
#pragma unroll
      for (int h = 0; h < Q; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[h][j] += cv * ct[h][j];
    }
#pragma unroll
    for (int h = 0; h < Q; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float x = v[h][j];
        x = x * (p.scale != nullptr ? sc[h][j] : 1.f) + (p.shift != nullptr ? sh[h][j] : 0.f);
        v[h][j] = x > 0.f ? x : x * p.slope;
      }
    if (p.out_mode == M2H_OUT_NHWC) {
      if (p.dst_split) {
        char* base = reinterpret_cast<char*>(p.dst + (size_t)out * p.ldc + (n0 & ~31)) + (n0 & 31) * 2;
        if constexpr (VEC == 8) {
          bf16x8 hi, lo;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bf16x4 hh = __builtin_convertvector(v[h], bf16x4);
            const bf16x4 ll = __builtin_convertvector(v[h] - __builtin_convertvector(hh, f32x4), bf16x4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              hi[4 * h + j] = hh[j];
              lo[4 * h + j] = ll[j];
            }
          }
          *reinterpret_cast<bf16x8*>(base) = hi;
          *reinterpret_cast<bf16x8*>(base + 64) = lo;
        } else {
          const bf16x4 hi = __builtin_convertvector(v[0], bf16x4);
          const bf16x4 lo = __builtin_convertvector(v[0] - __builtin_convertvector(hi, f32x4), bf16x4);
          *reinterpret_cast<bf16x4*>(base) = hi;
          *reinterpret_cast<bf16x4*>(base + 64) = lo;
        }
      } else {
#pragma unroll
        for (int h = 0; h < Q; ++h) *reinterpret_cast<f32x4*>(p.dst + (size_t)out * p.ldc + n0 + 4 * h) = v[h];
      }
    } else {
#pragma unroll
      for (int h = 0; h < Q; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + 4 * h + j;
          p.dst[((size_t)out + (size_t)(n & 15) * plane) * Cc + (n >> 4)] = v[h][j];
        }
    }
  }
}

template <int VEC>
static void launch_reduce_rows(const IGemmP& p, hipStream_t st) {
  const int ipr = p.N / VEC;
  int tsh = 0;
  while ((1 << tsh) < ipr && tsh < 8) ++tsh;
  const int rows = 256 >> tsh;
  const dim3 grid((unsigned)((p.M + rows - 1) / rows), p.convT ? 4 : 1), blk(256);
  switch (p.S) {
    case 2: M2H_LAUNCH((splitk_reduce_rows_kernel<2, VEC>), grid, blk, 0, st, p, tsh); break;
    case 3: M2H_LAUNCH((splitk_reduce_rows_kernel<3, VEC>), grid, blk, 0, st, p, tsh); break;
    case 4: M2H_LAUNCH((splitk_reduce_rows_kernel<4, VEC>), grid, blk, 0, st, p, tsh); break;
    case 8: M2H_LAUNCH((splitk_reduce_rows_kernel<8, VEC>), grid, blk, 0, st, p, tsh); break;
    default: M2H_LAUNCH((splitk_reduce_rows_kernel<0, VEC>), grid, blk, 0, st, p, tsh); break;
  }
}

// Tile choice: N picks the width; skinny M (rollout batches, GRU steps: weight-streaming bound, nothing to re-use along M)
// gets 32- or 64-row tiles so that four times as many blocks stream the weights.
void pick_tile(long M, int N, int& BM, int& BN) {
  BN = N > 64 ? 128 : (N > 32 ? 64 : (N > 16 ? 32 : 16));
  BM = 128;
  if (BN == 128) {
    if (M <= 32) BM = 32;
    else if (M <= 64) BM = 64;
  }
}

int splitk_for(long M, int N, int K, int phases, int BM, int BN) {
  if ((N & 3) != 0) return 1;
  const int nk = (K + BK - 1) / BK;
  const long mt = (M + BM - 1) / BM, ntl = (N + BN - 1) / BN;
  const long blocks = mt * ntl * phases;  // working blocks (padding blocks of the XCD map exit at once)
  long S = 1;
  // Fewer blocks than CUs: split K, aiming at two resident blocks per CU.  From one block per CU up the launch is left whole (round 4): at
  // 256-511 tiles a two-way split bought occupancy the layer did not need and paid a slab round trip plus a reduce launch for it
  // (the policy encoders at the 280-sample update batch, tools/enc_fwd_bench.py: conv 4x4/2 32 -> 64 forward 66 -> 50 us, the 3x3
  // conv's input gradient 49 -> 34 us).
  if (blocks < 256) S = (512 + blocks - 1) / blocks;
  // ... but keep enough k-tiles per split to amortise a block's fixed cost (row decode, cold first loads, slab write): measured
  // optimum at the rollout shapes (layer_bench --batch 14 --tm 32) is ~4 tiles for the MFMA-paced 128-row tile and ~16 for the
  // weight-streaming 32/64-row tiles (deeper splits made the 14-env U-Net pass 25 % slower)
  const long tmin = BM < 128 ? 16 : 4;
  if (S > nk / tmin) S = nk / tmin;
  return S < 1 ? 1 : (int)S;
}

int choose_splitk(const IGemmP& p, int BM, int BN, size_t ws_bytes) {
  if (p.ws == nullptr || g_force_splitk < 0 || (p.N & 3) != 0) return 1;
  const int phases = p.convT ? 4 : 1;
  const int Kw = p.fast_ok ? p.Kw : p.K;
  int S = splitk_for(p.M, p.N, Kw, phases, BM, BN);
  if (g_force_splitk > 0) {
    S = g_force_splitk;
    const int nk = (Kw + BK - 1) / BK;
    if (S > nk / 2) S = nk / 2;
  }
  while (S > 1 && (size_t)phases * S * p.M * p.N * sizeof(float) > ws_bytes) --S;
  return S < 1 ? 1 : S;
}

// Tail of a register-engine / LDS-DMA / shared-patch launch whose status is `rc`: with p.S > 1, the ordered reduce + epilogue over
// its split-K slabs (p.S per phase); `label` names the pair of launches for m2h_last_kernel
int finish_splitk(int rc, const IGemmP& p, hipStream_t st, const char* label) {
  if (rc != 0 || p.S == 1) return rc;
  const auto al16 = [](const void* q) { return (reinterpret_cast<size_t>(q) & 15) == 0; };
  // (the row-owning kernel reads scale / shift / class table as 16-byte vectors)
  if (g_splitk_rows >= 0 && al16(p.scale) && al16(p.shift) && al16(p.cls_table)) {
    // 16-byte pieces of the split32 row need what the fp32 row's f32x4 stores need already: ldc % 4 == 0 and a 16-byte aligned base
    const bool wide = p.N % 8 == 0 && (!p.dst_split || (p.ldc % 4 == 0 && al16(p.dst)));
    if (wide) launch_reduce_rows<8>(p, st);
    else launch_reduce_rows<4>(p, st);
  } else {
    const long total = (long)p.M * (p.N >> 2);
    long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    M2H_LAUNCH(splitk_epilogue_kernel, dim3((unsigned)g, p.convT ? 4 : 1), dim3(256), 0, st, p);
  }
  rc = launch_status("conv_igemm_f32 split-K epilogue");
  tl_last_launch = label;
  return rc;
}

// 256 x BN tile, 8 waves, two LDS stages, bf16x3 math on scalar-loader shapes only (no split-K: chosen when the tiles fill the chip).
// Wide N, enough work for one 256 x 128 tile per CU: eight waves (4 x 2 wave tiles of 64 x 64) share one staged
// pair of operand tiles.  The 128 x 128 kernel at two blocks per CU is bound by the chip's aggregate L2 -> LDS operand stream
// (PMC: ~8.5 TB/s of L2 reads with the matrix pipe 36 % and the LDS 39 % busy; one block per CU is only 7 % slower than two);
// the larger tile reads 384 operand rows per 256 x 128 outputs instead of 512.  (A 256 x 64 tile for the 64-wide first encoder
// stage measured slower: 252 vs 235 us.)
template <int BN>
static int launch_big(IGemmP& p, size_t ws_bytes, hipStream_t st) {
  constexpr int BM = 256;
  (void)ws_bytes;
  p.MT = (p.M + BM - 1) / BM;
  p.NT = (p.N + BN - 1) / BN;
  p.S = 1;
  const long mtpad = ((long)p.MT + 7) / 8 * 8;
  const long nblk = mtpad * p.NT;
  if (nblk * 4 > 0x7fffffffL) return fail(-1, "conv_igemm: grid too large (%ld blocks)", nblk);
  const int phases = p.convT ? 4 : 1;
  p.pmaj = p.convT ? 1 : 0;
  dim3 grid((unsigned)(p.pmaj ? nblk * 4 : nblk), 1, p.pmaj ? 1 : phases);
  if (p.presplit)
    M2H_LAUNCH((igemm_f32_kernel<BM, BN, 4, 2, 2, 32, 1, 2>), grid, dim3(512), 0, st, p);
  else
    M2H_LAUNCH((igemm_f32_kernel<BM, BN, 4, 2, 2, 32, 1, 1>), grid, dim3(512), 0, st, p);
  return launch_status("igemm_f32<256,128> (eight waves)");
}

template <int BM, int BN, int WM, int WN, int NSTAGE, int FR = 32>
static int launch_cfg(IGemmP& p, size_t ws_bytes, hipStream_t st) {
  const bool fast = p.fast_ok;
  p.MT = (p.M + BM - 1) / BM;
  p.NT = (p.N + BN - 1) / BN;
  p.S = choose_splitk(p, BM, BN, ws_bytes);
  const long mtpad = ((long)p.MT + 7) / 8 * 8;
  const long nblk = mtpad * p.NT;
  if (nblk > 0x7fffffffL) return fail(-1, "conv_igemm: grid too large (%ld blocks)", nblk);
  const int phases = p.convT ? 4 : 1;
  p.pmaj = (p.convT && nblk * 4 <= 0x7fffffffL) ? 1 : 0;   // (phases as grid z where the interleaved grid would overflow)
  dim3 grid((unsigned)(p.pmaj ? nblk * 4 : nblk), (unsigned)p.S, p.pmaj ? 1 : phases);
  const dim3 blk(64 * WM * WN);
  if (fast && p.math == 1 && p.presplit)
    M2H_LAUNCH((igemm_f32_kernel<BM, BN, WM, WN, NSTAGE, FR, 1, 2>), grid, blk, 0, st, p);
  else if (fast && p.math == 1)
    M2H_LAUNCH((igemm_f32_kernel<BM, BN, WM, WN, NSTAGE, FR, 1, 1>), grid, blk, 0, st, p);
  else if (fast)
    M2H_LAUNCH((igemm_f32_kernel<BM, BN, WM, WN, NSTAGE, FR, 1>), grid, blk, 0, st, p);
  else
    M2H_LAUNCH((igemm_f32_kernel<BM, BN, WM, WN, NSTAGE, FR, 0>), grid, blk, 0, st, p);
  static const std::string label = "igemm_f32<" + std::to_string(BM) + "," + std::to_string(BN) + ">";   // one per instantiation
  static const std::string label_sk = label + " + split-K reduce";
  return finish_splitk(launch_status(label.c_str()), p, st, label_sk.c_str());
}

#ifdef M2H_CLOCK_DIAG
extern "C" int m2h_diag_read_clocks(unsigned long long* host_out, int nblocks) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_clock_dbg), (size_t)nblocks * 6 * sizeof(unsigned long long));
}
#endif

// The register engine takes every launch the engines before it in conv_igemm_f32's list left: the eight-wave 256 x 128 tile from a
// chip's worth of tiles in bf16x3 math, the pick_tile ladder otherwise.
int launch_igemm_reg(IGemmP& p, size_t ws_bytes, hipStream_t st) {
  if (p.math == 1 && p.fast_ok && p.N % 128 == 0 && g_force_splitk <= 0) {
    const long tiles = (((long)p.M + 255) / 256) * (p.N / 128) * (p.convT ? 4 : 1);
    if (tiles >= CHIP_TILES) return launch_big<128>(p, ws_bytes, st);
  }
  int BM, BN;
  pick_tile(p.M, p.N, BM, BN);
  if (BM == 32) return launch_cfg<32, 128, 1, 4, 2>(p, ws_bytes, st);
  if (BM == 64) return launch_cfg<64, 128, 2, 2, 2>(p, ws_bytes, st);
  if (p.N > 64) return launch_cfg<128, 128, 2, 2, 2>(p, ws_bytes, st);
  // narrow-N tiles: one LDS stage doubles the resident blocks; measured better on every 64- and 32-wide layer once the loader
  // became scalar (layer_bench.py: down0 345 vs 382 us, up3 588 vs 618 us)
  if (p.N > 32) return launch_cfg<128, 64, 2, 2, 1>(p, ws_bytes, st);
  if (p.N > 16) return launch_cfg<128, 32, 4, 1, 1>(p, ws_bytes, st);
  return launch_cfg<128, 16, 4, 1, 1, 16>(p, ws_bytes, st);  // 16-wide MFMA: no half-empty tile
}

}  // namespace m2h
