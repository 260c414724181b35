"""The Auralizer's three kernels (TEST INFRASTRUCTURE): csrc/render.hip render_spectra, render_frames, render_mix and their chain,
Auralizer.render -- the table of test rows per family, the cells the rows must reach, seeded inputs, the float64 reference of every output
with its element-wise error scale, float32 numpy restatements of each kernel's algorithm in the kernel's own order, named mutants of those
restatements, and the restated launch geometry.

tests/test_gpu_render_kernels.py runs every row through the C entry point m2h/audio/render.py itself calls against ``reference``;
tests/test_render_kernels_cpu.py checks without a GPU that the rows reach every cell, that every restatement stays inside an eighth of its
(family, kind)'s tau on every row, that every mutant leaves the bound on the rows named for it (by MIN_MARGIN at the least), that the
composed restatement (spectra -> frames -> mix) is inside the chain's tau, and that the restated geometry is the source's.

Rules (tests/train_kernels.py's, as tests/separator_kernels.py states them).  Checks are LOCAL: every kernel is referenced in float64 from
the float32 values it was handed -- the frames rows are handed float32 spectra built on the CPU (a float64 rfft, put in the kernel's slot
layout and rounded), the mix rows float32 frame buffers of seeded noise -- so an error is charged to the kernel that made it and any window
the entry point admits can be posed.  NO ELEMENT IS LEFT OUT: every output buffer is NaN before the call, every element is compared, and an
element outside the window must still be NaN.  Input buffers hold NaN wherever the window does not make the kernel read: source samples of
blocks before first_block, RIRs before the base pointer's k0, spectra a window holds that no frame reads, and every frame sample (not only
the unread halves) that no output block of the window reads.

The packed transform is the feeder's: load_packed, fft_dif, ifft_dit, bit_rev, twiddles and the pair algebra (rfft_unpack, rfft_repack) are
imported from tests/feeder_kernels.py; the fixed-trip transforms of fft_lds.h perform the same operations per element in the same order.

Slot layout of a spectrum (M = 16384 complex slots): slot 0 {S[0], S[M]}, slot q = S[q] for 1 <= q <= M/2, conj(S[q]) for M/2 < q < M.

Scales
  spectra  Re and Im of every slot of a block: s = ||x_block||_2 (a bin is a mixed-sign sum of the block's samples times unit-modulus
           factors); the reference is numpy's float64 rfft at 32768 points.  A block of zeros asks for exact zeros (s = 0).
  frames   every one of the 32000 kept samples of frame m: s_m = sqrt(sum_p ||y_{m,p}||_2^2 / 32768), y_{m,p} the float64 inverse transform
           of the ONE product X_{m-p} (.) H_{kappa(m-p),p} of the float32 spectra as handed in (its norm by Parseval): the size of a
           transform's error, which spreads over all points alike, added in quadrature over the partitions.  Sample 31999 has reference
           ~ 0 and the same scale.
  mix      images = float32(a + b) of the two frame samples exactly (s = 0; one frame alone at o = 0 and o = F); mix: s =
           sqrt(sum_s (g_s v_s)^2) from the float32 image values, tau = TAU_FP32.
  chain    Auralizer.render against render_ref.render_f64: output block o of (r, s, ear) takes the quadrature sum of ||y_{j,p}||_2^2 / 32768
           over the products with j + p in {o, o - 1} (the two frames over it); the mixture sqrt(sum_s (g_s s_s)^2).

Kinds and taus.  tau of a (family, kind) = 8 x the ceiling the CPU test holds that kind's float32 restatement under (RESTATEMENT_WORST; the
measured worsts are in the header of tests/test_gpu_render_kernels.py); never the GPU's own number.
  spectra  noise / impulse at the row's last sample / dc (mean 20 sigma).  dc has a tau of its own: bin 0 of a DC-heavy block is
           sqrt(n) ||x||_2, 126 s at n = 16000, and its own float32 rounding alone is 126 x 6e-8 s = 7.5e-6 s.
  frames   noise / impulse.  The rows' last block is one sample and their last partition one tap, as the issue sets them, so the LAST frame of
           every such row (m = J + Pn - 2) is one sample times one tap: a constant spectrum, whose inverse transform is one non-zero sample.
           Against s = |y| / sqrt(32768) the coherent twiddle roundings of that transform stand sqrt(32768)-fold higher than against noise
           (the feeder's impulse rows, tests/feeder_kernels.py): those FRAMES (not their rows) are the kind "impulse" with a tau of their own;
           every other frame of the same row keeps the noise tau.
  mix      TAU_FP32, as the issue sets it.
  chain    noise / dc.

DEPARTURES from the issue and rows beyond it, each with its reason:
  frames   + frames.dense (J = Pn = 1, a full block times a full partition): the issue's J = Pn = 1 row is one sample times one tap, which
           leaves the densest single product (fftconv's 16000 x 16000) unseen at the kernel level.
           + a moving window row with kh0 = 1 > 0 (J = 5, frames 3..4, RIRs 1..4): the issue's slack row has kh0 = 0, where the mutant
           "kh0 ignored" is the restatement itself.
           + a moving window row whose buffers run past what its frames read (J = 5, frames 1..2, blocks and RIRs 0..4 held, 3 and 4 NaN):
           in the issue's windows nx and nh end at j_hi.
  mix      + L_out = 6: the issue's lengths give left = 1, 3 and 4 only (L_out mod 4), the cell list asks for left = 2 too.
           + the window that is block o = F alone (F = 2, L_out = 32005, blocks [2, 3), frame 1 only): in every wider window block F - 1
           reads the first half of frame F - 1, so only here is that half NaN while block F runs -- a kernel that multiplied the absent
           frame F by zero instead of not reading it (a hand plant, which every other row and test let through) leaves NaN here.
           NaN planting goes further than the two halves the issue names: every frame sample no output block of the window reads is NaN,
           the rest of a cut last block's frame among them (a quad's float4 load may cover up to three of those; they are never stored).
           "the o < F test dropped" reads frame F, which the buffer does not hold: the restatement addresses the flat buffer as the kernel
           does (the next (r, s)'s first frame, or ones past the end).

Worst restatement ratios (tests/test_render_kernels_cpu.py::test_zz_mutant_margins prints them): spectra noise 6.46e-7
(spectra.source.len16000.fb0.nblk1.outer1.noise), impulse 4.54e-7, dc 1.04e-5 (spectra.source.len15999.fb0.nblk1.outer3.dc); frames noise
3.00e-6 and impulse 8.95e-6 (both frames.whole.RS3.J3.Pn2: the noise worst is frame 2, one sample times the enveloped first partition plus a
block times one tap; a full block times a full partition, frames.dense, stands at 8.8e-7); mix 2.81e-7; chain noise 1.52e-6, dc 6.49e-7.

Mutant margins (worst |g - r| / (tau s) over a mutant's named rows, the smallest over those rows; inf = an exact or unwritten element
differs, or a value is not finite):
  spectra  upper slots unconjugated 2.9e+03, S[M] missing from slot 0 4.0e+01, slot M/2 left unwritten inf, last sample of an odd length
           dropped 8.6e+01, ear read at element stride 1 1.4e+05, first_block ignored inf (reads the NaN block), strides swapped 1.9e+03
  frames   kappa = m 8.4e+09, jx0 ignored 6.8e+06, kh0 ignored inf, last partition dropped 2.3e+06, p_lo = 0 always 8.3e+09, the k = M/2
           pair skipped 1.4e+02, DC and Nyquist products swapped 3.7e+02, ears swapped 2.8e+05, scale 1 / (2M) 1.1e+05
  mix      earlier frame at i 3.2e+10, one gain for every source 8.7e+04, the other four inf
"""
import numpy as np

import render_ref as REF
from elem_bound import TAU_FP32
from feeder_kernels import _cmul, bit_rev, fft_dif, ifft_dit, load_packed, rfft_repack, rfft_unpack, twiddles
from separator_kernels import check  # noqa: F401  (NaN where the reference is NaN, the element bound elsewhere, the count compared)
from train_kernels import F32, cdiv, seed_of

# ---- the restated geometry of csrc/render.hip (tests/test_render_kernels_cpu.py holds it against the source)
B, LOGM, RMAXP = 16000, 14, 16
M = 1 << LOGM
NFFT, FRAME = 2 * M, 2 * B
TRANSFORM_BLOCK, MIX_BLOCK = 1024, 256
PAIRS_PER_THREAD, GROUP = M // 2 // TRANSFORM_BLOCK, 4

FAMILIES = ("spectra", "frames", "mix", "chain")
MIN_MARGIN = 4.0
# ceilings of the worst restatement ratio per (family, kind) against the float64 reference, held by the CPU test; tau = 8 x the ceiling
RESTATEMENT_WORST = {("spectra", "noise"): 7e-7, ("spectra", "impulse"): 5e-7, ("spectra", "dc"): 1.2e-5,
                     ("frames", "noise"): 3.5e-6, ("frames", "impulse"): 1e-5,
                     ("chain", "noise"): 1.8e-6, ("chain", "dc"): 8e-7}
TAU = {k: 8 * v for k, v in RESTATEMENT_WORST.items()}
TAU[("mix", "noise")] = TAU_FP32
RESTATEMENT_WORST[("mix", "noise")] = TAU_FP32 / 8

_TW = twiddles(NFFT)
_K = np.arange(1, M // 2 + 1)
_IK, _IM = bit_rev(_K, LOGM), bit_rev(M - _K, LOGM)
_TR, _TI = _TW[_K, 0], _TW[_K, 1]


def _rng(row):
    return np.random.default_rng(seed_of(row["id"]))


def tau_of(family, kind):
    return TAU[(family, kind)]


def envelope(Lr):
    """60 dB from the first tap to the last."""
    return 10.0 ** (-3.0 * np.arange(Lr) / max(Lr - 1, 1))


def fma(a, b, c):
    """fmaf: the product of two float32 values is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def to_slots(S):
    """rfft bins [..., M + 1] -> the kernel's slots [..., M] (complex)."""
    out = np.empty(S.shape[:-1] + (M,), dtype=S.dtype)
    out[..., 0] = S[..., 0].real + 1j * S[..., M].real
    out[..., 1:M // 2 + 1] = S[..., 1:M // 2 + 1]
    out[..., M // 2 + 1:] = np.conj(S[..., M // 2 + 1:M])
    return out


def from_slots(Z):
    out = np.empty(Z.shape[:-1] + (M + 1,), dtype=Z.dtype)
    out[..., 0], out[..., M] = Z[..., 0].real, Z[..., 0].imag
    out[..., 1:M // 2 + 1] = Z[..., 1:M // 2 + 1]
    out[..., M // 2 + 1:M] = np.conj(Z[..., M // 2 + 1:])
    return out


def pairs32(Z):
    """complex [...] -> float32 [..., 2]"""
    return np.stack((Z.real, Z.imag), -1).astype(F32)


def cplx64(a):
    """float32 [..., 2] -> complex128 [...]"""
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def energy(Y):
    """||irfft(Y, 32768)||_2^2 of bins [..., M + 1], by Parseval."""
    a = (Y.real ** 2 + Y.imag ** 2)
    return (a[..., 0] + a[..., M] + 2.0 * a[..., 1:M].sum(-1)) / NFFT


def _fetch(flat, idx):
    """flat[idx], ones past the end: what a mutant reads outside the buffer."""
    ok = idx < flat.size
    return np.where(ok, flat[np.minimum(idx, flat.size - 1)], F32(1.0))


# ----------------------------------------------------------------------------------------------------------------------------------
# spectra (render_spectra_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
SPECTRA_MUTANTS = ("upper slots unconjugated", "S[M] missing from slot 0", "slot M/2 left unwritten", "last sample of an odd length dropped",
                   "ear read at element stride 1", "first_block ignored", "mid and inner strides swapped")
KINDS = ("noise", "impulse", "dc")
SPECTRA_SOURCE = ((1, 0, 1, 1), (15999, 0, 1, 3), (16000, 0, 1, 1), (16001, 1, 1, 3), (40001, 0, 3, 1), (40001, 1, 2, 3))      # row_len, first_block, nblk, n_outer
SPECTRA_RIR = ((1, 1, 0, 1), (700, 1, 0, 1), (16001, 1, 0, 1), (33000, 1, 0, 1), (700, 3, 1, 2), (16001, 3, 1, 2))               # Lr, K, k0, n_mid
SPECTRA_RS = 2


def _spectra_rows():
    R = []
    for row_len, fb, nblk, n_outer in SPECTRA_SOURCE:
        for kind in KINDS:
            R.append(dict(id="spectra.source.len%d.fb%d.nblk%d.outer%d.%s" % (row_len, fb, nblk, n_outer, kind), family="spectra", form="source", kind=kind,
                          row_len=row_len, first_block=fb, nblk=nblk, n_outer=n_outer, n_mid=1, n_inner=1, es=1, K=1, k0=0))
    for Lr, K, k0, n_mid in SPECTRA_RIR:
        for kind in KINDS:
            R.append(dict(id="spectra.rir.Lr%d.K%d.k%d.mid%d.%s" % (Lr, K, k0, n_mid, kind), family="spectra", form="rir", kind=kind, row_len=Lr, first_block=0,
                          nblk=cdiv(Lr, B), n_outer=SPECTRA_RS, n_mid=n_mid, n_inner=2, es=2, K=K, k0=k0))
    return R


SPECTRA_ROWS = _spectra_rows()


def spectra_args(row):
    """(offset of the base pointer in floats, the entry point's integer arguments after the three pointers)"""
    L = row["row_len"]
    if row["form"] == "source":
        return 0, (row["n_outer"], 1, 1, L, 0, 0, L, 1, row["first_block"], row["nblk"])
    return row["k0"] * L * 2, (row["n_outer"], row["n_mid"], 2, row["K"] * L * 2, L * 2, 1, L, 2, 0, row["nblk"])


def spectra_grid(row):
    return (row["nblk"], row["n_mid"] * row["n_inner"], row["n_outer"]), TRANSFORM_BLOCK


def block_lengths(row):
    return [min(B, row["row_len"] - (row["first_block"] + b) * B) for b in range(row["nblk"])]


def _shows_phase(row):
    """Some block's spectrum is not real: a sample that is not zero at a position other than 0."""
    n = block_lengths(row)
    return n[-1] > 1 if row["kind"] == "impulse" else max(n) > 1


def spectra_cells(row):
    n = block_lengths(row)
    out = {(row["kind"], row["form"]), "n_outer = 1" if row["n_outer"] == 1 else "n_outer > 1"}
    out |= {"odd n" if v % 2 else "even n" for v in n}
    if 1 in n:
        out.add("n = 1")
    if B in n:
        out.add("n = B")
    if row["first_block"] > 0:
        out.add("first_block > 0")
    if row["nblk"] > 1:
        out.add("nblk > 1")
    if row["k0"] > 0:
        out.add("base pointer at k0 > 0")
    if row["form"] == "rir" and row["nblk"] > 1 and n[-1] == 1:
        out.add("one-tap partition")
    return out


def spectra_all_cells():
    return ({(k, f) for k in KINDS for f in ("source", "rir")} |
            {"n_outer = 1", "n_outer > 1", "odd n", "even n", "n = 1", "n = B", "first_block > 0", "nblk > 1", "base pointer at k0 > 0", "one-tap partition"})


def signal(g, kind, shape, env=None):
    """[..., n] float64: noise of sigma 0.1, one impulse at the last sample, or noise on a mean of 20 sigma -- under `env` where given."""
    if kind == "impulse":
        x = np.zeros(shape)
        x[..., -1] = 0.04 - 0.07 * (np.arange(x[..., -1].size).reshape(x[..., -1].shape) % 2)
        return x
    x = 0.1 * g.standard_normal(shape) + (2.0 if kind == "dc" else 0.0)
    return x if env is None else x * env


def spectra_inputs(row):
    g = _rng(row)
    L = row["row_len"]
    if row["form"] == "source":
        x = signal(g, row["kind"], (row["n_outer"], L)).astype(F32)
        x[:, :row["first_block"] * B] = np.nan                   # blocks before the window: not the kernel's to read
    else:
        x = np.moveaxis(signal(g, row["kind"], (row["n_outer"], row["K"], 2, L), envelope(L)), -2, -1).astype(F32)      # [RS, K, Lr, 2]
        x[:, :row["k0"]] = np.nan                                # RIRs before the base pointer
        x = np.ascontiguousarray(x)
    return dict(x=x)


def _spectra_blocks(row, inp, mutant=None, dtype=F32):
    """The samples the kernel loads: [n_outer, n_mid n_inner, nblk, B], zero from a block's n on, by the kernel's own address arithmetic."""
    off, (n_outer, n_mid, n_inner, os_, ms, is_, L, es, fb, nblk) = spectra_args(row)
    if mutant == SPECTRA_MUTANTS[4]:
        es = 1
    if mutant == SPECTRA_MUTANTS[5]:
        fb = 0
    if mutant == SPECTRA_MUTANTS[6]:
        ms, is_ = is_, ms
    flat = inp["x"].reshape(-1)
    o, c, b, t = np.ix_(np.arange(n_outer), np.arange(n_mid * n_inner), np.arange(nblk), np.arange(B))
    a = (fb + b) * B
    n = np.minimum(L - a, B)
    if mutant == SPECTRA_MUTANTS[3]:
        n = n - n % 2
    idx = off + o * os_ + (c // n_inner) * ms + (c % n_inner) * is_ + (a + t) * es
    return np.where(t < n, _fetch(flat, np.where(t < n, idx, 0)), F32(0.0)).astype(dtype)


def spectra_reference(row, inp):
    x = _spectra_blocks(row, inp, dtype=np.float64)
    Z = to_slots(np.fft.rfft(x, NFFT))
    r = np.stack((Z.real, Z.imag), -1)
    s = np.sqrt((x * x).sum(-1))[..., None, None]
    return {"spec": (r, np.broadcast_to(s, r.shape).copy())}


def spectrum_fp32(blocks, mutant=None):
    """[..., B] float32 -> the kernel's slots [..., M, 2]: packed load, decimation in frequency, the pair-wise unpack."""
    zr, zi = fft_dif(*load_packed(np.ascontiguousarray(blocks), M), _TW, LOGM)
    out = np.full(zr.shape + (2,), np.nan, dtype=F32)
    z0r, z0i = zr[..., 0], zi[..., 0]
    out[..., 0, 0] = z0r + z0i
    out[..., 0, 1] = 0 if mutant == SPECTRA_MUTANTS[1] else z0r - z0i
    er, ei, tor, toi = rfft_unpack(_TR, _TI, zr[..., _IK], zi[..., _IK], zr[..., _IM], zi[..., _IM])
    last = -1 if mutant == SPECTRA_MUTANTS[2] else None
    lo = slice(0, -1)                                                  # k < M/2: slot M - k
    sgn = F32(-1.0) if mutant == SPECTRA_MUTANTS[0] else F32(1.0)
    out[..., M - _K[lo], 0], out[..., M - _K[lo], 1] = (er - tor)[..., lo], sgn * (ei - toi)[..., lo]
    out[..., _K[:last], 0], out[..., _K[:last], 1] = (er + tor)[..., :last], (ei + toi)[..., :last]
    return out


def spectra_fp32(row, inp, mutant=None):
    with np.errstate(invalid="ignore"):
        return {"spec": spectrum_fp32(_spectra_blocks(row, inp, mutant), mutant)}


# ----------------------------------------------------------------------------------------------------------------------------------
# frames (render_frames_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
FRAMES_MUTANTS = ("kappa = the frame index m", "jx0 ignored", "kh0 ignored", "last partition dropped", "p_lo = 0 always (clamped index)",
                  "the k = M/2 pair skipped", "DC and Nyquist products swapped", "ears swapped", "scale 1 / (2M)")


def _frames_row(name, RS, J, Pn, K, m0, nm, jx0, nx, kh0, nh, dense=False):
    return dict(id="frames.%s.RS%d.J%d.Pn%d.K%d.m%d+%d.x%d+%d.h%d+%d" % (name, RS, J, Pn, K, m0, nm, jx0, nx, kh0, nh), family="frames", RS=RS, J=J, Pn=Pn, K=K,
                m0=m0, nm=nm, jx0=jx0, nx=nx, kh0=kh0, nh=nh, dense=dense)


def _plan_rows(J, Pn, K, RS):
    from m2h.audio.render import render_plan
    plan = render_plan((J - 1) * B + 1, (Pn - 1) * B + 1, K, 1, tail=True)
    return [_frames_row("plan%d" % i, RS, J, Pn, K, ch["frames"][0], ch["frames"][1] - ch["frames"][0], ch["x"][0], ch["x"][1] - ch["x"][0], ch["h"][0],
                        ch["h"][1] - ch["h"][0]) for i, ch in enumerate(plan["chunks"])]


FRAMES_ROWS = ([_frames_row("one", 1, 1, 1, 1, 0, 1, 0, 1, 0, 1), _frames_row("dense", 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, dense=True),
                _frames_row("whole", 3, 3, 2, 1, 0, 4, 0, 3, 0, 1)] + _plan_rows(3, 2, 1, 2) +
               [_frames_row("slack", 2, 5, 2, 1, 3, 2, 1, 4, 0, 1), _frames_row("slack", 2, 5, 2, 5, 3, 2, 1, 4, 0, 5), _frames_row("slack", 2, 5, 2, 5, 3, 2, 2, 3, 1, 4),
                _frames_row("slack", 1, 5, 2, 5, 1, 2, 0, 5, 0, 5),
                _frames_row("short", 1, 1, 3, 1, 0, 3, 0, 1, 0, 1), _frames_row("moving", 2, 3, 3, 3, 0, 5, 0, 3, 0, 3),
                _frames_row("limit", 1, 2, 16, 1, 0, 17, 0, 2, 0, 1), _frames_row("limit", 1, 2, 16, 2, 0, 17, 0, 2, 0, 2)])


def frames_grid(row):
    return (row["nm"], row["RS"], 2), TRANSFORM_BLOCK


def frames_reads(row):
    """[(m, [(p, j) ...]) ...] of the window's frames, and j_lo, j_hi as the entry point computes them."""
    J, Pn, m0, nm = row["J"], row["Pn"], row["m0"], row["nm"]
    fr = [(m, [(p, m - p) for p in range(max(m - (J - 1), 0), min(m, Pn - 1) + 1)]) for m in range(m0, m0 + nm)]
    return fr, max(m0 - (Pn - 1), 0), min(m0 + nm - 1, J - 1)


def frame_kind(row, m):
    return "impulse" if not row["dense"] and m == row["J"] + row["Pn"] - 2 else "noise"


def frames_cells(row):
    fr, j_lo, j_hi = frames_reads(row)
    J, Pn = row["J"], row["Pn"]
    moving = row["K"] != 1
    out = {"moving" if moving else "static", "RS > 1" if row["RS"] > 1 else "RS = 1", "m0 > 0" if row["m0"] > 0 else "m0 = 0"}
    out |= {"a frame of kind " + frame_kind(row, m) for m, _ in fr}
    if any(m - (J - 1) > 0 for m, _ in fr):
        out.add("p_lo > 0")
    if any(m < Pn - 1 for m, _ in fr):
        out.add("p_hi < Pn - 1")
    if J < Pn:
        out.add("J < Pn")
    if Pn == RMAXP:
        out.add("Pn = 16")
    if row["jx0"] < j_lo:
        out.add("slack in jx0")
    if row["jx0"] + row["nx"] - 1 > j_hi:
        out.add("slack in nx")
    if moving and row["kh0"] < j_lo:
        out.add("slack in kh0" if row["kh0"] == 0 else "slack in kh0, kh0 > 0")
    if row["dense"]:
        out.add("a full block times a full partition")
    return out


def frames_all_cells():
    return {"moving", "static", "RS > 1", "RS = 1", "m0 > 0", "m0 = 0", "a frame of kind noise", "a frame of kind impulse", "p_lo > 0", "p_hi < Pn - 1", "J < Pn",
            "Pn = 16", "slack in jx0", "slack in nx", "slack in kh0", "slack in kh0, kh0 > 0", "a full block times a full partition"}


def frames_inputs(row):
    """float32 spectra in the kernel's slot layout of noise blocks (last block one sample) and of noise RIRs under the 60 dB envelope (last
    partition one tap) -- a full block and a full partition in the dense row; NaN where the window holds a spectrum no frame reads."""
    g = _rng(row)
    RS, J, Pn, K, jx0, nx, kh0, nh = (row[k] for k in ("RS", "J", "Pn", "K", "jx0", "nx", "kh0", "nh"))
    L, Lr = (J * B, Pn * B) if row["dense"] else ((J - 1) * B + 1, (Pn - 1) * B + 1)
    x = np.zeros((RS, J * B))
    x[:, :L] = 0.1 * g.standard_normal((RS, L))
    h = np.zeros((RS, K, 2, Pn * B))
    h[..., :Lr] = g.standard_normal((RS, K, 2, Lr)) * envelope(Lr)
    fr, _, _ = frames_reads(row)
    xspec = np.full((RS, nx, M, 2), np.nan, dtype=F32)
    hspec = np.full((RS, nh, 2, Pn, M, 2), np.nan, dtype=F32)
    moving = K != 1
    for j in sorted({j for _, ps in fr for _, j in ps}):
        xspec[:, j - jx0] = pairs32(to_slots(np.fft.rfft(x[:, j * B:(j + 1) * B], NFFT)))
    for k, p in sorted({((j - kh0) if moving else 0, p) for _, ps in fr for p, j in ps}):
        hspec[:, k, :, p] = pairs32(to_slots(np.fft.rfft(h[:, k + kh0 if moving else 0, :, p * B:(p + 1) * B], NFFT)))
    return dict(xspec=xspec, hspec=hspec)


def frames_reference(row, inp):
    RS, K, jx0, kh0, nm, m0 = (row[k] for k in ("RS", "K", "jx0", "kh0", "nm", "m0"))
    moving = K != 1
    fr, _, _ = frames_reads(row)
    r, s = np.zeros((RS, nm, 2, FRAME)), np.zeros((RS, nm, 2, FRAME))
    cache = {}

    def bins(a, key):
        if key not in cache:
            cache[key] = from_slots(cplx64(a))
        return cache[key]
    for m, ps in fr:
        Y, E = 0.0, 0.0
        for p, j in ps:
            k = j - kh0 if moving else 0
            Yp = bins(inp["xspec"][:, j - jx0], ("x", j))[:, None] * bins(inp["hspec"][:, k, :, p], ("h", k, p))
            Y, E = Y + Yp, E + energy(Yp)
        r[:, m - m0] = np.fft.irfft(Y, NFFT)[..., :FRAME]
        s[:, m - m0] = np.sqrt(E / NFFT)[..., None]
    return {"frames": (r, s)}


def _take(a, i, axis=1):
    """a[:, i] or, outside the buffer, ones: what a mutant reads there."""
    return a[:, i] if 0 <= i < a.shape[axis] else np.ones_like(a[:, 0])


def frame_fp32(ps, get_x, get_h, mutant=None):
    """One frame for every (r s, ear): ps the (p, j) products in the kernel's order, get_x(j) -> [RS, M, 2], get_h(p, j) -> [RS, 2, M, 2].
    The slot-wise products summed in float32 (slot 0: the two real products by fmaf), the re-pack, decimation in time, the scale."""
    yr = yi = None
    for p, j in ps:
        X, H = get_x(j)[:, None], get_h(p, j)
        if mutant == FRAMES_MUTANTS[7]:
            H = H[:, ::-1]
        xr, xi, hr, hi = X[..., 0], X[..., 1], H[..., 0], H[..., 1]
        if yr is None:
            yr, yi = np.zeros(hr.shape, dtype=F32), np.zeros(hr.shape, dtype=F32)
        pr, pi = _cmul(xr, xi, hr, hi)
        y0r, y0i = fma(xr[..., 0], hr[..., 0], yr[..., 0]), fma(xi[..., 0], hi[..., 0], yi[..., 0])
        yr, yi = yr + pr, yi + pi
        yr[..., 0], yi[..., 0] = y0r, y0i
    zr, zi = np.zeros_like(yr), np.zeros_like(yi)
    y0, ym = (yi[..., 0], yr[..., 0]) if mutant == FRAMES_MUTANTS[6] else (yr[..., 0], yi[..., 0])
    half = F32(0.5)
    zr[..., 0], zi[..., 0] = half * (y0 + ym), half * (y0 - ym)
    ymr, ymi = yr[..., M - _K], yi[..., M - _K].copy()
    ymi[..., -1] = -ymi[..., -1]                                       # k = M/2 is its own partner: conj(Y[M/2])
    zkr, zki, zmr, zmi = rfft_repack(_TR, _TI, yr[..., _K], yi[..., _K], ymr, ymi)
    last = -1 if mutant == FRAMES_MUTANTS[5] else None
    zr[..., _IM[:-1]], zi[..., _IM[:-1]] = zmr[..., :-1], zmi[..., :-1]
    zr[..., _IK[:last]], zi[..., _IK[:last]] = zkr[..., :last], zki[..., :last]
    zr, zi = ifft_dit(zr, zi, _TW, LOGM)
    sc = F32(1.0) / F32(2 * M if mutant == FRAMES_MUTANTS[8] else M)
    return np.stack((zr * sc, zi * sc), -1).reshape(zr.shape[:-1] + (2 * M,))[..., :FRAME].astype(F32)


def frames_fp32(row, inp, mutant=None):
    RS, J, Pn, K, jx0, kh0, nm, m0 = (row[k] for k in ("RS", "J", "Pn", "K", "jx0", "kh0", "nm", "m0"))
    moving = K != 1
    xs, hs = inp["xspec"], inp["hspec"]
    out = np.empty((RS, nm, 2, FRAME), dtype=F32)
    jx = 0 if mutant == FRAMES_MUTANTS[1] else jx0
    kh = 0 if mutant == FRAMES_MUTANTS[2] else kh0
    with np.errstate(invalid="ignore"):
        for m in range(m0, m0 + nm):
            p_lo, p_hi = max(m - (J - 1), 0), min(m, Pn - 1)
            if mutant == FRAMES_MUTANTS[3]:
                p_hi = min(p_hi, Pn - 2)
            if mutant == FRAMES_MUTANTS[4]:
                p_lo = 0
            ps = [(p, min(m - p, J - 1)) for p in range(p_lo, p_hi + 1)]
            if not ps:
                ps = [(0, None)]                                       # (the last-partition mutant on a one-partition frame: nothing summed)
            def get_x(j):
                return np.zeros_like(xs[:, 0]) if j is None else _take(xs, j - jx)
            def get_h(p, j):
                if j is None:
                    return np.zeros_like(hs[:, 0, :, 0])
                kk = (m if mutant == FRAMES_MUTANTS[0] else j) - kh if moving else 0
                return _take(hs, kk)[:, :, p]
            out[:, m - m0] = frame_fp32(ps, get_x, get_h, mutant)
    return {"frames": out}


# ----------------------------------------------------------------------------------------------------------------------------------
# mix (render_mix_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
MIX_MUTANTS = ("the earlier frame read at i instead of B + i", "the o < F test dropped", "o - m0 offset ignored", "images carrying the gain",
               "one gain for every source", "the left < 4 tail not written")
MIX_GAINS = {1: ((-1.5,), (0.75,)), 3: ((0.7, 0.0, -1.5), (-0.25, 2.0, 0.0)), 6: ((0.7, 0.0, -1.5, 0.3, 1.0, -0.2), (-0.25, 2.0, 0.0, 0.5, -1.0, 0.1))}


def _mix_row(R, S, m0, nm, F, o0, o1, L_out, images, gains):
    return dict(id="mix.R%d.S%d.m%d+%d.F%d.o%d-%d.L%d.%s.%s" % (R, S, m0, nm, F, o0, o1, L_out, "images" if images else "noimages", gains), family="mix", R=R, S=S,
                m0=m0, nm=nm, F=F, o0=o0, o1=o1, L_out=L_out, images=images, gains=gains)


MIX_ROWS = [_mix_row(*a) for a in (
    (1, 1, 0, 1, 1, 0, 1, 1, True, "default"), (2, 3, 0, 1, 1, 0, 1, 5, False, "custom"), (1, 3, 0, 1, 1, 0, 1, 6, True, "custom"),
    (1, 6, 0, 1, 1, 0, 1, 15999, True, "default"), (2, 1, 0, 1, 1, 0, 1, 16000, False, "custom"), (1, 3, 0, 2, 2, 0, 2, 16001, True, "custom"),
    (2, 3, 0, 3, 3, 0, 3, 40001, True, "custom"), (1, 6, 0, 3, 3, 0, 3, 40004, True, "custom"), (2, 1, 0, 3, 3, 0, 3, 48000, False, "default"),
    (1, 3, 0, 2, 2, 0, 3, 32005, True, "custom"),
    (2, 3, 0, 2, 3, 1, 2, 40001, True, "custom"), (2, 3, 1, 2, 3, 2, 3, 40001, True, "default"), (2, 3, 0, 3, 3, 2, 3, 40001, True, "custom"),
    (1, 3, 0, 3, 3, 2, 3, 40001, False, "custom"), (1, 3, 1, 1, 2, 2, 3, 32005, True, "custom"))]


def mix_grid(row):
    quads = (row["o1"] - row["o0"]) * B // 4
    return (cdiv(quads, MIX_BLOCK), 2, row["R"]), MIX_BLOCK


def mix_window(row):
    """(f_lo, f_hi, first sample, one past the last sample written)"""
    o0, o1, F = row["o0"], row["o1"], row["F"]
    return max(o0 - 1, 0), min(o1 - 1, F - 1), o0 * B, min(o1 * B, row["L_out"])


def mix_gains(row):
    R, S = row["R"], row["S"]
    if row["gains"] == "default":
        return np.full((R, S), F32(1.0 / S), dtype=F32)
    return np.asarray(MIX_GAINS[S][:R], dtype=F32)


def mix_cells(row):
    f_lo, f_hi, n0, n1 = mix_window(row)
    L, F = row["L_out"], row["F"]
    out = {"S = %d" % row["S"], "R = %d" % row["R"], "images on" if row["images"] else "images off", "m0 tight" if row["m0"] == f_lo else "m0 slack",
           "gains " + row["gains"]}
    if n1 - n0 >= 4:      # whole quads: a 16-byte store where the (r, ear) row starts on 16 bytes -- every row, or one row in four
        out.add("vector store, every row aligned" if L % 4 == 0 else "scalar store: unaligned row")
    if n1 == L:
        out.add("left = %d" % (L % 4 or 4))
        if L % 4:
            out.add("scalar store: left < 4")
    for o in range(row["o0"], row["o1"]):
        out.add("o = 0" if o == 0 else "o = F" if o == F else "0 < o < F")
    return out


def mix_all_cells():
    return ({"S = 1", "S = 3", "S = 6", "R = 1", "R = 2", "images on", "images off", "m0 tight", "m0 slack", "gains default", "gains custom", "vector store, every row aligned",
             "scalar store: unaligned row", "scalar store: left < 4", "o = 0", "o = F", "0 < o < F"} | {"left = %d" % i for i in (1, 2, 3, 4)})


def mix_read_mask(row):
    """[nm, 2 B] bool: the frame samples some output block of the window reads."""
    m0, nm, F, L = row["m0"], row["nm"], row["F"], row["L_out"]
    read = np.zeros((nm, FRAME), dtype=bool)
    for o in range(row["o0"], row["o1"]):
        cnt = min(B, L - o * B)
        if o < F:
            read[o - m0, :cnt] = True
        if o >= 1:
            read[o - 1 - m0, B:B + cnt] = True
    return read


def mix_inputs(row):
    g = _rng(row)
    R, S, nm = row["R"], row["S"], row["nm"]
    fr = g.standard_normal((R * S, nm, 2, FRAME)).astype(F32)
    fr[:, ~mix_read_mask(row)[:, None, :].repeat(2, 1)] = np.nan
    return dict(frames=fr, gains=mix_gains(row))


def _mix_run(row, inp, dtype, mutant=None):
    R, S, m0, nm, F, L = (row[k] for k in ("R", "S", "m0", "nm", "F", "L_out"))
    flat = inp["frames"].reshape(-1)
    gains = inp["gains"]
    mix = np.full((R, 2, L), np.nan, dtype=dtype)
    images = np.full((R, S, 2, L), np.nan, dtype=dtype) if row["images"] else None
    q = np.full((R, 2, L), np.nan)                                     # sum (g v)^2
    mo = 0 if mutant == MIX_MUTANTS[2] else m0
    for o in range(row["o0"], row["o1"]):
        lo, hi = o * B, min((o + 1) * B, L)
        if mutant == MIX_MUTANTS[5] and hi == L:
            hi = L - L % 4
        i = np.arange(hi - lo)
        for r in range(R):
            for ear in range(2):
                acc, qq = np.zeros(hi - lo, dtype=dtype), np.zeros(hi - lo)
                for s in range(S):
                    base = ((r * S + s) * nm * 2 + ear) * FRAME
                    v = np.zeros(hi - lo, dtype=dtype)
                    if o < F or mutant == MIX_MUTANTS[1]:
                        v = _fetch(flat, base + (o - mo) * 2 * FRAME + i).astype(dtype)
                    if o >= 1:
                        v = v + _fetch(flat, base + (o - 1 - mo) * 2 * FRAME + (0 if mutant == MIX_MUTANTS[0] else B) + i).astype(dtype)
                    gs = gains[r, 0 if mutant == MIX_MUTANTS[4] else s]
                    if dtype == F32:
                        if images is not None:
                            images[r, s, ear, lo:hi] = gs * v if mutant == MIX_MUTANTS[3] else v
                        acc = fma(gs, v, acc)
                    else:
                        v = v.astype(F32).astype(np.float64)           # the float32 image value the kernel made
                        if images is not None:
                            images[r, s, ear, lo:hi] = v
                        acc = acc + float(gs) * v
                        qq = qq + (float(gs) * v) ** 2
                mix[r, ear, lo:hi], q[r, ear, lo:hi] = acc, qq
    return mix, images, q


def mix_reference(row, inp):
    mix, images, q = _mix_run(row, inp, np.float64)
    out = {"mix": (mix, np.sqrt(np.nan_to_num(q)))}
    if images is not None:
        out["images"] = (images, np.zeros(images.shape))
    return out


def mix_fp32(row, inp, mutant=None):
    with np.errstate(invalid="ignore"):
        mix, images, _ = _mix_run(row, inp, F32, mutant)
    return {"mix": mix, "images": images} if images is not None else {"mix": mix}


# ----------------------------------------------------------------------------------------------------------------------------------
# chain (Auralizer.render)
# ----------------------------------------------------------------------------------------------------------------------------------
CHAIN_R = 2
CHAIN_ROWS = ([dict(id="chain.S2.L40001.Lr33000.K%d.tail.mb%d.noise" % (K, mb), family="chain", S=2, L=40001, Lr=33000, K=K, tail=True, max_blocks=mb, kind="noise")
               for K in (1, 3) for mb in (1, 1024)] +
              [dict(id="chain.S1.L16001.Lr16001.K1.tail.mb1024.dc", family="chain", S=1, L=16001, Lr=16001, K=1, tail=True, max_blocks=1024, kind="dc")])
_CHAIN = {}


def chain_cells(row):
    return {("K = %d" % row["K"], "max_blocks = %d" % row["max_blocks"], row["kind"])}


def chain_all_cells():
    return {("K = %d" % K, "max_blocks = %d" % mb, "noise") for K in (1, 3) for mb in (1, 1024)} | {("K = 1", "max_blocks = 1024", "dc")}


def chain_key(row):
    return (row["S"], row["L"], row["Lr"], row["K"], row["tail"], row["kind"])


def chain_inputs(row):
    """Seeded by the case, not by max_blocks: the rows of one case share inputs, reference and restatement."""
    g = np.random.default_rng(seed_of("chain.%s" % (chain_key(row),)))
    S, L, Lr, K = row["S"], row["L"], row["Lr"], row["K"]
    x = signal(g, row["kind"], (CHAIN_R, S, L)).astype(F32)
    off = 1.0 if row["kind"] == "dc" else 0.0
    h = ((off + (0.05 if off else 1.0) * g.standard_normal((CHAIN_R, S, K, Lr, 2))) * envelope(Lr)[:, None]).astype(F32)
    gains = (np.asarray(MIX_GAINS[3], dtype=F32)[:, :S] if S > 1 else np.full((CHAIN_R, 1), F32(1.0), dtype=F32))
    return dict(sources=x, rirs=h, gains=gains)


def chain_reference(row, inp):
    """(cached per case) {"images": (r, s), "mix": (r, s)} from render_ref.render_f64."""
    key = ("ref",) + chain_key(row)
    if key in _CHAIN:
        return _CHAIN[key]
    x, h, gains = inp["sources"].astype(np.float64), inp["rirs"].astype(np.float64), inp["gains"].astype(np.float64)
    S, L, Lr, K = row["S"], row["L"], row["Lr"], row["K"]
    mix, images = REF.render_f64(x, h, gains=gains, tail=row["tail"])
    J, Pn = cdiv(L, B), cdiv(Lr, B)
    L_out = mix.shape[-1]
    O = cdiv(L_out, B)
    X = np.stack([np.fft.rfft(x[..., j * B:(j + 1) * B], NFFT) for j in range(J)], 2)                                     # [R, S, J, bins]
    H = np.stack([np.fft.rfft(np.moveaxis(h[..., p * B:(p + 1) * B, :], -1, -2), NFFT) for p in range(Pn)], 4)            # [R, S, K, 2, Pn, bins]
    e = np.zeros((CHAIN_R, S, 2, J + Pn))                                                                                  # per frame
    for j in range(J):
        for p in range(Pn):
            e[..., j + p] += energy(X[:, :, j, None] * H[:, :, 0 if K == 1 else j, :, p])
    s_img = np.zeros(images.shape)
    for o in range(O):
        s_img[..., o * B:(o + 1) * B] = np.sqrt((e[..., o] + (e[..., o - 1] if o >= 1 else 0.0)) / NFFT)[..., None]
    s_mix = np.sqrt(((gains[:, :, None, None] * s_img) ** 2).sum(1))
    _CHAIN[key] = {"images": (images, s_img), "mix": (mix, s_mix)}
    return _CHAIN[key]


def chain_fp32(row, inp):
    """(cached per case) the composed restatement: spectra -> frames -> mix, as one chunk (the arithmetic does not depend on the chunking)."""
    key = ("fp32",) + chain_key(row)
    if key in _CHAIN:
        return _CHAIN[key]
    x, h, gains = inp["sources"], inp["rirs"], inp["gains"]
    S, L, Lr, K = row["S"], row["L"], row["Lr"], row["K"]
    RS = CHAIN_R * S
    J, Pn = cdiv(L, B), cdiv(Lr, B)
    F = J + Pn - 1
    L_out = L + Lr - 1 if row["tail"] else L
    xb = np.zeros((RS, J * B), dtype=F32)
    xb[:, :L] = x.reshape(RS, L)
    hb = np.zeros((RS, K, 2, Pn * B), dtype=F32)
    hb[..., :Lr] = np.moveaxis(h.reshape(RS, K, Lr, 2), -1, -2)
    xs = spectrum_fp32(xb.reshape(RS, J, B))                           # [RS, J, M, 2]
    hs = spectrum_fp32(hb.reshape(RS, K, 2, Pn, B))                    # [RS, K, 2, Pn, M, 2]
    frames = np.empty((RS, F, 2, FRAME), dtype=F32)
    for m in range(F):
        ps = [(p, m - p) for p in range(max(m - (J - 1), 0), min(m, Pn - 1) + 1)]
        frames[:, m] = frame_fp32(ps, lambda j: xs[:, j], lambda p, j: hs[:, j if K != 1 else 0, :, p])
    mrow = dict(R=CHAIN_R, S=S, m0=0, nm=F, F=F, o0=0, o1=cdiv(L_out, B), L_out=L_out, images=True)
    _CHAIN[key] = mix_fp32(mrow, dict(frames=frames, gains=gains))
    return _CHAIN[key]


# ----------------------------------------------------------------------------------------------------------------------------------
# the families together
# ----------------------------------------------------------------------------------------------------------------------------------
ROWS = {"spectra": SPECTRA_ROWS, "frames": FRAMES_ROWS, "mix": MIX_ROWS, "chain": CHAIN_ROWS}
ROWS_BY_ID = {r["id"]: r for rows in ROWS.values() for r in rows}
CELLS = {"spectra": spectra_cells, "frames": frames_cells, "mix": mix_cells, "chain": chain_cells}
_ALL = {"spectra": spectra_all_cells, "frames": frames_all_cells, "mix": mix_all_cells, "chain": chain_all_cells}
INPUTS = {"spectra": spectra_inputs, "frames": frames_inputs, "mix": mix_inputs, "chain": chain_inputs}
REFERENCE = {"spectra": spectra_reference, "frames": frames_reference, "mix": mix_reference, "chain": chain_reference}
FP32 = {"spectra": spectra_fp32, "frames": frames_fp32, "mix": mix_fp32}


def cells(row):
    return CELLS[row["family"]](row)


def all_cells(family):
    return _ALL[family]()


def inputs(row):
    return INPUTS[row["family"]](row)


def reference(row, inp):
    """{output: (r, s)} in float64; NaN in r: the element is not the kernel's to write."""
    return REFERENCE[row["family"]](row, inp)


def kinds_of(row, name, shape):
    """{kind: index into the output `name` (a tuple for numpy) of the elements held to tau_of(family, kind)}: a frames row by frame, every
    other row as a whole."""
    if row["family"] == "frames":
        out = {}
        for mi in range(row["nm"]):
            out.setdefault(frame_kind(row, row["m0"] + mi), []).append(mi)
        return {k: (slice(None), v) for k, v in out.items()}
    return {row.get("kind", "noise"): (slice(None),)}


def compare(row, name, g, r, s):
    """-> {kind: (worst, scale, holds, count)} of one output, each kind's elements against its own tau."""
    return {kind: check(np.asarray(g)[ix], r[ix], s[ix], tau_of(row["family"], kind)) for kind, ix in kinds_of(row, name, np.shape(r)).items()}


def largest_buffer_bytes(row):
    f = row["family"]
    if f == "spectra":
        return 8 * M * row["n_outer"] * row["n_mid"] * row["n_inner"] * row["nblk"]
    if f == "frames":
        return max(8 * M * row["RS"] * row["nh"] * 2 * row["Pn"], 4 * row["RS"] * row["nm"] * 2 * FRAME)
    if f == "mix":
        return 4 * max(row["R"] * row["S"] * row["nm"] * 2 * FRAME, row["R"] * row["S"] * 2 * row["L_out"])
    return 8 * M * CHAIN_R * row["S"] * row["K"] * 2 * cdiv(row["Lr"], B)


def _frames_last_in_window(r):
    return r["m0"] + r["nm"] == r["J"] + r["Pn"] - 1


# (family, mutant) -> predicate on the row: the rows the bound must reject the mutant on
MUTANT_ROWS = {
    ("spectra", SPECTRA_MUTANTS[0]): _shows_phase,
    ("spectra", SPECTRA_MUTANTS[1]): lambda r: True,
    ("spectra", SPECTRA_MUTANTS[2]): lambda r: True,
    ("spectra", SPECTRA_MUTANTS[3]): lambda r: any(n % 2 for n in block_lengths(r)),
    ("spectra", SPECTRA_MUTANTS[4]): lambda r: r["form"] == "rir" and r["row_len"] > 1,
    ("spectra", SPECTRA_MUTANTS[5]): lambda r: r["first_block"] > 0,
    ("spectra", SPECTRA_MUTANTS[6]): lambda r: r["form"] == "rir",
    ("frames", FRAMES_MUTANTS[0]): lambda r: r["K"] != 1 and r["Pn"] > 2,      # (with two partitions the second is the one tap 60 dB down)
    ("frames", FRAMES_MUTANTS[1]): lambda r: r["jx0"] > 0,
    ("frames", FRAMES_MUTANTS[2]): lambda r: r["K"] != 1 and r["kh0"] > 0,
    # (the last partition's one tap lies 60 dB down: where a louder partition shares its frame it is worth little; the last frame holds it alone)
    ("frames", FRAMES_MUTANTS[3]): lambda r: r["Pn"] > 1 and _frames_last_in_window(r),
    ("frames", FRAMES_MUTANTS[4]): lambda r: "p_lo > 0" in frames_cells(r),
    ("frames", FRAMES_MUTANTS[5]): lambda r: True,
    # (one sample times one tap: both real bins of both spectra are the sample itself, and the two products are equal)
    ("frames", FRAMES_MUTANTS[6]): lambda r: not (r["J"] == 1 and r["Pn"] == 1 and not r["dense"]),
    ("frames", FRAMES_MUTANTS[7]): lambda r: True,
    ("frames", FRAMES_MUTANTS[8]): lambda r: True,
    ("mix", MIX_MUTANTS[0]): lambda r: r["o1"] > 1,
    ("mix", MIX_MUTANTS[1]): lambda r: r["o1"] - 1 == r["F"],
    ("mix", MIX_MUTANTS[2]): lambda r: r["m0"] > 0,
    ("mix", MIX_MUTANTS[3]): lambda r: r["images"] and bool((mix_gains(r) != 1).any()),
    ("mix", MIX_MUTANTS[4]): lambda r: r["S"] > 1 and r["gains"] == "custom",
    ("mix", MIX_MUTANTS[5]): lambda r: r["L_out"] % 4 != 0 and mix_window(r)[3] == r["L_out"],
}
