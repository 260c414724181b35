"""The audio feeder and the evaluation inverse transform (TEST INFRASTRUCTURE): csrc/stft.hip (stft_frames, stft_post, istft_pre, istft_ola,
feeder_round_mix, rms_normalize, bss_metrics), csrc/fftconv.hip with the any-block-size transforms of csrc/fft_lds.h, and the two
DFT-as-GEMM calls of m2h/audio/stft.py -- the table of test rows per family, the cells the rows must reach, seeded inputs, the float64
reference of every output with its element-wise error scale, float32 numpy restatements of each kernel's algorithm in the kernel's own
order, and named mutants of those restatements.

tests/test_gpu_feeder_kernels.py runs every row through the entry point the project itself uses against ``reference``;
tests/test_feeder_kernels_cpu.py checks without a GPU that the rows reach every cell, that every restatement stays inside half its
family's tau on every row, that every mutant leaves the bound on the rows named for it (by MIN_MARGIN at the least), and that the restated
launch geometry is the sources'.

Scales (the rule of tests/train_kernels.py; checks are LOCAL: every kernel is referenced in float64 from the float32 values it was handed):
  frames     exact (s = 0): one correctly rounded float32 product, zeros in [n_fft, ldf)
  dft        sqrt(sum t^2) over the products of a row of the transform
  post       |X|: |r| + u(m) / tau, u(m) = min(sqrt(FLUSH), FLUSH / m) -- re * re + im * im may lose up to FLUSH to underflow, which is worth
             u(m) to its square root (all of a magnitude below 4e-19, nothing of one above 1e-17); log1p: s(m) / (1 + m) + |r|; phase: |r|;
             mode 2: log1p of the EXACT fp16 value, s = |r|, left out where the float64 magnitude lies within TIE_WINDOW m + u(m) of an fp16
             rounding tie (tie rule 1).  TIE_WINDOW = 8 * 2^-24, four times the float32 error bound of sqrt(fl(fl(re^2) + fl(im^2))): the
             issue's window tau m with tau = TAU_FP32 would leave out 4 .. 8 % of a row (an fp16 ulp is 5e-4 .. 1e-3 of m), past the 1 % cap
             it sets itself; the narrower window leaves out about 0.14 % (0.196 % of a row at the most) and asks more of the kernel, not less.
  pre        |mag|; columns [2 nb, ldr) keep their sentinel (s = 0)
  ola        sqrt(sum (f w)^2) / wss + |r|; zero fill exact
  round_mix  exact: rint, wrap to int16, * 2^-15, then (mix + q) * scale as two correctly rounded operations (in float64, rounded twice)
  rms        |r|
  bss        function of sums, in dB: c sum rel(sigma) + |r|, c = 10 / ln 10, rel = s(sigma) / |sigma|; s(<s,s>) = sum t, s(<s,x>) = sum |t|,
             s(|d|^2) = sum d^2 + 2 sqrt(sum d^2 (|x| + |a s|)^2) -- the rounding of d = x - a s carries eps (|x| + |a s|), mixed in sign.
             Terms of second order in eps (the float32 means, the cast of alpha: the sums are stationary in both) are below 1e-9 of every
             sum on these rows and left out.  An output is held to the bound where the linearisation stands: tau s(sigma) <= 0.1 sigma for
             every sum under its logarithms; that fails on the L = 2 rows alone (two mean-free samples are collinear: |x - alpha s|^2 is
             rounding noise) and there for si_sdr / si_sdri only.  si_sir, si_sar and their improvements divide by rounding noise, in the
             reference as here: finite and si_sir > 60 dB is all that is asked of them, as in tests/test_gpu_eval_metrics.py.
  fftconv    every output of one (clip, ear) takes s = the rms of the float64 linear result over the L + Lr - 1 points it occupies (an
             FFT's rounding error does not stay with the element).  Where the result fills the transform this is the rms over the nfft
             circular points; a transform longer than needed adds zeros that shrink that rms -- 13-fold at 100 + 100 - 1 points in
             2^15 -- and not the error (the restatement sits at 8.5e-6 of the nfft rms there, at 6.7e-7 of this one).
             tau: MEASURED, 8 x the worst ratio of the packed float32 restatement (packed load, decimation in frequency, pair-wise unpack,
             product, re-pack, decimation in time) against np.convolve in float64, over the feeder-kind and DC-heavy rows and the two chain
             rows: worst 1.61e-6 (the chain's 16000 x 16000 convolutions; 1.54e-6 on fftconv.L16385.Lr16384.n15.feeder.CS6), held under
             1.625e-6 = tau / 8, tau = 1.3e-5.  The impulse rows have a tau of their own, 8 x 4e-5 = 3.2e-4 (worst 3.90e-5,
             fftconv.L16000.Lr16000.n15.impulse.CS6): the transform of one impulse is a pure tone in every bin, the roundings of the
             twiddles add coherently into a few spur samples, and against the rms of a result that is ONE non-zero sample (peak / sqrt(n))
             they stand sqrt(n)-fold higher than against the rms of noise; these rows are there for the structure (wrap, odd lengths, the
             ear stride: margins of 1e5 tau), not for the rounding.
  chain      per-source samples equal round(float64 convolution), wrapped and scaled, but where the float64 value lies within
             TAU["fftconv"] s of a half-integer: one LSB (tie rule 2); the mixture exact from the per-source values the kernel made.  The
             share within the window grows with the level: the chain rows' responses peak at 0.025, not the 0.05 of
             tests/test_gpu_feeder.py, which keeps the share at 0.83 % and 0.93 % (cap 2 %); the restatement flips 0.010 % and 0.018 %.

Left-out shares (conditions on the inputs, computed from the reference alone): tie rule 1 at most 0.196 % of a row
(post.B2.C3.T5.nb17.lds40.mode2.mag; cap 1 %), tie rule 2 at most 0.927 % (chain.L2049.Lr2000; cap 2 %).

Worst restatement ratios over each family's rows (tests/test_feeder_kernels_cpu.py::test_zz_mutant_margins prints them): frames and
round_mix exact, dft 2.6e-6, post 2.4e-7, pre 1.0e-7, ola 1.4e-7, rms 1.7e-7, bss 5.3e-8, fftconv 1.54e-6 (impulse rows 3.90e-5), chain
1.61e-6; every family but fftconv and chain keeps TAU_FP32 and its restatement TAU_FP32 / 2.

Mutant margins (worst |g - r| / (tau s) over a mutant's named rows, the smallest over those rows; inf = an exact output differs or a value
is not finite):
  frames     all four inf
  post       fp16 rounding after log1p inf (a planted subnormal's exact zero), c / t swapped 3.6e+05, Im read at lds / 2 inf, atan2(re, im) inf
  pre        channel ignored inf, sin / cos swapped 7.1e+04, row stride 2 nb inf
  ola        t1 unclamped 1.3e+05, n > n_fft as the break inf, no tiny test inf (one row), no trim 9.2e+06, last frame dropped 2.5e+04
  round_mix  all four inf
  rms        mean over n padded to 1024 6.0e+02, zero clip divided inf (one row)
  bss        channel sum for channel mean 1.0e+04, means kept 8.0e+04, tail dropped 1.9e+01, mono-mixture path halved 3.7e+03
  fftconv    rotated by one 1.8e+01, last sample of an odd length dropped 1.2e+01, k = M/2 skipped 9.4e+01, DC / Nyquist swapped 2.7e+02,
             ear stride 2.5e+02
"""
import itertools

import numpy as np
import torch

import train_kernels as K
from elem_bound import TAU_FP32
from train_kernels import FLUSH, F32, cdiv, enters_grid_stride_loop, grid_for, seed_of, wave_tree  # noqa: F401

FAMILIES = ("frames", "dft", "post", "pre", "ola", "round_mix", "rms", "bss", "fftconv", "chain")
TAU = {f: TAU_FP32 for f in FAMILIES}
# fftconv: 8 x the packed float32 restatement's worst ratio (module docstring); tests/test_feeder_kernels_cpu.py holds every row's ratio
# under the eighth.  The impulse rows have a tau of their own.
FFTCONV_RESTATEMENT_WORST = {"feeder": 1.625e-6, "dc": 1.625e-6, "impulse": 4e-5}
TAU["fftconv"] = TAU["chain"] = 8 * FFTCONV_RESTATEMENT_WORST["feeder"]
TAU_FFTCONV_IMPULSE = 8 * FFTCONV_RESTATEMENT_WORST["impulse"]
MIN_MARGIN = 4.0
LSQ_COND = 4.0
TIE_WINDOW = 8 * 2.0 ** -24
TIE1_CAP, TIE2_CAP = 0.01, 0.02
SENT = -7.25
BIG_BYTES = 4 << 20                         # "a few MB": only the grid-stride rows hold a buffer above it
# launch geometry restated (tests/test_feeder_kernels_cpu.py holds it against the sources)
SGRID_CAP, SGRID_BLOCK, CLIP_BLOCK, FFTCONV_BLOCK = 8192, 256, 1024, 1024
FFTCONV_LOG2N = (11, 12, 13, 14, 15)
N_METRICS = 11
WELL = (0, 3, 4, 5, 6, 7, 8)      # si_sdr, sd_sdr, snr, srr, si_sdri, sd_sdri, snri


def hann_periodic(n):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(F32)


def _rng(row):
    return np.random.default_rng(seed_of(row["id"]))


def tau_of(row):
    return TAU_FFTCONV_IMPULSE if row["family"] == "fftconv" and row["kind"] == "impulse" else TAU[row["family"]]


def second_trip(total):
    """A thread of an sgrid launch (blocks of 256, at most 8192 of them) takes a second element."""
    return enters_grid_stride_loop(total, SGRID_CAP)


def check(g, r, s, tau, skip=None):
    """(worst |g - r| / s, least-squares scale, holds) over the elements not in `skip`: train_kernels.check's element bound, its scale
    condition where the output is well conditioned (tests/rollout_kernels.py), and exact equality where the reference is not finite."""
    g, r, s = (np.asarray(t, dtype=np.float64).reshape(-1) for t in (g, r, np.broadcast_to(np.asarray(s, dtype=np.float64), np.shape(r))))
    keep = np.ones(r.shape, dtype=bool) if skip is None else ~np.asarray(skip).reshape(-1)
    g, r, s = g[keep], r[keep], s[keep]
    inf = ~np.isfinite(r)
    if not np.array_equal(g[inf], r[inf]) or not np.isfinite(g[~inf]).all():
        return float("inf"), float("nan"), False
    g, r, s = (torch.from_numpy(np.ascontiguousarray(t[~inf])) for t in (g, r, s))
    if r.numel() == 0:
        return 0.0, 1.0, True
    worst, scale, _ = K.check(g, r, s, tau)
    rr = float((r * r).sum())
    cond = float((s * r.abs()).sum()) / rr if rr > 0 else float("inf")
    return worst, scale, worst <= tau and (cond > LSQ_COND or abs(scale - 1.0) <= tau)


# ----------------------------------------------------------------------------------------------------------------------------------
# frames (stft.hip stft_frames_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
FRAMES_MUTANTS = ("reflection that repeats the edge sample", "right reflection 2L - idx", "pad rounded up", "zero tail omitted")


def frames_T(L, n_fft, hop):
    """STFT.__call__'s frame count."""
    return 1 + (L + 2 * (n_fft // 2) - n_fft) // hop


def _frames_row(n_fft, hop, ldf, L, S):
    return dict(id="frames.n%d.h%d.ld%d.L%d.S%d" % (n_fft, hop, ldf, L, S), family="frames", n_fft=n_fft, hop=hop, ldf=ldf, L=L, S=S, T=frames_T(L, n_fft, hop))


FRAMES_BIG_L = 32768 * 32 + 1       # T = 32769 frames of 64: S T ldf = 2^21 + 64
FRAMES_ROWS = [_frames_row(*a) for a in ((1023, 512, 1024, 16000, 3), (1023, 512, 1024, 512, 1), (1023, 512, 1024, 1535, 2), (1023, 512, 1056, 4000, 1),
                                         (1022, 512, 1024, 2048, 2), (31, 16, 32, 16, 3), (31, 16, 32, 17, 3), (31, 16, 32, 500, 3), (63, 32, 64, FRAMES_BIG_L, 1))]


def frames_reflects_right(row):
    return (row["T"] - 1) * row["hop"] + row["n_fft"] - 1 - row["n_fft"] // 2 >= row["L"]


def frames_cells(row):
    out = {"n_fft=%d" % row["n_fft"], "odd n_fft" if row["n_fft"] % 2 else "even n_fft", "ldf at its minimum" if row["ldf"] == (row["n_fft"] + 31) // 32 * 32 else "ldf above its minimum",
           "T=1" if row["T"] == 1 else "T>1", "S=1" if row["S"] == 1 else "S>1", "right reflection" if frames_reflects_right(row) else "no right reflection",
           "second trip of the grid-stride loop" if second_trip(row["S"] * row["T"] * row["ldf"]) else "one element per thread"}
    if row["L"] == row["n_fft"] // 2 + 1:
        out.add("L = pad + 1")
    if row["L"] % row["hop"]:
        out.add("L not a multiple of hop")
    return out


def frames_all_cells():
    return {"n_fft=1023", "n_fft=1022", "n_fft=31", "n_fft=63", "odd n_fft", "even n_fft", "ldf at its minimum", "ldf above its minimum", "T=1", "T>1", "S=1", "S>1",
            "right reflection", "no right reflection", "second trip of the grid-stride loop", "one element per thread", "L = pad + 1", "L not a multiple of hop"}


def frames_inputs(row):
    return dict(y=_rng(row).standard_normal((row["S"], row["L"])).astype(F32), window=hann_periodic(row["n_fft"]))


def _frames_index(row, mutant=None):
    n_fft, hop, L, T = row["n_fft"], row["hop"], row["L"], row["T"]
    pad = (n_fft + 1) // 2 if mutant == FRAMES_MUTANTS[2] else n_fft // 2
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :] - pad
    idx = np.where(idx < 0, -idx - 1 if mutant == FRAMES_MUTANTS[0] else -idx, idx)
    if mutant == FRAMES_MUTANTS[0]:
        hi = 2 * L - 1 - idx
    elif mutant == FRAMES_MUTANTS[1]:
        hi = np.minimum(2 * L - idx, L - 1)     # (index L itself would leave the clip)
    else:
        hi = 2 * (L - 1) - idx
    return np.where(idx >= L, hi, idx)


def frames_reference(row, inp):
    S, T, n_fft, ldf = row["S"], row["T"], row["n_fft"], row["ldf"]
    r = np.zeros((S, T, ldf))
    prod = inp["window"].astype(np.float64)[None, None, :] * inp["y"].astype(np.float64)[:, _frames_index(row)]     # exact in float64: 24 + 24 bits
    r[:, :, :n_fft] = prod.astype(F32)
    return {"frames": (r, 0.0)}


def frames_fp32(row, inp, mutant=None):
    S, T, n_fft, ldf = row["S"], row["T"], row["n_fft"], row["ldf"]
    out = np.full((S, T, ldf), SENT, dtype=F32)
    out[:, :, :n_fft] = inp["window"][None, None, :] * inp["y"][:, _frames_index(row, mutant)]
    if mutant != FRAMES_MUTANTS[3]:
        out[:, :, n_fft:] = 0
    return {"frames": out}


# ----------------------------------------------------------------------------------------------------------------------------------
# dft (ops.linear with STFT.W / ISTFT.W, default math mode)
# ----------------------------------------------------------------------------------------------------------------------------------
DFT_M = (1, 32, 33, 96)
DFT_ROWS = [dict(id="dft.%s.M%d" % (w, M), family="dft", which=w, M=M) for w in ("stft", "istft") for M in DFT_M]
_W = {}


def dft_weight(which):
    """The float32 matrix the project's own class builds (on the CPU here)."""
    if which not in _W:
        from m2h.audio.stft import ISTFT, STFT
        _W[which] = (STFT("cpu") if which == "stft" else ISTFT("cpu")).W.numpy()
    return _W[which]


def dft_cells(row):
    return {row["which"], "M=%d" % row["M"], (row["which"], "M=%d" % row["M"])}


def dft_all_cells():
    return {"stft", "istft"} | {"M=%d" % M for M in DFT_M} | {(w, "M=%d" % M) for w in ("stft", "istft") for M in DFT_M}


def dft_inputs(row):
    x = _rng(row).standard_normal((row["M"], 1024)).astype(F32)
    if row["which"] == "stft":
        x[:, :1023] *= hann_periodic(1023)      # windowed frames; column 1023 is the row's zero padding
        x[:, 1023] = 0
    return dict(x=x, W=dft_weight(row["which"]))


def dft_reference(row, inp):
    x, W = inp["x"].astype(np.float64), inp["W"].astype(np.float64)
    return {"y": (x @ W.T, np.sqrt((x * x) @ (W * W).T))}


def dft_fp32(row, inp, mutant=None):
    """(a plain float32 product: the engine's own k order is pinned by tests/forward_routes.py)"""
    return {"y": inp["x"] @ inp["W"].T}


# ----------------------------------------------------------------------------------------------------------------------------------
# post (stft.hip stft_post_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
POST_MUTANTS = ("fp16 rounding after log1p", "c / t swapped in the BHWC index", "Im read at lds / 2", "atan2(re, im)")
POST_SHAPES = ((3, 2, 32, 512, 1024), (1, 1, 1, 512, 1024), (2, 3, 5, 17, 40))
POST_BIG = (65, 2, 32, 512, 1024)
POST_OUTS = ("mag", "phase", "both")
# (re, im) planted at bins 0 .. 16 of the first frame of the first signal, and mirrored at the last bins of the last frame of the last signal
POST_PLANTS = ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 1.5), (-0.0, -2.5), (1.5, 0.0), (-2.0, 0.0), (-2.0, -0.0), (3e-8, 4e-8), (3e-6, -4e-6),
               (6e-5, 1e-5), (1e-4, 0.0), (60000.0, -40000.0), (65510.0, 0.0), (1e-20, -1e-21), (-1e-25, 1e-30))


def _post_row(shape, mode, outs):
    B, C, T, nb, lds = shape
    return dict(id="post.B%d.C%d.T%d.nb%d.lds%d.mode%d.%s" % (B, C, T, nb, lds, mode, outs), family="post", B=B, C=C, T=T, nb=nb, lds=lds, mode=mode, outs=outs)


POST_ROWS = [_post_row(sh, m, o) for sh in POST_SHAPES for m in (0, 1, 2) for o in POST_OUTS] + [_post_row(POST_BIG, 1, "both")]


def post_cells(row):
    shape = "B%d C%d T%d nb%d lds%d" % (row["B"], row["C"], row["T"], row["nb"], row["lds"])
    out = {shape, "second trip of the grid-stride loop" if second_trip(row["B"] * row["nb"] * row["T"] * row["C"]) else "one element per thread",
           "lds > 2 nb" if row["lds"] > 2 * row["nb"] else "lds = 2 nb"}
    if row["B"] <= 3:
        out.add((shape, "mode %d" % row["mode"], row["outs"]))
    return out


def post_all_cells():
    sh = ["B%d C%d T%d nb%d lds%d" % s for s in POST_SHAPES]
    return (set(sh) | {"B%d C%d T%d nb%d lds%d" % POST_BIG, "second trip of the grid-stride loop", "one element per thread", "lds > 2 nb", "lds = 2 nb"} |
            {(s, "mode %d" % m, o) for s in sh for m in (0, 1, 2) for o in POST_OUTS})


def post_inputs(row):
    B, C, T, nb, lds = (row[k] for k in ("B", "C", "T", "nb", "lds"))
    spec = np.full((B * C, T, lds), np.nan, dtype=F32)         # columns [2 nb, lds) are not the kernel's to read
    spec[:, :, :2 * nb] = _rng(row).standard_normal((B * C, T, 2 * nb)).astype(F32)
    for i, (re, im) in enumerate(POST_PLANTS):
        spec[0, 0, i], spec[0, 0, nb + i] = re, im
        if B * C * T > 1:
            spec[-1, -1, nb - 1 - i], spec[-1, -1, 2 * nb - 1 - i] = re, im
    return dict(spec=spec)


def _bhwc(a, row, swapped=False):
    """[B C, T, nb] -> [B, nb, T, C]"""
    a = a.reshape(row["B"], row["C"], row["T"], row["nb"])
    if swapped:      # MUTANT: [B, nb, C, T] behind the same shape
        return np.ascontiguousarray(a.transpose(0, 3, 1, 2)).reshape(row["B"], row["nb"], row["T"], row["C"])
    return np.ascontiguousarray(a.transpose(0, 3, 2, 1))


def underflow_slack(m):
    """What the loss of up to FLUSH from re * re + im * im is worth to its square root (nothing at an exact zero: nothing underflows)."""
    return np.where(m == 0, 0.0, np.minimum(np.sqrt(FLUSH), FLUSH / np.maximum(m, 1e-300)))


def fp16_near_tie(m, window):
    """The float64 magnitude lies within `window` of a value halfway between two fp16 neighbours (65520, below infinity, among them)."""
    fin = lambda a: np.where(np.isinf(a), 65536.0, a.astype(np.float64))      # noqa: E731
    with np.errstate(over="ignore"):
        h = m.astype(np.float16)
        lo, hi = fin(np.nextafter(h, np.float16(-np.inf))), fin(np.nextafter(h, np.float16(np.inf)))
    h64 = fin(h)
    hi = np.where(np.isinf(h), 2 * 65536.0, hi)
    return np.minimum(np.abs(m - (h64 + lo) / 2), np.abs(m - (h64 + hi) / 2)) <= window


def post_reference(row, inp, tau=None):
    tau = TAU["post"] if tau is None else tau
    nb = row["nb"]
    sp = inp["spec"].astype(np.float64)
    re, im = _bhwc(sp[:, :, :nb], row), _bhwc(sp[:, :, nb:2 * nb], row)
    m = np.hypot(re, im)
    s_m = m + underflow_slack(m) / tau
    out = {}
    if row["outs"] != "phase":
        if row["mode"] == 0:
            out["mag"] = (m, s_m)
        elif row["mode"] == 1:
            out["mag"] = (np.log1p(m), s_m / (1 + m) + np.log1p(m))
        else:
            with np.errstate(over="ignore"):
                r = np.log1p(m.astype(np.float16).astype(np.float64))
            out["mag"] = (r, np.where(np.isfinite(r), r, 0.0), fp16_near_tie(m, TIE_WINDOW * m + underflow_slack(m)))
    if row["outs"] != "mag":
        ph = np.arctan2(im, re)
        out["phase"] = (ph, np.abs(ph))
    return out


def post_fp32(row, inp, mutant=None):
    nb, lds = row["nb"], row["lds"]
    sp = inp["spec"]
    io = lds // 2 if mutant == POST_MUTANTS[2] else nb
    sw = mutant == POST_MUTANTS[1]
    re, im = _bhwc(sp[:, :, :nb], row, sw), _bhwc(sp[:, :, io:io + nb], row, sw)
    out = {}
    with np.errstate(all="ignore"):
        if row["outs"] != "phase":
            m = np.sqrt(re * re + im * im)
            if row["mode"] == 2 and mutant != POST_MUTANTS[0]:
                m = m.astype(np.float16).astype(F32)
            if row["mode"] >= 1:
                m = np.log1p(m)
            if row["mode"] == 2 and mutant == POST_MUTANTS[0]:
                m = m.astype(np.float16).astype(F32)
            out["mag"] = m.astype(F32)
        if row["outs"] != "mag":
            out["phase"] = (np.arctan2(re, im) if mutant == POST_MUTANTS[3] else np.arctan2(im, re)).astype(F32)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# pre (stft.hip istft_pre_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
PRE_MUTANTS = ("channel ignored", "sin / cos swapped", "row stride 2 nb")


def _pre_row(B, T, nb, ldr, C, c, wide=False):
    return dict(id="pre.B%d.T%d.nb%d.ldr%d.C%d.c%d%s" % (B, T, nb, ldr, C, c, ".wide" if wide else ""), family="pre", B=B, T=T, nb=nb, ldr=ldr, C=C, c=c, wide=wide)


PRE_ROWS = ([_pre_row(3, 32, 512, 1024, C, c) for C in (1, 2, 3) for c in range(C)] + [_pre_row(1, 1, 512, 1024, 1, 0)] +
            [_pre_row(2, 5, 17, 40, 3, c) for c in range(3)] + [_pre_row(3, 32, 512, 1024, 2, 1, wide=True)])


def pre_cells(row):
    return {("B%d T%d nb%d ldr%d" % (row["B"], row["T"], row["nb"], row["ldr"]), "C=%d" % row["C"], "c=%d" % row["c"]),
            "phases in [-8 pi, 8 pi]" if row["wide"] else "phases in [-pi, pi]", "ldr > 2 nb" if row["ldr"] > 2 * row["nb"] else "ldr = 2 nb"}


def pre_all_cells():
    out = {("B3 T32 nb512 ldr1024", "C=%d" % C, "c=%d" % c) for C in (1, 2, 3) for c in range(C)} | {("B1 T1 nb512 ldr1024", "C=1", "c=0")}
    out |= {("B2 T5 nb17 ldr40", "C=3", "c=%d" % c) for c in range(3)}
    return out | {"phases in [-8 pi, 8 pi]", "phases in [-pi, pi]", "ldr > 2 nb", "ldr = 2 nb"}


def pre_inputs(row):
    g = _rng(row)
    shape = (row["B"], row["nb"], row["T"], row["C"])
    mag = np.abs(g.standard_normal(shape)).astype(F32)
    mag[g.random(shape) < 0.02] = 0
    w = 8 * np.pi if row["wide"] else np.pi
    phase = g.uniform(-w, w, shape).astype(F32)
    phase.reshape(-1)[:4] = (0.0, np.pi, -np.pi, np.pi / 2)
    return dict(mag=mag, phase=phase)


def pre_reference(row, inp):
    B, T, nb, ldr, c = (row[k] for k in ("B", "T", "nb", "ldr", "c"))
    m = inp["mag"].astype(np.float64)[..., c].transpose(0, 2, 1)       # [B, T, nb]
    p = inp["phase"].astype(np.float64)[..., c].transpose(0, 2, 1)
    r, s = np.full((B, T, ldr), SENT), np.zeros((B, T, ldr))
    r[..., :nb], r[..., nb:2 * nb] = m * np.cos(p), m * np.sin(p)
    s[..., :nb] = s[..., nb:2 * nb] = m
    return {"rows": (r, s)}


def pre_fp32(row, inp, mutant=None):
    B, T, nb, ldr = (row[k] for k in ("B", "T", "nb", "ldr"))
    c = 0 if mutant == PRE_MUTANTS[0] else row["c"]
    m, p = inp["mag"][..., c].transpose(0, 2, 1), inp["phase"][..., c].transpose(0, 2, 1)
    co, si = (m * np.cos(p)).astype(F32), (m * np.sin(p)).astype(F32)
    if mutant == PRE_MUTANTS[1]:
        co, si = si, co
    stride = 2 * nb if mutant == PRE_MUTANTS[2] else ldr
    out = np.full(B * T * ldr, SENT, dtype=F32)
    rows = out[:B * T * stride].reshape(B * T, stride)
    rows[:, :nb], rows[:, nb:2 * nb] = co.reshape(B * T, nb), si.reshape(B * T, nb)
    return {"rows": out.reshape(B, T, ldr)}


# ----------------------------------------------------------------------------------------------------------------------------------
# ola (stft.hip istft_ola_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
OLA_MUTANTS = ("t1 unclamped", "n > n_fft as the break", "no tiny test", "no trim", "last frame dropped")
TINY = float(F32(1.1754944e-38))


def _ola_row(S, T, n_fft, hop, ldf, length):
    return dict(id="ola.S%d.T%d.n%d.h%d.ld%d.len%d" % (S, T, n_fft, hop, ldf, length), family="ola", S=S, T=T, n_fft=n_fft, hop=hop, ldf=ldf, length=length,
                full=n_fft + hop * (T - 1))


OLA_ROWS = [_ola_row(*a) for a in ((3, 32, 1022, 512, 1024, 16000), (1, 1, 1022, 512, 1024, 511), (1, 1, 1022, 512, 1024, 2000), (2, 5, 1022, 512, 1024, 3070 - 511),
                                   (2, 5, 1022, 512, 1024, 3070 - 510), (2, 9, 1022, 256, 1024, 2500), (2, 3, 1022, 1022, 1024, 2555), (2, 4, 30, 16, 32, 60),
                                   (132, 32, 1022, 512, 1024, 16000))]


def _ola_jjmax(row):
    return row["length"] - 1 + row["n_fft"] // 2


def ola_cells(row):
    jm, full = _ola_jjmax(row), row["full"]
    out = {"n_fft=%d hop=%d" % (row["n_fft"], row["hop"]), "T=1" if row["T"] == 1 else "T>1", "%d frames per sample" % cdiv(row["n_fft"], row["hop"]),
           "second trip of the grid-stride loop" if second_trip(row["S"] * row["length"]) else "one element per thread"}
    out.add("zero fill past the signal" if jm >= full else "ends at the last sample" if jm == full - 1 else "ends inside the signal")
    if jm == full:
        out.add("first zero-fill sample is the last output")
    if row["hop"] >= row["n_fft"]:
        out.add("wss <= tiny")
    if min(jm, full - 1) >= row["T"] * row["hop"]:
        out.add("t1 clamped")
    return out


def ola_all_cells():
    return {"n_fft=1022 hop=512", "n_fft=1022 hop=256", "n_fft=1022 hop=1022", "n_fft=30 hop=16", "T=1", "T>1", "1 frames per sample", "2 frames per sample",
            "4 frames per sample", "second trip of the grid-stride loop", "one element per thread", "zero fill past the signal", "ends at the last sample",
            "ends inside the signal", "first zero-fill sample is the last output", "wss <= tiny", "t1 clamped"}


def ola_inputs(row):
    S, T, n_fft, ldf = row["S"], row["T"], row["n_fft"], row["ldf"]
    fr = np.full((S, T, ldf), np.nan, dtype=F32)               # columns [n_fft, ldf) are not the kernel's to read
    fr[:, :, :n_fft] = _rng(row).standard_normal((S, T, n_fft)).astype(F32)
    return dict(frames=fr, window=hann_periodic(n_fft))


def _ola_terms(row, fr, w, dtype, mutant=None):
    """The kernel's loop, vectorised over the outputs: step k takes frame t1 - k; -> (acc, wss, sum (f w)^2) in `dtype`."""
    S, T, n_fft, hop, length, full = (row[k] for k in ("S", "T", "n_fft", "hop", "length", "full"))
    jj = np.arange(length) + (0 if mutant == OLA_MUTANTS[3] else n_fft // 2)
    inside = jj < full
    t1 = jj // hop
    top = T - 2 if mutant == OLA_MUTANTS[4] else T - 1
    if mutant != OLA_MUTANTS[0]:
        t1 = np.minimum(t1, top)
    # one frame and one window sample past the end, for the mutants that read them: the next signal's first frame, 0.5 for the window
    frx = np.concatenate((fr.reshape(S * T, -1), np.full((1, fr.shape[-1]), 1.0, dtype=fr.dtype)), 0).astype(dtype)
    wx = np.concatenate((w, [0.5])).astype(dtype)
    acc, wss, q = (np.zeros((S, length), dtype=dtype) for _ in range(3))
    live = inside.copy()
    for k in range(cdiv(n_fft, hop) + 1):
        t = t1 - k
        n = jj - t * hop
        live = live & (t >= 0) & ((n <= n_fft) if mutant == OLA_MUTANTS[1] else (n < n_fft))
        if not live.any():
            break
        tc, nc = np.clip(t, 0, T), np.clip(n, 0, n_fft)
        f = frx[(np.arange(S)[:, None] * T + tc[None, :]), nc[None, :]]
        wv = wx[nc][None, :]
        z = np.zeros((), dtype=dtype)
        acc = acc + np.where(live[None, :], f * wv, z)
        wss = wss + np.where(live[None, :], wv * wv, z)
        q = q + np.where(live[None, :], (f * wv) ** 2, z)
    return acc, wss, q


def ola_reference(row, inp):
    acc, wss, q = _ola_terms(row, inp["frames"].astype(np.float64), inp["window"].astype(np.float64), np.float64)
    div = wss > TINY
    den = np.where(div, wss, 1.0)
    r = acc / den
    return {"y": (r, np.sqrt(q) / den + np.abs(r))}


def ola_fp32(row, inp, mutant=None):
    with np.errstate(all="ignore"):
        acc, wss, _ = _ola_terms(row, inp["frames"], inp["window"], F32, mutant)
        div = np.ones(wss.shape, dtype=bool) if mutant == OLA_MUTANTS[2] else wss > F32(TINY)
        return {"y": np.where(div, acc / wss, acc).astype(F32)}


# ----------------------------------------------------------------------------------------------------------------------------------
# round_mix (stft.hip feeder_round_mix_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
RM_MUTANTS = ("half away from zero", "saturation instead of wrap", "scale before the add", "start ignored")
RM_L, RM_S, RM_SCALES, RM_LAYOUTS = (1, 255, 257, 16000), (1, 4), (1.0, 0.5, 1.0 / 3.0), ((0, 0), (7, 20))
RM_TIES = (0.5, 1.5, 2.5, -0.5, -1.5, 3.49, 32767.4, 32768.0, -32769.0, 40000.2, 32767.5, -32768.5, -40000.7, 6.5)
RM_BIG_L = 2 ** 19 + 1


def _rm_row(first, scale, conv, lay, L, S):
    start, extra = lay
    return dict(id="round_mix.first%d.scale%.3f.%s.start%d.L%d.S%d" % (first, scale, "conv" if conv else "noconv", start, L, S), family="round_mix", first=first,
                scale=scale, conv=conv, start=start, ldfull=L + extra, L=L, S=S)


def _rm_rows():
    R = []
    for (i0, first), (i1, sc), (i2, conv), (i3, lay), (i4, L), (i5, S) in itertools.product(enumerate((1, 0)), enumerate(RM_SCALES), enumerate((False, True)),
                                                                                         enumerate(RM_LAYOUTS), enumerate(RM_L), enumerate(RM_S)):
        if (i0 + i1 + i2 + i3 + i4 + i5) % 2 == 0:      # half of the cross: every (first, scale, conv_out) with every (start, L, S)'s parity class
            R.append(_rm_row(first, sc, conv, lay, L, S))
    return R + [_rm_row(0, 1.0 / 3.0, True, (7, 20), RM_BIG_L, 4)]


RM_ROWS = _rm_rows()


def rm_cells(row):
    out = {("first=%d" % row["first"], "scale=%.3f" % row["scale"], "conv_out given" if row["conv"] else "conv_out NULL"),
           "second trip of the grid-stride loop" if second_trip(row["S"] * row["L"]) else "one element per thread"}
    if row["L"] in RM_L:
        out.add(("start=%d" % row["start"], "L=%d" % row["L"], "S=%d" % row["S"]))
    return out


def rm_all_cells():
    return ({("first=%d" % f, "scale=%.3f" % s, c) for f in (0, 1) for s in RM_SCALES for c in ("conv_out given", "conv_out NULL")} |
            {("start=%d" % st, "L=%d" % L, "S=%d" % S) for st, _ in RM_LAYOUTS for L in RM_L for S in RM_S} |
            {"second trip of the grid-stride loop", "one element per thread"})


def rm_inputs(row):
    g = _rng(row)
    S, L, ld, st = row["S"], row["L"], row["ldfull"], row["start"]
    full = np.full((S, ld), 12345.0, dtype=F32)                # outside [start, start + L): not the kernel's to read
    v = (3000 * g.standard_normal((S, L))).astype(F32)
    k = min(L, len(RM_TIES))
    v[:, :k] = np.asarray(RM_TIES[:k], dtype=F32)
    if L > 2 * len(RM_TIES):
        v[:, -k:] = np.round(v[:, -k:]) + F32(0.5)             # more half-integers, of both parities
    full[:, st:st + L] = v
    mix = np.full((S, L), np.nan, dtype=F32) if row["first"] else (0.3 * g.standard_normal((S, L))).astype(F32)
    return dict(full=full, mix=mix)


def rm_reference(row, inp):
    v = inp["full"][:, row["start"]:row["start"] + row["L"]].astype(np.float64)
    q = np.round(v).astype(np.int64).astype(np.int16).astype(np.float64) / 32768.0
    acc = q if row["first"] else (inp["mix"].astype(np.float64) + q).astype(F32).astype(np.float64)
    mix = (acc * float(F32(row["scale"]))).astype(F32).astype(np.float64)
    return {"conv_out": (q, 0.0), "mix": (mix, 0.0)}


def rm_fp32(row, inp, mutant=None):
    st = 0 if mutant == RM_MUTANTS[3] else row["start"]
    v = inp["full"][:, st:st + row["L"]]
    with np.errstate(all="ignore"):
        r = (np.sign(v) * np.floor(np.abs(v) + F32(0.5))) if mutant == RM_MUTANTS[0] else np.rint(v)
        r = r.astype(np.int64)
        r16 = np.clip(r, -32768, 32767) if mutant == RM_MUTANTS[1] else r.astype(np.int16)
        q = r16.astype(F32) * F32(1.0 / 32768.0)
        sc = F32(row["scale"])
        if mutant == RM_MUTANTS[2]:
            mix = q * sc if row["first"] else inp["mix"] + q * sc
        else:
            mix = (q if row["first"] else inp["mix"] + q) * sc
    return {"conv_out": q.astype(F32), "mix": mix.astype(F32)}


# ----------------------------------------------------------------------------------------------------------------------------------
# rms (stft.hip rms_normalize_kernel: one block of 1024 per clip)
# ----------------------------------------------------------------------------------------------------------------------------------
RMS_MUTANTS = ("mean over n padded to 1024", "zero clip divided")
RMS_N, RMS_NORM = (1, 1000, 1024, 1025, 16384, 16385), 1.2
RMS_ROWS = ([dict(id="rms.S%d.n%d" % (S, n), family="rms", S=S, n=n, zero=False) for S in (1, 3) for n in RMS_N] +
            [dict(id="rms.S3.n1025.zero_clip", family="rms", S=3, n=1025, zero=True)])


def rms_cells(row):
    n = row["n"]
    out = {"S=%d" % row["S"], "n=%d" % n, "n below the block" if n < CLIP_BLOCK else "ragged last stride" if n % CLIP_BLOCK else "whole strides"}
    if row["zero"]:
        out.add("an all-zero clip between two others")
    return out


def rms_all_cells():
    return {"S=1", "S=3"} | {"n=%d" % n for n in RMS_N} | {"n below the block", "ragged last stride", "whole strides", "an all-zero clip between two others"}


def rms_inputs(row):
    mag = np.abs(_rng(row).standard_normal((row["S"], row["n"]))).astype(F32)
    if row["zero"]:
        mag[1] = 0
    return dict(mag=mag)


def strided_sum1024(terms):
    """[S, L] float32 -> [S] float64: thread i of a 1024-thread block adds elements i, i + 1024, ... in float32; block_sum_d adds the
    threads in double."""
    S, L = terms.shape
    k = max(1, cdiv(L, CLIP_BLOCK))
    pad = np.zeros((S, k * CLIP_BLOCK), dtype=F32)
    pad[:, :L] = terms
    acc = np.zeros((S, CLIP_BLOCK), dtype=F32)
    for i in range(k):
        acc = acc + pad[:, i * CLIP_BLOCK:(i + 1) * CLIP_BLOCK]
    return acc.astype(np.float64).sum(1)


def rms_reference(row, inp):
    p = inp["mag"].astype(np.float64)
    rms = np.sqrt((p * p).mean(1, keepdims=True))
    r = np.where(rms != 0, p * float(F32(RMS_NORM)) / np.where(rms != 0, rms, 1.0), p)
    return {"mag": (r, np.abs(r))}


def rms_fp32(row, inp, mutant=None):
    p = inp["mag"]
    n = row["n"]
    den = cdiv(n, CLIP_BLOCK) * CLIP_BLOCK if mutant == RMS_MUTANTS[0] else n
    with np.errstate(all="ignore"):
        rms = np.sqrt((strided_sum1024(p * p) / den).astype(F32))[:, None]
        k = F32(RMS_NORM) / rms
        scaled = (p * k).astype(F32)
    return {"mag": scaled if mutant == RMS_MUTANTS[1] else np.where(rms != 0, scaled, p)}


# ----------------------------------------------------------------------------------------------------------------------------------
# bss (stft.hip bss_metrics_kernel: one block of 1024 per clip)
# ----------------------------------------------------------------------------------------------------------------------------------
BSS_MUTANTS = ("channel sum for channel mean", "means kept", "L mod 1024 tail dropped", "mono-mixture path halved")
BSS_L, BSS_S, BSS_KINDS = (2, 1023, 1024, 1025, 4097, 16000), (1, 5), ("clips", "dc", "near_perfect")
BSS_ROWS = [dict(id="bss.L%d.S%d.%s.%s" % (L, S, "binaural" if mr else "mono", k), family="bss", L=L, S=S, mix_r=mr, kind=k)
            for L in BSS_L for S in BSS_S for mr in (True, False) for k in BSS_KINDS]
BSS_C = 10.0 / np.log(10.0)


def bss_cells(row):
    L = row["L"]
    return {("L=%d" % L, "S=%d" % row["S"]), ("mix_r given" if row["mix_r"] else "mix_r NULL", row["kind"]), ("L=%d" % L, row["kind"]),
            "L below the block" if L < CLIP_BLOCK else "ragged last stride" if L % CLIP_BLOCK else "whole strides"}


def bss_all_cells():
    return ({("L=%d" % L, "S=%d" % S) for L in BSS_L for S in BSS_S} | {(m, k) for m in ("mix_r given", "mix_r NULL") for k in BSS_KINDS} |
            {("L=%d" % L, k) for L in BSS_L for k in BSS_KINDS} | {"L below the block", "ragged last stride", "whole strides"})


def bss_inputs(row):
    g = _rng(row)
    S, L = row["S"], row["L"]
    t = np.arange(L) / 16000.0
    if row["kind"] == "dc":          # offset 0.5 on signals of size 0.01
        ref = 0.5 + 0.01 * g.standard_normal((S, L))
        other = 0.005 * g.standard_normal((S, L))
        est = 0.5 + 0.01 * (ref - 0.5) / 0.01 * g.uniform(0.5, 1.5, (S, 1)) + 0.003 * g.standard_normal((S, L))
        ml, mr = ref + other, 0.8 * (ref - 0.5) + 1.2 * other + 0.45
    else:                           # tests/test_gpu_eval_metrics.py _clips
        ref = np.stack([0.2 * np.sin(2 * np.pi * g.uniform(200, 3000) * t) + 0.05 * g.standard_normal(L) + 0.01 for _ in range(S)])
        other = 0.1 * g.standard_normal((S, L))
        noise = 0.03 if row["kind"] == "clips" else 1.5e-4      # near_perfect: about 60 dB below the scaled target
        est = ref * g.uniform(0.5, 0.9, (S, 1)) + noise * g.standard_normal((S, L)) - 0.02
        ml, mr = ref + other, 0.8 * ref + 1.2 * other + 0.05
    out = dict(ref=ref.astype(F32), est=est.astype(F32), mix_l=ml.astype(F32), mix_r=mr.astype(F32) if row["mix_r"] else None)
    return out


def bss_reference(row, inp, tau=None):
    """-> {"out": (r [S, 11], s, skip)}: skip marks si_sir / si_sar and their improvements, and the outputs whose linearisation does not stand."""
    tau = TAU["bss"] if tau is None else tau
    cen = lambda v: v.astype(np.float64) - v.astype(np.float64).mean(1, keepdims=True)      # noqa: E731
    s = cen(inp["ref"])
    xs = [cen(inp["est"]), 0.5 * (cen(inp["mix_l"]) + cen(inp["mix_r"])) if inp["mix_r"] is not None else cen(inp["mix_l"])]
    S = s.shape[0]
    ss = (s * s).sum(1)
    r, sc, well = np.zeros((2, S, 6)), np.zeros((2, S, 6)), np.ones((2, S, 6), dtype=bool)
    with np.errstate(all="ignore"):
        for w, x in enumerate(xs):
            sx = (s * x).sum(1)
            rel_sx, rel_ss = np.abs(s * x).sum(1) / np.abs(sx), 1.0
            a = sx / ss
            d1, d2 = x - s, x - a[:, None] * s
            n1, n2 = (d1 * d1).sum(1), (d2 * d2).sum(1)
            s_n1 = n1 + 2 * np.sqrt((d1 * d1 * (np.abs(x) + np.abs(s)) ** 2).sum(1))
            s_n2 = n2 + 2 * np.sqrt((d2 * d2 * (np.abs(x) + np.abs(a[:, None] * s)) ** 2).sum(1)) + 2 * np.abs(a) * np.abs((d2 * s).sum(1))
            rel_n1, rel_n2 = s_n1 / n1, s_n2 / n2
            u = 1.0 - 1.0 / a
            rel_u = (rel_sx + rel_ss) / np.abs(a) / np.abs(u)
            snr = 10 * np.log10(ss / n1)
            r[w, :, 0], sc[w, :, 0] = 10 * np.log10(a * a * ss / n2), BSS_C * (2 * rel_sx + rel_ss + rel_n2)
            r[w, :, 3], sc[w, :, 3] = snr + 10 * np.log10(a * a), BSS_C * (rel_ss + rel_n1 + 2 * (rel_sx + rel_ss))
            r[w, :, 4], sc[w, :, 4] = snr, BSS_C * (rel_ss + rel_n1)
            r[w, :, 5], sc[w, :, 5] = -10 * np.log10(u * u), BSS_C * 2 * rel_u
            ok_sx, ok1, ok2, oku = (tau * q <= 0.1 for q in (rel_sx, rel_n1, rel_n2, rel_u))
            well[w, :, 0], well[w, :, 3], well[w, :, 4], well[w, :, 5] = ok_sx & ok2, ok_sx & ok1, ok1, ok_sx & oku
    out, so, ok = np.zeros((S, N_METRICS)), np.zeros((S, N_METRICS)), np.zeros((S, N_METRICS), dtype=bool)
    with np.errstate(invalid="ignore"):     # (L = 2: inf - inf, skipped below)
        for j in (0, 3, 4, 5):
            out[:, j], so[:, j], ok[:, j] = r[0, :, j], sc[0, :, j] + np.abs(r[0, :, j]), well[0, :, j]
        for j, k in ((6, 0), (7, 3), (8, 4)):
            out[:, j] = r[0, :, k] - r[1, :, k]
            so[:, j] = sc[0, :, k] + sc[1, :, k] + np.abs(r[0, :, k]) + np.abs(r[1, :, k])
            ok[:, j] = well[0, :, k] & well[1, :, k]
    skip = ~ok | ~np.isfinite(out) | ~np.isfinite(so)
    return {"out": (np.where(skip, 0.0, out), np.where(skip, 0.0, so), skip)}


def bss_fp32(row, inp, mutant=None):
    ref, est, ml, mr = inp["ref"], inp["est"], inp["mix_l"], inp["mix_r"]
    S, L = ref.shape
    keep = (L // CLIP_BLOCK) * CLIP_BLOCK if mutant == BSS_MUTANTS[2] else L
    tot = lambda t: strided_sum1024(np.ascontiguousarray(t[:, :keep]))      # noqa: E731
    EPS = 1e-13
    with np.errstate(all="ignore"):
        mean = (lambda v: np.zeros((S, 1), dtype=F32)) if mutant == BSS_MUTANTS[1] else (lambda v: (tot(v) / L).astype(F32)[:, None])
        sv = ref - mean(ref)
        x0 = est - mean(est)
        l = ml - mean(ml)
        if mr is not None:
            x1 = (l + (mr - mean(mr))) if mutant == BSS_MUTANTS[0] else F32(0.5) * (l + (mr - mean(mr)))
        else:
            x1 = F32(0.5) * l if mutant == BSS_MUTANTS[3] else l
        ss = tot(sv * sv)
        m = np.zeros((2, S, 6))
        for w, xv in enumerate((x0, x1)):
            alpha = tot(sv * xv) / ss
            af = alpha.astype(F32)[:, None]
            d1, d2 = xv - sv, xv - sv * af
            noise1, noise2 = tot(d1 * d1), tot(d2 * d2)
            b = tot(sv * d2) / ss + EPS
            bf = b.astype(F32)[:, None]
            d = (d2 - sv * bf) + F32(EPS)
            artif = tot(d * d)
            signal2 = alpha * alpha * ss
            snr = 10 * np.log10(ss / noise1)
            m[w] = np.stack((10 * np.log10(signal2 / noise2), 10 * np.log10(signal2 / (b * b * ss)), 10 * np.log10(signal2 / artif),
                             snr + 10 * np.log10(alpha * alpha), snr, -10 * np.log10((1 - 1 / alpha) * (1 - 1 / alpha))), 1)
        out = np.concatenate((m[0], (m[0] - m[1])[:, (0, 3, 4, 1, 2)]), 1)
    return {"out": out.astype(F32)}


# ----------------------------------------------------------------------------------------------------------------------------------
# fftconv (fftconv.hip fftconv_kernel<LOGM>, fft_lds.h load_packed / fft_dif / ifft_dit / rfft_unpack / rfft_repack)
# ----------------------------------------------------------------------------------------------------------------------------------
FC_MUTANTS = ("output rotated by one sample (circular wrap by one)", "last sample of an odd length dropped", "the k = M/2 pair skipped",
              "DC and Nyquist products swapped", "ear stride 1")
FC_TABLE = ((900, 1000, 11), (1025, 1024, 11), (2049, 2000, 12), (2000, 2049, 12), (4000, 2049, 13), (8000, 8001, 14), (16000, 16000, 15), (16385, 16384, 15),
            (1, 1500, 11), (1500, 1, 11), (100, 100, 11), (100, 100, 15))
FC_KINDS = ("feeder", "impulse", "dc")


def _fc_rows():
    R = []
    for i, (L, Lr, n) in enumerate(FC_TABLE):
        for j, kind in enumerate(FC_KINDS):     # every table row with every kind and both CS; every (CS, kind) over the table
            CS = (1, 6)[(i + j) % 2]
            R.append(dict(id="fftconv.L%d.Lr%d.n%d.%s.CS%d" % (L, Lr, n, kind, CS), family="fftconv", L=L, Lr=Lr, log2n=n, kind=kind, CS=CS))
    return R


FC_ROWS = _fc_rows()


def fc_cells(row):
    L, Lr, n = row["L"], row["Lr"], row["log2n"]
    tab = "L=%d Lr=%d 2^%d" % (L, Lr, n)
    out = {(tab, row["kind"]), (tab, "CS=%d" % row["CS"]), ("CS=%d" % row["CS"], row["kind"]), "instance 2^%d" % n}
    if L % 2:
        out.add("odd L")
    if Lr % 2:
        out.add("odd Lr")
    if L + Lr - 1 == 1 << n:
        out.add("fills the transform exactly")
    if L + Lr - 1 <= (1 << n) // 2 and n > 11:
        out.add("a transform longer than needed")
    if L == 1:
        out.add("L=1")
    if Lr == 1:
        out.add("Lr=1")
    return out


def fc_all_cells():
    tabs = ["L=%d Lr=%d 2^%d" % t for t in FC_TABLE]
    return ({(t, k) for t in tabs for k in FC_KINDS} | {(t, "CS=%d" % c) for t in tabs for c in (1, 6)} | {("CS=%d" % c, k) for c in (1, 6) for k in FC_KINDS} |
            {"instance 2^%d" % n for n in FFTCONV_LOG2N} | {"odd L", "odd Lr", "fills the transform exactly", "a transform longer than needed", "L=1", "Lr=1"})


def feeder_audio(g, shape_mono, shape_rir):
    """The feeder's synthetic audio (tests/test_gpu_feeder.py _inputs): mono = round(3000 N(0,1)) as int16, RIR = N(0,1) exp(-t / 0.05 s),
    peak-normalised to 0.05."""
    mono = np.clip(np.round(3000 * g.standard_normal(shape_mono)), -32768, 32767).astype(F32)
    Lr = shape_rir[-2]
    rir = (g.standard_normal(shape_rir) * np.exp(-np.arange(Lr) / 16000.0 / 0.05)[:, None]).astype(F32)
    rir /= np.abs(rir).max(axis=(-2, -1), keepdims=True)
    return mono, (rir * F32(0.05)).astype(F32)


def fc_inputs(row):
    g = _rng(row)
    CS, L, Lr = row["CS"], row["L"], row["Lr"]
    if row["kind"] == "feeder":
        mono, rir = feeder_audio(g, (CS, L), (CS, Lr, 2))
    elif row["kind"] == "impulse":  # an impulse at the last sample of the clip and of either ear's response
        mono, rir = np.zeros((CS, L), dtype=F32), np.zeros((CS, Lr, 2), dtype=F32)
        mono[:, L - 1] = 12345 - 100 * np.arange(CS)
        rir[:, Lr - 1] = (0.04, -0.03)
    else:
        mono = np.round(2000 + 30 * g.standard_normal((CS, L))).astype(F32)
        rir = (0.01 + 0.001 * g.standard_normal((CS, Lr, 2))).astype(F32)
    return dict(mono=mono, rirs=rir, tw=twiddles(1 << row["log2n"]))


def twiddles(nfft):
    """BinauralFeeder._twiddle_table: exp(-2 pi i k / nfft), k < nfft / 2, interleaved float32 from float64."""
    k = np.arange(nfft // 2, dtype=np.float64)
    return np.stack([np.cos(2.0 * np.pi * k / nfft), -np.sin(2.0 * np.pi * k / nfft)], axis=1).astype(F32)


def conv_reference(mono, rirs, nfft):
    """mono [CS, L], rirs [CS, Lr, 2] -> (the float64 linear convolution in its nfft circular points [CS, 2, nfft], s of the same shape: the
    rms of the result over the L + Lr - 1 points it occupies)."""
    CS = mono.shape[0]
    r = np.zeros((CS, 2, nfft))
    for c in range(CS):
        for ear in range(2):
            y = np.convolve(mono[c].astype(np.float64), rirs[c, :, ear].astype(np.float64))
            r[c, ear, :y.size] = y
    s = np.sqrt((r * r).sum(-1, keepdims=True) / (mono.shape[1] + rirs.shape[1] - 1))
    return r, np.broadcast_to(s, r.shape).copy()


def fc_reference(row, inp):
    return {"full": conv_reference(inp["mono"], inp["rirs"], 1 << row["log2n"])}


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def _cmulc(ar, ai, br, bi):      # a * conj(b)
    return ar * br + ai * bi, ai * br - ar * bi


def _stage(zr, zi, tw, logm, s, inverse):
    M = 1 << logm
    half = M >> (s + 1)
    shp = zr.shape[:-1]
    tr, ti = tw[(np.arange(half) << s) * 2, 0], tw[(np.arange(half) << s) * 2, 1]
    vr, vi = zr.reshape(shp + (-1, 2, half)), zi.reshape(shp + (-1, 2, half))
    ar, ai, br, bi = vr[..., 0, :], vi[..., 0, :], vr[..., 1, :], vi[..., 1, :]
    if inverse:
        br, bi = _cmulc(br, bi, tr, ti)
        o = (ar + br, ai + bi, ar - br, ai - bi)
    else:
        o = (ar + br, ai + bi) + _cmul(ar - br, ai - bi, tr, ti)
    return np.stack((o[0], o[2]), -2).reshape(shp + (M,)), np.stack((o[1], o[3]), -2).reshape(shp + (M,))


def fft_dif(zr, zi, tw, logm):
    for s in range(logm):
        zr, zi = _stage(zr, zi, tw, logm, s, False)
    return zr, zi


def ifft_dit(zr, zi, tw, logm):
    for s in range(logm - 1, -1, -1):
        zr, zi = _stage(zr, zi, tw, logm, s, True)
    return zr, zi


def bit_rev(k, logm):
    k = np.asarray(k)
    r = np.zeros_like(k)
    for i in range(logm):
        r |= ((k >> i) & 1) << (logm - 1 - i)
    return r


def load_packed(x, M, drop_odd=False):
    """x [..., n] -> z[m] = x[2m] + i x[2m + 1], zero from sample n on."""
    n = x.shape[-1]
    if drop_odd:
        n -= n % 2
    pad = np.zeros(x.shape[:-1] + (2 * M,), dtype=F32)
    pad[..., :n] = x[..., :n]
    return pad[..., 0::2].copy(), pad[..., 1::2].copy()


def rfft_unpack(tr, ti, zkr, zki, zmr, zmi):
    """fft_lds.h rfft_unpack of the pair (k, M-k), t = tw[k] -> (E, T O): S[k] = E + T O, conj(S[M-k]) = E - T O."""
    half = F32(0.5)
    er, ei = half * (zkr + zmr), half * (zki - zmi)
    dr, di = half * (zkr - zmr), half * (zki + zmi)
    return (er, ei) + _cmul(tr, ti, di, -dr)


def rfft_repack(tr, ti, ykr, yki, ymr, ymi):
    """fft_lds.h rfft_repack of Y[k] and conj(Y[M-k]) -> (Z'[k], Z'[M-k]) for the inverse packed transform."""
    half = F32(0.5)
    e2r, e2i = half * (ykr + ymr), half * (yki + ymi)
    o2r, o2i = _cmulc(half * (ykr - ymr), half * (yki - ymi), tr, ti)
    return e2r - o2i, e2i + o2r, e2r + o2i, -e2i + o2r


def fc_fp32(row, inp, mutant=None):
    logm = row["log2n"] - 1
    M = 1 << logm
    tw = inp["tw"]
    drop = mutant == FC_MUTANTS[1]
    rirs = inp["rirs"]
    if mutant == FC_MUTANTS[4]:     # ear e: Lr consecutive floats from rirs + cs * Lr * 2 + e
        flat = np.concatenate((rirs.reshape(rirs.shape[0], -1), np.zeros((rirs.shape[0], 1), dtype=F32)), 1)
        h = np.stack((flat[:, 0:row["Lr"]], flat[:, 1:row["Lr"] + 1]), 1)
    else:
        h = rirs.transpose(0, 2, 1)                             # [CS, 2, Lr]
    xr, xi = fft_dif(*load_packed(inp["mono"], M, drop), tw, logm)
    hr, hi = fft_dif(*load_packed(np.ascontiguousarray(h), M, drop), tw, logm)
    xr, xi = xr[:, None, :], xi[:, None, :]
    zr, zi = hr.copy(), hi.copy()
    half = F32(0.5)
    # slot 0: the two real bins
    y0, ym = (xr[..., 0] + xi[..., 0]) * (hr[..., 0] + hi[..., 0]), (xr[..., 0] - xi[..., 0]) * (hr[..., 0] - hi[..., 0])
    if mutant == FC_MUTANTS[3]:
        y0, ym = ym, y0
    zr[..., 0], zi[..., 0] = half * (y0 + ym), half * (y0 - ym)
    k = np.arange(1, M // 2 + 1)
    ik, im = bit_rev(k, logm), bit_rev(M - k, logm)
    tr, ti = tw[k, 0], tw[k, 1]

    exr, exi, oxr, oxi = rfft_unpack(tr, ti, xr[..., ik], xi[..., ik], xr[..., im], xi[..., im])
    ehr, ehi, ohr, ohi = rfft_unpack(tr, ti, hr[..., ik], hi[..., ik], hr[..., im], hi[..., im])
    ykr, yki = _cmul(exr + oxr, exi + oxi, ehr + ohr, ehi + ohi)
    ymr, ymi = _cmul(exr - oxr, exi - oxi, ehr - ohr, ehi - ohi)
    zkr, zki, zmr, zmi = rfft_repack(tr, ti, ykr, yki, ymr, ymi)
    last = -1 if mutant == FC_MUTANTS[2] else None
    zr[..., im[:-1]], zi[..., im[:-1]] = zmr[..., :-1], zmi[..., :-1]
    zr[..., ik[:last]], zi[..., ik[:last]] = zkr[..., :last], zki[..., :last]
    zr, zi = ifft_dit(zr, zi, tw, logm)
    sc = F32(1.0) / F32(M)
    out = np.stack((zr * sc, zi * sc), -1).reshape(zr.shape[:-1] + (2 * M,)).astype(F32)
    if mutant == FC_MUTANTS[0]:
        out = np.roll(out, 1, -1)
    return {"full": out}


# ----------------------------------------------------------------------------------------------------------------------------------
# chain (BinauralFeeder.convolve_round)
# ----------------------------------------------------------------------------------------------------------------------------------
CHAIN_ROWS = [dict(id="chain.L%d.Lr%d" % (L, Lr), family="chain", B=2, S=2, L=L, Lr=Lr) for L, Lr in ((16000, 16000), (2049, 2000))]


def chain_nfft(L, Lr):
    """BinauralFeeder.convolve_round's transform length."""
    p = 1
    while p < L + Lr - 1:
        p *= 2
    return max(p, 2048)


def chain_cells(row):
    return {"L=%d Lr=%d" % (row["L"], row["Lr"])}


def chain_all_cells():
    return {"L=16000 Lr=16000", "L=2049 Lr=2000"}


def chain_inputs(row):
    mono, rir = feeder_audio(_rng(row), (row["B"], row["S"], row["L"]), (row["B"], row["S"], row["Lr"], 2))
    return dict(mono=mono, rirs=rir * F32(0.5))      # (a quieter room: the share of samples within tau s of a tie grows with the level, tie rule 2)


def chain_reference(row, inp, tau=None):
    """-> {"per_source": (q [S][B, 2, L] in int16 units, near [S][B, 2, L]: within tau s of a half-integer)}; the mixture is judged from the
    per-source values the implementation made (chain_mix)."""
    tau = TAU["chain"] if tau is None else tau
    B, S, L, Lr = (row[k] for k in ("B", "S", "L", "Lr"))
    nfft, start = chain_nfft(L, Lr), (Lr - 1) // 2
    r, s = conv_reference(inp["mono"].reshape(B * S, L), inp["rirs"].reshape(B * S, Lr, 2), nfft)
    v = r.reshape(B, S, 2, nfft)[..., start:start + L].transpose(1, 0, 2, 3)        # [S, B, 2, L]
    s = s.reshape(B, S, 2, nfft)[..., start:start + L].transpose(1, 0, 2, 3)
    q = np.round(v).astype(np.int64).astype(np.int16).astype(np.float64)
    near = np.abs(v - (np.floor(v) + 0.5)) <= tau * s
    return {"per_source": (q, near)}


def chain_mix(per_source):
    """The exact float32 mixture of S per-source waveforms [S][B, 2, L] (already * 2^-15): adds in order, then the 1 / S of the last launch."""
    acc = per_source[0].astype(F32)
    for p in per_source[1:]:
        acc = (acc + p.astype(F32)).astype(F32)
    return (acc * F32(1.0 / len(per_source))).astype(F32)


def chain_fp32(row, inp, mutant=None):
    B, S, L, Lr = (row[k] for k in ("B", "S", "L", "Lr"))
    nfft, start = chain_nfft(L, Lr), (Lr - 1) // 2
    fc = dict(log2n=nfft.bit_length() - 1, Lr=Lr)
    full = fc_fp32(fc, dict(mono=inp["mono"].reshape(B * S, L), rirs=inp["rirs"].reshape(B * S, Lr, 2), tw=twiddles(nfft)))["full"].reshape(B, S, 2, nfft)
    per = []
    for s in range(S):
        rm = dict(start=start, L=L, first=1, scale=1.0)
        per.append(rm_fp32(rm, dict(full=full[:, s].reshape(B * 2, nfft), mix=None))["conv_out"].reshape(B, 2, L))
    return {"per_source": per, "mix": chain_mix(per)}


# ----------------------------------------------------------------------------------------------------------------------------------
# the families together
# ----------------------------------------------------------------------------------------------------------------------------------
ROWS = {"frames": FRAMES_ROWS, "dft": DFT_ROWS, "post": POST_ROWS, "pre": PRE_ROWS, "ola": OLA_ROWS, "round_mix": RM_ROWS, "rms": RMS_ROWS, "bss": BSS_ROWS,
        "fftconv": FC_ROWS, "chain": CHAIN_ROWS}
ROWS_BY_ID = {r["id"]: r for rows in ROWS.values() for r in rows}
CELLS = {"frames": frames_cells, "dft": dft_cells, "post": post_cells, "pre": pre_cells, "ola": ola_cells, "round_mix": rm_cells, "rms": rms_cells, "bss": bss_cells,
         "fftconv": fc_cells, "chain": chain_cells}
_ALL = {"frames": frames_all_cells, "dft": dft_all_cells, "post": post_all_cells, "pre": pre_all_cells, "ola": ola_all_cells, "round_mix": rm_all_cells,
        "rms": rms_all_cells, "bss": bss_all_cells, "fftconv": fc_all_cells, "chain": chain_all_cells}
INPUTS = {"frames": frames_inputs, "dft": dft_inputs, "post": post_inputs, "pre": pre_inputs, "ola": ola_inputs, "round_mix": rm_inputs, "rms": rms_inputs,
          "bss": bss_inputs, "fftconv": fc_inputs, "chain": chain_inputs}
REFERENCE = {"frames": frames_reference, "dft": dft_reference, "post": post_reference, "pre": pre_reference, "ola": ola_reference, "round_mix": rm_reference,
             "rms": rms_reference, "bss": bss_reference, "fftconv": fc_reference}
FP32 = {"frames": frames_fp32, "dft": dft_fp32, "post": post_fp32, "pre": pre_fp32, "ola": ola_fp32, "round_mix": rm_fp32, "rms": rms_fp32, "bss": bss_fp32,
        "fftconv": fc_fp32}


def cells(row):
    return CELLS[row["family"]](row)


def all_cells(family):
    return _ALL[family]()


def inputs(row):
    return INPUTS[row["family"]](row)


def reference(row, inp):
    """{output: (r, s) or (r, s, skip)} in float64."""
    return REFERENCE[row["family"]](row, inp)


def sgrid_total(row):
    """Work items of the row's sgrid launch (None: the family's kernel is not an sgrid one)."""
    f = row["family"]
    if f == "frames":
        return row["S"] * row["T"] * row["ldf"]
    if f == "post":
        return row["B"] * row["nb"] * row["T"] * row["C"]
    if f == "pre":
        return row["B"] * row["T"] * row["nb"]
    if f == "ola":
        return row["S"] * row["length"]
    if f == "round_mix":
        return row["S"] * row["L"]
    return None


def largest_buffer_bytes(row):
    f = row["family"]
    if f == "frames":
        return 4 * max(row["S"] * row["T"] * row["ldf"], row["S"] * row["L"])
    if f == "post":
        return 4 * row["B"] * row["C"] * row["T"] * row["lds"]
    if f == "pre":
        return 4 * max(row["B"] * row["T"] * row["ldr"], row["B"] * row["nb"] * row["T"] * row["C"])
    if f == "ola":
        return 4 * max(row["S"] * row["T"] * row["ldf"], row["S"] * row["length"])
    if f == "round_mix":
        return 4 * row["S"] * row["ldfull"]
    if f == "dft":
        return 4 * 1024 * 1024
    if f == "rms":
        return 4 * row["S"] * row["n"]
    if f == "bss":
        return 4 * row["S"] * row["L"]
    if f == "fftconv":
        return 4 * row["CS"] * 2 * (1 << row["log2n"])
    return 4 * row["B"] * row["S"] * 2 * chain_nfft(row["L"], row["Lr"])


# mutant -> (family, predicate on the row: the rows the bound must reject the mutant on)
MUTANT_ROWS = {
    FRAMES_MUTANTS[0]: ("frames", lambda r: True),
    FRAMES_MUTANTS[1]: ("frames", frames_reflects_right),
    FRAMES_MUTANTS[2]: ("frames", lambda r: r["n_fft"] % 2 == 1),
    FRAMES_MUTANTS[3]: ("frames", lambda r: True),
    POST_MUTANTS[0]: ("post", lambda r: r["mode"] == 2 and r["outs"] != "phase"),
    POST_MUTANTS[1]: ("post", lambda r: r["C"] > 1 and r["T"] > 1),
    POST_MUTANTS[2]: ("post", lambda r: r["lds"] > 2 * r["nb"]),
    POST_MUTANTS[3]: ("post", lambda r: r["outs"] != "mag"),
    PRE_MUTANTS[0]: ("pre", lambda r: r["c"] > 0),
    PRE_MUTANTS[1]: ("pre", lambda r: True),
    PRE_MUTANTS[2]: ("pre", lambda r: r["ldr"] > 2 * r["nb"]),
    OLA_MUTANTS[0]: ("ola", lambda r: min(_ola_jjmax(r), r["full"] - 1) >= r["T"] * r["hop"]),
    OLA_MUTANTS[1]: ("ola", lambda r: min(_ola_jjmax(r), r["full"] - 1) >= r["n_fft"]),
    OLA_MUTANTS[2]: ("ola", lambda r: r["hop"] >= r["n_fft"]),
    OLA_MUTANTS[3]: ("ola", lambda r: True),
    OLA_MUTANTS[4]: ("ola", lambda r: True),
    RM_MUTANTS[0]: ("round_mix", lambda r: True),
    RM_MUTANTS[1]: ("round_mix", lambda r: r["L"] > 1),
    RM_MUTANTS[2]: ("round_mix", lambda r: r["first"] == 0 and r["scale"] != 1.0),
    RM_MUTANTS[3]: ("round_mix", lambda r: r["start"] > 0),
    RMS_MUTANTS[0]: ("rms", lambda r: r["n"] % CLIP_BLOCK != 0),
    RMS_MUTANTS[1]: ("rms", lambda r: r["zero"]),
    BSS_MUTANTS[0]: ("bss", lambda r: r["mix_r"] and r["L"] > 2),
    BSS_MUTANTS[1]: ("bss", lambda r: r["kind"] == "dc" and r["L"] > 2),
    BSS_MUTANTS[2]: ("bss", lambda r: r["L"] % CLIP_BLOCK > 1 and r["L"] > 2),        # (one sample of 4097 moves a ratio of sums by 1.5 .. 3.4 tau s)
    BSS_MUTANTS[3]: ("bss", lambda r: not r["mix_r"] and r["L"] > 2),
    FC_MUTANTS[0]: ("fftconv", lambda r: True),
    # (the 8001st sample of a feeder response has decayed to 4.5e-5 of its peak: 2.7 tau s)
    FC_MUTANTS[1]: ("fftconv", lambda r: (r["L"] % 2 == 1 or r["Lr"] % 2 == 1) and not (r["kind"] == "feeder" and r["Lr"] == 8001)),
    # (bin M/2 of a DC-heavy pair holds 1e-6 of its energy; two impulses at samples of equal parity have equal DC and Nyquist products)
    FC_MUTANTS[2]: ("fftconv", lambda r: r["kind"] == "feeder"),
    FC_MUTANTS[3]: ("fftconv", lambda r: r["kind"] != "impulse"),
    FC_MUTANTS[4]: ("fftconv", lambda r: r["Lr"] > 1),
}
