"""The kernels of the shipped path, Separator / SeparatorStream (TEST INFRASTRUCTURE): csrc/separate.hip (sep_frames, sep_stft_post,
sep_istft_pre, sep_bin_rows, sep_istft_ola, sep_istft_xfade and their window forms), csrc/resample.hip (the four tile sizes, with one
phase and with a table, and the direct kernel) and the three slice kernels of csrc/layout.hip -- the table of test rows per family, the
cells the rows must reach, seeded inputs, the float64 reference of every output with its element-wise error scale, float32 numpy
restatements of each kernel's algorithm in the kernel's own order, named mutants of those restatements, and the restated launch geometry.

tests/test_gpu_separator_kernels.py runs every row through the m2h.ops function the project itself calls (m2h_sep_frames and the split32
slice through the C ABI: ops does not reach them) against ``reference``; tests/test_separator_kernels_cpu.py checks without a GPU that the
rows reach every cell, that every restatement stays inside half its family's tau on every row, that every mutant leaves the bound on the
rows named for it (by MIN_MARGIN at the least), and that the restated geometry is the sources'.

Rules (tests/train_kernels.py's, unchanged).  Checks are LOCAL: every kernel is referenced in float64 from the float32 tensors it was
handed, the partial sums an earlier cross-fade call left in y and the resampler's table G among them.  NO ELEMENT IS LEFT OUT of any
comparison: ``check`` returns the count it compared and every test asserts that it is the size of the whole output buffer.  Output buffers
are NaN before the call (but where m2h.ops allocates the output itself: pre without out=, post, the float32 slice rows -- every element of
those is written and compared); a reference element that is NaN is one the definition does not write, and the output must still be NaN
there (samples at or past L, segments outside [s0, s0 + nseg), window positions outside the span, the floats around a view).  Input buffers
hold NaN wherever the definition reads zero (window positions at or past `end`, the resampler's neighbouring rows in the isolation rows,
frame columns 1022 and 1023 of the inverse transform's rows): the kernels select those positions, they do not multiply them.

Scales
  frames     exact (s = 0): one correctly rounded product, 0 at n = 1023, 0 for samples at or past `end`
  post       log1p|X_c|: s(m) / (1 + m) + |r|, s(m) = m + u(m) / tau with feeder_kernels' underflow term u.
             phasor D / |D|, D = X_0 + X_1: s = 1 per component; exactly (1, 0) where both components of D are zero (s = 0)
  pre        expm1(max(P, 0)) * (re | im): s = |r|, exactly 0 where P <= 0
  bin_rows   exact: max(mask_c, 0) * (re | im), one correctly rounded product
  ola        sqrt(sum (f w)^2) / wss + |r| (undivided where wss <= tiny)
  xfade      sum over the chunk's covering segments of (xwin / W) s_ola + |prior partial| + |r|; what the call does not write keeps the
             float32 value (or the NaN) it held, exactly
  resample   y[n] = sum_k G[p][k] x[j0 - k] in float64 from the float32 x and G: s = sqrt(sum (g x)^2)
  slice      unmasked and plane forms exact.  Masked, r = log1p(z), z = max(m (e - 1), 0), e = exp(x): the exponent's argument carries
             eps |x| (x log2 e is rounded before exp2), which is worth e |x| eps to e, and e its own eps e: e is known to e (1 + |x|) eps.
             The subtraction e - 1 is exact or adds eps |e - 1| <= eps e, so m (e - 1) carries |m| e (1 + |x|) eps absolutely -- however
             small e - 1 is, which is the cancellation -- and log1p divides it by 1 + z.  With the result's own rounding:
             s = |m| e (1 + |x|) / (1 + z) + |r|, and exactly 0 (s = 0) where m (e - 1) <= 0.  The restatement of masked_log_mag
             (exp2, log2 (u) z / (u - 1), rcp) needs no further term: 1.4e-7 at the worst on float32 output.
             split32 output: hi + lo of an exact value is exact (s = 0, the reference is split the same way); of a masked value
             s + 2^-17 |r|, the output's own rounding joining s as in tests/test_gpu_forward_fp64.py (s holds |r|, so tau s stays above
             the 2^-17 |r| the format keeps; the restatement stands at 3.34e-6).

tau: TAU_FP32 for every family, but for ONE row: resample.1000-1.two_tiles+1.xoff0.yoff1, the direct kernel's fmaf chain of T = 20001 taps.
Its float32 restatement (the k = 0 .. T-1 chain with fmaf's single rounding: the product is exact in float64) stands at 1.67e-5 of
sqrt(sum (g x)^2), above TAU_FP32 / 2: a sequential float32 sum of T terms carries about eps sqrt(T / 2) = 6e-6 of that scale, 1.67e-5 at the
worst of the row's 514 outputs.  By the rule feeder_kernels.py used for fftconv the rows with T >= 4096 (this one alone) take
tau = 8 x 1.75e-5 = 1.4e-4, derived from the reference and the restatement alone, and the CPU test holds the restatement under 1.75e-5.
Worst restatement ratios of everything else (tests/test_separator_kernels_cpu.py::test_zz_mutant_margins prints them): frames and bin_rows
exact, post 1.26e-7, pre 1.80e-7, ola 1.39e-7, xfade 1.21e-7, resample 2.72e-6 (resample.512000-16000.two_tiles+1.xoff2.yoff3, T = 641),
slice 3.34e-6 (slice.B2.F512.T32.C2.mixed.split32).

DEPARTURES from the issue, each with its reason:
  post       magnitude at the 1e37 plants: the reference is the float64 log1p|X_c| with the family's scale, like every other bin, and
             where |X_c| >= 2^64 the output may be +inf in its place.  re * re + im * im is a float32 sum in this kernel as in stft_post
             and overflows there; the test pins that behaviour, it does not endorse it: a kernel that kept the magnitude finite passes
             as well, any other value fails.  (|X| >= 2^64 does not occur for audio.)  The phasor is held to s = 1 there like everywhere.
  xfade      "b clamped by S - 1" and its mutant "b unclamped": unreachable.  A quad starts at n0 < n_end <= L, so n0 div hop <=
             (L - 1) div hop = ceil(L / hop) - 1 = S - 1 for every hop: the clamp never binds.  The mutant is kept and
             test_xfade_b_clamp_is_dead asserts that it is bit-identical to the restatement on every row (margin 0).  The cell that is
             reachable, a short last segment, is kept.
  ola        "the wss guard": with the periodic Hann window every sample has wss >= w[511]^2 = 1.  The row ola.R1.L16000.wzero hands the
             kernel a window with w[511] = 0 and w[510] = 1e-20 (the window is an input): samples 512 t are an undivided exact 0 and
             samples 512 t - 1 an undivided product.
             "store past L" can only show where something follows the last sample written: the window row with cap > end - origin.
  xfade      no chunk holds more than 3 segments (the issue's nseg in 1..3): the samples 4 segments cover are reached by chunked rows.
  resample   the ratios of tests/test_gpu_resample.py reach the tiles of 512 and 256 outputs with one phase only; 64000 -> 3000 and
             128000 -> 3000 are added for those tiles with a table (test_resampler_choice_reaches_every_kernel proves both statements from
             the restated rule).  The direct kernel has no tile and no seam: its rows hold one block of 256 outputs and 1..3 more.
             "lead count wrong" is the lead not cut at cnt; "cnt off by one at the seam" the last tile's last output not stored.
  slice      the two grid-stride rows hold the smallest totals above 4096 x 256: 4 x 262145 and 5 x 209716 = 1048580 items.

Mutant margins (worst |g - r| / (tau s) over a mutant's named rows, the smallest over those rows; inf = an exact or unwritten element
differs, or a value is not finite):
  frames     all six inf
  post       no scaling by big inf, guard yields (0, 0) inf, phasor of channel 0 alone inf (an exact (1, 0)), channels swapped 1.5e+06,
             t / k transposed inf
  pre        clamp missing inf, re / im swapped 8.5e+08, row stride 512 inf
  bin_rows   all three inf
  ola        t1 unclamped 4.3e+04, n > 1022 as the break inf, s0 ignored inf, store past L inf, origin ignored inf
  xfade      W over the chunk's segments only 1.1e+07, prior partial ignored 2.5e+04, prior partial always read inf, xwin without the
             division 1.8e+04, b unclamped 0 (dead code, above)
  resample   one tap dropped 6.9e+02, taps shifted by one 4.8e+01, half omitted from t 3.6e+04, the other five inf
  slice      mask applied to the log value 2.2e+04, the other five inf
"""
import numpy as np

import feeder_kernels as Fk
from elem_bound import TAU_FP32
from train_kernels import F32, cdiv, seed_of

FAMILIES = ("frames", "post", "pre", "bin_rows", "ola", "xfade", "resample", "slice")
TAU = {f: TAU_FP32 for f in FAMILIES}
MIN_MARGIN = 4.0
TINY = Fk.TINY
# ceilings of the worst restatement ratio per family against the float64 reference (the long-chain row apart), held by the CPU test
RESTATEMENT_WORST = {"frames": 0.0, "post": 2e-7, "pre": 2e-7, "bin_rows": 0.0, "ola": 2e-7, "xfade": 2e-7, "resample": 3e-6, "slice": 4e-6}

# ---- the restated geometry of csrc/separate.hip (tests/test_separator_kernels_cpu.py holds it against the source)
SEP_SEG, SEP_T, SEP_NB, SEP_LD, SEP_NFFT, SEP_NIFFT, SEP_HOP, SEP_KT = 16000, 32, 512, 1024, 1023, 1022, 512, 32
SEP_GRID_CAP, SEP_BLOCK = 16384, 256
SEP_HOPS = (16000, 8000, 4000)
# ---- and of csrc/resample.hip
RS_THREADS, RS_LDS_BYTES, RS_MAX_RATIO = 256, 64 * 1024, 1024


# resample rows whose chain has RS_LONG_CHAIN_T taps or more (1000 -> 1: T = 20001, the direct kernel) take a tau of their own, 8 x the worst
# ratio of the float32 fmaf-chain restatement against the float64 reference (module docstring); the CPU test holds the row under the eighth
RS_LONG_CHAIN_T, RS_LONG_CHAIN_WORST = 4096, 1.75e-5
TAU_RS_LONG_CHAIN = 8 * RS_LONG_CHAIN_WORST


def tau_of(row):
    if row["family"] == "resample" and rs_design(row["f_in"], row["f_out"])[3] >= RS_LONG_CHAIN_T:
        return TAU_RS_LONG_CHAIN
    return TAU[row["family"]]


def restatement_limit(row):
    return RS_LONG_CHAIN_WORST if tau_of(row) == TAU_RS_LONG_CHAIN else tau_of(row) / 2


def sep_grid(total):
    return max(1, min(cdiv(total, SEP_BLOCK), SEP_GRID_CAP))


def second_pass(total):
    """A thread of a sep_grid launch takes a second item."""
    return total > sep_grid(total) * SEP_BLOCK


def _rng(row):
    return np.random.default_rng(seed_of(row["id"]))


def check(g, r, s, tau, inf_ok=None):
    """(worst |g - r| / s, least-squares scale, holds, elements compared): where the reference is NaN the output must be NaN (not written);
    everything else goes through feeder_kernels.check (train_kernels.check with the flush slack; exact equality where r is infinite).
    inf_ok: elements where +inf is accepted in place of a value inside the bound (post's magnitude past the float32 range)."""
    g = np.asarray(g).reshape(-1)
    if inf_ok is not None:
        g = np.where(np.asarray(inf_ok).reshape(-1) & (g == np.inf), np.asarray(r, dtype=np.float64).reshape(-1), g)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), np.shape(r)) if np.ndim(s) == 0 else np.asarray(s, dtype=np.float64).reshape(-1)
    assert g.size == r.size == s.size, (g.size, r.size, s.size)
    un = np.isnan(r)
    if not np.isnan(g[un]).all() or np.isnan(g[~un]).any():
        return float("inf"), float("nan"), False, g.size
    if un.all():
        return 0.0, 1.0, True, g.size
    worst, scale, ok = Fk.check(g[~un], r[~un], s[~un], tau)
    return worst, scale, ok, g.size


# ----------------------------------------------------------------------------------------------------------------------------------
# frames (sep_frames_kernel: m2h_sep_frames, _hop, _win)
# ----------------------------------------------------------------------------------------------------------------------------------
FRAMES_MUTANTS = ("edge sample repeated", "reflect about end instead of the segment", "g <= end", "hop ignored", "origin ignored", "channel stride L for cap")


def _frames_row(name, R, end, hop, s0, nseg, origin=0, cap=None, entry="ops"):
    win = cap is not None
    return dict(id="frames." + name, family="frames", R=R, end=end, hop=hop, s0=s0, nseg=nseg, origin=origin, cap=cap if win else end, win=win, entry=entry)


FRAMES_ROWS = [
    _frames_row("R2.L32001.hop16000.s0.n3", 2, 32001, 16000, 0, 3),
    _frames_row("R2.L32001.hop16000.s1.n2.cabi", 2, 32001, 16000, 1, 2, entry="m2h_sep_frames"),
    _frames_row("R3.L24001.hop8000.s1.n2", 3, 24001, 8000, 1, 2),
    _frames_row("R1.L9002.hop4000.s0.n3", 1, 9002, 4000, 0, 3),
    _frames_row("R1.L9002.hop4000.s2.n1", 1, 9002, 4000, 2, 1),
    _frames_row("R2.win.hop8000.o8000.cap20000.end25003.s1.n3", 2, 25003, 8000, 1, 3, origin=8000, cap=20000),
    _frames_row("R1.win.hop16000.o16000.cap16005.end23777.s1.n1", 1, 23777, 16000, 1, 1, origin=16000, cap=16005),
    _frames_row("R257.L15999.hop16000.s0.n1.big", 257, 15999, 16000, 0, 1),
]


def frames_total(row):
    return row["nseg"] * row["R"] * 2 * SEP_T * (SEP_LD // 4)


def frames_cells(row):
    hop, end, s0, nseg = row["hop"], row["end"], row["s0"], row["nseg"]
    out = {"hop %d" % hop, "reflect j < 0", "reflect j >= 16000", "second pass of the grid-stride loop" if second_pass(frames_total(row)) else "one item per thread",
           "entry " + ("m2h_sep_frames" if row["entry"] != "ops" else "m2h_sep_frames_win" if row["win"] else "m2h_sep_frames_hop")}
    if s0 > 0:
        out.add("s0 > 0")
    segs = range(s0, s0 + nseg)
    if any(s * hop + SEP_SEG < end for s in segs):
        out.add("reflect inside the segment although the recording goes on")
    if any(end - s * hop == 1 for s in segs):
        out.add("a last segment holding 1 sample")
    if any(0 < end - s * hop < SEP_SEG and (end - s * hop + 511) % SEP_HOP not in (0, 511) for s in segs):
        out.add("end in the middle of a frame")
    if row["cap"] % 4:
        out.add("channel rows misaligned")
    if row["win"] and row["origin"] > 0:
        out.add("window form with origin > 0")
    if row["win"] and row["cap"] > end - row["origin"]:
        out.add("cap > end - origin over a NaN tail")
    return out


def frames_all_cells():
    return {"hop 16000", "hop 8000", "hop 4000", "s0 > 0", "reflect j < 0", "reflect j >= 16000", "reflect inside the segment although the recording goes on",
            "a last segment holding 1 sample", "end in the middle of a frame", "channel rows misaligned", "window form with origin > 0",
            "cap > end - origin over a NaN tail", "second pass of the grid-stride loop", "one item per thread", "entry m2h_sep_frames", "entry m2h_sep_frames_hop",
            "entry m2h_sep_frames_win"}


def hann_window_fwd():
    """[1024]: periodic Hann(1023) and one zero."""
    return np.concatenate((Fk.hann_periodic(SEP_NFFT), np.zeros(1, dtype=F32)))


def frames_inputs(row):
    R, cap, held = row["R"], row["cap"], row["end"] - row["origin"]
    buf = np.full((R, 2, cap), np.nan, dtype=F32)            # at or past `end`: not the kernel's to use
    buf[:, :, :min(cap, held)] = _rng(row).standard_normal((R, 2, min(cap, held))).astype(F32)
    return dict(buf=buf, window=hann_window_fwd())


def _frames_values(row, inp, mutant=None):
    """float64 products [nseg, R, 2, 32, 1023] and the validity mask, by the kernel's index arithmetic."""
    R, cap, end, hop, s0, nseg, origin = (row[k] for k in ("R", "cap", "end", "hop", "s0", "nseg", "origin"))
    j = np.arange(SEP_T)[:, None] * SEP_HOP + np.arange(SEP_NFFT)[None, :] - SEP_NFFT // 2
    if mutant == FRAMES_MUTANTS[0]:
        j = np.where(j < 0, -j - 1, j)
        j = np.where(j >= SEP_SEG, 2 * SEP_SEG - 1 - j, j)
    else:
        j = np.where(j < 0, -j, j)
        if mutant != FRAMES_MUTANTS[1]:
            j = np.where(j >= SEP_SEG, 2 * (SEP_SEG - 1) - j, j)
    base = (s0 + np.arange(nseg)) * (SEP_SEG if mutant == FRAMES_MUTANTS[3] else hop)
    g = base[:, None, None] + j[None]
    if mutant == FRAMES_MUTANTS[1]:
        g = np.abs(np.where(g >= end, 2 * (end - 1) - g, g))
    valid = g <= end if mutant == FRAMES_MUTANTS[2] else g < end
    idx = g - (0 if mutant == FRAMES_MUTANTS[4] else origin)
    stride = end if mutant == FRAMES_MUTANTS[5] else cap
    flat = np.concatenate((inp["buf"].reshape(-1), np.ones(8, dtype=F32)))          # (what a mutant finds past the buffer)
    fi = np.clip(np.arange(2 * R)[:, None, None, None] * stride + idx[None], 0, flat.size - 1)
    with np.errstate(invalid="ignore"):
        prod = inp["window"][:SEP_NFFT].astype(np.float64) * flat[fi].astype(np.float64)       # exact in float64: 24 + 24 bits
    prod = np.where(valid[None], prod, 0.0).astype(F32)
    return np.ascontiguousarray(prod.reshape(R, 2, nseg, SEP_T, SEP_NFFT).transpose(2, 0, 1, 3, 4))


def frames_fp32(row, inp, mutant=None):
    out = np.zeros((row["nseg"], row["R"], 2, SEP_T, SEP_LD), dtype=F32)
    out[..., :SEP_NFFT] = _frames_values(row, inp, mutant)
    return {"frames": out}


def frames_reference(row, inp):
    """(float32 holds the exact reference exactly: the rounded product)"""
    return {"frames": (frames_fp32(row, inp)["frames"], 0.0)}


# ----------------------------------------------------------------------------------------------------------------------------------
# post (sep_stft_post_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
POST_MUTANTS = ("no scaling by big", "guard yields (0, 0)", "phasor of channel 0 alone", "channels swapped in the magnitude", "t / k transposed")
# (re0, im0, re1, im1): components near 1e37 and 1e-37 (normal numbers, equal signs within a component: the downmix stays normal and finite),
# exact-zero downmixes of non-zero channels, zeros
POST_PLANTS = ((1e37, -2e37, 3e37, -1e37), (-2e37, 1e30, -1e37, 2e30), (1e-37, 2e-37, 2e-37, 1e-37), (-3e-37, 0.0, -1e-37, 0.0), (0.0, 2e-37, 0.0, 1e-37),
               (1.5, -2.5, -1.5, 2.5), (3e-3, 4.0, -3e-3, -4.0), (0.0, 0.0, 0.0, 0.0), (-0.0, 0.0, 0.0, -0.0), (2.0, 0.0, 1.0, 0.0), (0.0, -3.0, 0.0, -1.0),
               (1e37, 1e-37, 1e37, 1e-37), (6e18, 6e18, 6e18, 6e18), (1e-20, 1e-20, 2e-20, 3e-20), (-1.0, 1e-30, -1.0, 1e-30), (1e19, 0.0, -1e19, 3.0))
POST_ROWS = [dict(id="post.N%d" % N, family="post", N=N) for N in (1, 3)]
F32_SQRT_MAX = 2.0 ** 64


def post_plant_sites(N):
    """Plant p goes to bin tile p mod 16 of the last batch row: twice over the 16 tiles."""
    return [(N - 1, SEP_KT * (p % 16) + (7 * p) % SEP_KT, (5 * p + 3) % SEP_T, POST_PLANTS[p % len(POST_PLANTS)]) for p in range(32)]


def post_cells(row):
    """(from the inputs themselves: a plant that another overwrote, or a builder that changed, shows here)"""
    N = row["N"]
    re, im = _post_parts(post_inputs(row)["spec"], N, np.float64)          # [N, 2, 32, 512]
    out = {"N=%d" % N}
    if ((re == 0) & (im == 0)).all(axis=(1, 3)).any():
        out.add("all-zero frames")
    dz = (re[:, 0] + re[:, 1] == 0) & (im[:, 0] + im[:, 1] == 0)
    nz = ((re != 0) | (im != 0)).all(axis=1)
    if (dz & nz).any():
        out.add("exact-zero downmix of non-zero channels")
    mx = np.maximum(np.abs(re[:, 0] + re[:, 1]), np.abs(im[:, 0] + im[:, 1]))
    for name, lo, hi in (("components near 1e37", 1e36, 1e38), ("components near 1e-37", 1e-38, 1e-36)):
        hit = (mx >= lo) & (mx <= hi)
        if hit.any():
            out.add(name)
    bre, bim = _post_parts(post_inputs(row, plants=False)["spec"], N, np.float64)          # what the bins held before the plants
    planted = ((re != bre) | (im != bim)).any(axis=1)
    return out | {"plants in bin tile %d" % (k // SEP_KT) for k in np.unique(np.nonzero(planted)[2])}


def post_all_cells():
    return {"N=1", "N=3", "all-zero frames", "exact-zero downmix of non-zero channels", "components near 1e37", "components near 1e-37"} | \
           {"plants in bin tile %d" % i for i in range(16)}


def post_inputs(row, plants=True):
    N = row["N"]
    spec = _rng(row).standard_normal((N, 2, SEP_T, SEP_LD)).astype(F32)
    spec[0, :, 1] = 0                                           # an all-zero frame in both channels
    spec[N - 1, :, SEP_T - 1] = 0
    for n, k, t, (re0, im0, re1, im1) in post_plant_sites(N) if plants else ():
        if t in (1, SEP_T - 1):
            t = 2
        spec[n, 0, t, k], spec[n, 0, t, SEP_NB + k], spec[n, 1, t, k], spec[n, 1, t, SEP_NB + k] = re0, im0, re1, im1
    return dict(spec=spec.reshape(N * 2 * SEP_T, SEP_LD))


def _post_parts(spec, N, dtype):
    sp = spec.reshape(N, 2, SEP_T, SEP_LD).astype(dtype)
    return sp[..., :SEP_NB], sp[..., SEP_NB:]                    # [N, 2, 32, 512]


def _nktc(a, transposed=False):
    """[N, C, 32, 512] -> [N, 512, 32, C]"""
    if transposed:      # MUTANT: [N, 32, 512, C] behind the same shape
        return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(a.shape[0], SEP_NB, SEP_T, a.shape[1])
    return np.ascontiguousarray(a.transpose(0, 3, 2, 1))


def post_reference(row, inp):
    N, tau = row["N"], TAU["post"]
    re, im = _post_parts(inp["spec"], N, np.float64)
    m = np.hypot(re, im)
    over = m >= F32_SQRT_MAX
    s_m = m + Fk.underflow_slack(m) / tau
    r_mag = np.log1p(m)
    s_mag = s_m / (1 + m) + r_mag
    dr, di = re[:, 0] + re[:, 1], im[:, 0] + im[:, 1]
    h = np.hypot(dr, di)
    zero = h == 0
    hs = np.where(zero, 1.0, h)
    ph = np.stack((np.where(zero, 1.0, dr / hs), np.where(zero, 0.0, di / hs)), 1)      # [N, 2 (re, im), 32, 512]
    s_ph = np.broadcast_to(np.where(zero, 0.0, 1.0)[:, None], ph.shape)
    return {"mag": (_nktc(r_mag), _nktc(s_mag), _nktc(over)), "phasor": (_nktc(ph), _nktc(np.ascontiguousarray(s_ph)))}


def post_fp32(row, inp, mutant=None):
    N = row["N"]
    re, im = _post_parts(inp["spec"], N, F32)
    with np.errstate(all="ignore"):
        m = np.log1p(np.sqrt(re * re + im * im)).astype(F32)
        if mutant == POST_MUTANTS[3]:
            m = m[:, ::-1]
        if mutant == POST_MUTANTS[2]:
            dr, di = re[:, 0].copy(), im[:, 0].copy()
        else:
            dr, di = re[:, 0] + re[:, 1], im[:, 0] + im[:, 1]
        big = np.maximum(np.abs(dr), np.abs(di))
        zero = big == 0
        if mutant != POST_MUTANTS[0]:
            bs = np.where(zero, F32(1), big)
            dr, di = dr / bs, di / bs
        inv = F32(1) / np.sqrt(dr * dr + di * di)
        pr, pi = dr * inv, di * inv
        g0 = F32(0) if mutant == POST_MUTANTS[1] else F32(1)
        ph = np.stack((np.where(zero, g0, pr), np.where(zero, F32(0), pi)), 1).astype(F32)
    tr = mutant == POST_MUTANTS[4]
    return {"mag": _nktc(m, tr), "phasor": _nktc(ph, tr)}


# ----------------------------------------------------------------------------------------------------------------------------------
# pre (sep_istft_pre_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
PRE_MUTANTS = ("clamp missing", "re / im swapped", "row stride 512")
PRE_ROWS = [dict(id="pre.N%d%s" % (N, ".out" if o else ""), family="pre", N=N, out=o) for N, o in ((1, False), (3, False), (3, True))]
PRE_PLANTS = (-3.0, -1e-30, 0.0, -0.0, 1e-30, 1e-6, 1.0, 12.5, 20.0)


def pre_cells(row):
    P = pre_inputs(row)["P"]
    out = {"N=%d" % row["N"], "out= given" if row["out"] else "out allocated"}
    if (P < 0).any():
        out.add("negative P")
    if (P == 0).any():
        out.add("zero P")
    if float(P.max()) == 20.0:
        out.add("P up to 20")
    return out


def pre_all_cells():
    return {"N=1", "N=3", "out= given", "out allocated", "negative P", "zero P", "P up to 20"}


def pre_inputs(row):
    g = _rng(row)
    N = row["N"]
    P = (3 * g.standard_normal((N, SEP_NB, SEP_T, 1))).astype(F32)
    P.reshape(-1)[:len(PRE_PLANTS)] = PRE_PLANTS
    P.reshape(-1)[-len(PRE_PLANTS):] = PRE_PLANTS
    a = g.uniform(-np.pi, np.pi, (N, SEP_NB, SEP_T))
    phasor = np.stack((np.cos(a), np.sin(a)), -1).astype(F32)
    return dict(P=P, phasor=phasor)


def _pre_rows(mre, mim, stride=SEP_LD):
    """[N, 512, 32] products -> rows [N 32, 1024] (a buffer of NaN, written at the row stride)"""
    N = mre.shape[0]
    flat = np.full(N * SEP_T * SEP_LD, np.nan, dtype=mre.dtype)
    at = (np.arange(N * SEP_T) * stride)[:, None] + np.arange(SEP_NB)[None, :]
    flat[at] = mre.transpose(0, 2, 1).reshape(N * SEP_T, SEP_NB)
    flat[at + SEP_NB] = mim.transpose(0, 2, 1).reshape(N * SEP_T, SEP_NB)
    return flat.reshape(N * SEP_T, SEP_LD)


def pre_reference(row, inp):
    P, ph = inp["P"][..., 0].astype(np.float64), inp["phasor"].astype(np.float64)
    m = np.expm1(np.maximum(P, 0.0))
    r = _pre_rows(m * ph[..., 0], m * ph[..., 1])
    return {"rows": (r, np.abs(r))}


def pre_fp32(row, inp, mutant=None):
    P, ph = inp["P"][..., 0], inp["phasor"]
    with np.errstate(all="ignore"):
        m = np.expm1(P if mutant == PRE_MUTANTS[0] else np.maximum(P, F32(0))).astype(F32)
    re, im = (ph[..., 1], ph[..., 0]) if mutant == PRE_MUTANTS[1] else (ph[..., 0], ph[..., 1])
    return {"rows": _pre_rows((m * re).astype(F32), (m * im).astype(F32), SEP_NB if mutant == PRE_MUTANTS[2] else SEP_LD)}


# ----------------------------------------------------------------------------------------------------------------------------------
# bin_rows (sep_bin_rows_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
BIN_MUTANTS = ("other channel's mask", "clamp missing", "t / k transposed")
BIN_ROWS = [dict(id="bin_rows.N%d.%s" % (N, "inplace" if ip else "out"), family="bin_rows", N=N, inplace=ip) for N, ip in ((1, True), (1, False), (3, True), (3, False))]


def bin_cells(row):
    out = {"N=%d" % row["N"], "in place" if row["inplace"] else "out of place"}
    if (bin_inputs(row)["masks"] < 0).any():
        out.add("negative masks")
    return out


def bin_all_cells():
    return {"N=1", "N=3", "in place", "out of place", "negative masks"}


def bin_inputs(row):
    g = _rng(row)
    N = row["N"]
    masks = g.standard_normal((N, SEP_NB, SEP_T, 2)).astype(F32)              # half of them negative
    masks.reshape(-1)[:3] = (0.0, -0.0, -1e-30)
    return dict(spec=g.standard_normal((N * 2 * SEP_T, SEP_LD)).astype(F32), masks=masks)


def bin_fp32(row, inp, mutant=None):
    N = row["N"]
    mk = inp["masks"]
    if mutant == BIN_MUTANTS[2]:
        mk = mk.reshape(N, SEP_T, SEP_NB, 2).transpose(0, 2, 1, 3)
    if mutant == BIN_MUTANTS[0]:
        mk = mk[..., ::-1]
    if mutant != BIN_MUTANTS[1]:
        mk = np.maximum(mk, F32(0))
    mk = np.ascontiguousarray(mk.transpose(0, 3, 2, 1))                         # [N, c, t, k]
    sp = inp["spec"].reshape(N, 2, SEP_T, 2, SEP_NB)
    return {"rows": (mk[:, :, :, None, :] * sp).astype(F32).reshape(N * 2 * SEP_T, SEP_LD)}


def bin_reference(row, inp):
    return {"rows": (bin_fp32(row, inp)["rows"], 0.0)}


# ----------------------------------------------------------------------------------------------------------------------------------
# ola (sep_ola_sample, sep_istft_ola_kernel: m2h_sep_istft_ola, _win)
# ----------------------------------------------------------------------------------------------------------------------------------
OLA_MUTANTS = ("t1 unclamped", "n > 1022 as the break", "s0 ignored", "store past L", "origin ignored")
OLA_BLOCK = 64      # batch rows per block of a reference evaluation


def ola_core(fr, w, dtype, mutant=None):
    """sep_ola_sample over every j of every batch row.  fr [B, 32, 1024], w [1022] -> (acc, wss, sum (f w)^2) [B, 16000] in `dtype`: step k
    takes frame t1 - k, as the kernel's loop."""
    B = fr.shape[0]
    jj = np.arange(SEP_SEG) + SEP_NIFFT // 2
    t1 = jj // SEP_HOP
    if mutant != OLA_MUTANTS[0]:
        t1 = np.minimum(t1, SEP_T - 1)
    # one frame and two window samples past the end, for the mutants that read them: the next batch row's first frame, 0.5 for the window
    frx = np.concatenate((fr.reshape(B * SEP_T, SEP_LD), np.ones((1, SEP_LD), dtype=fr.dtype)), 0)
    wx = np.concatenate((np.asarray(w[:SEP_NIFFT]), [0.5, 0.5])).astype(dtype)
    acc, wss, q = (np.zeros((B, SEP_SEG), dtype=dtype) for _ in range(3))
    live = np.ones(SEP_SEG, dtype=bool)
    z = np.zeros((), dtype=dtype)
    for k in range(3):
        t = t1 - k
        n = jj - t * SEP_HOP
        live = live & (t >= 0) & ((n <= SEP_NIFFT) if mutant == OLA_MUTANTS[1] else (n < SEP_NIFFT))
        if not live.any():
            break
        tc, nc = np.clip(t, 0, SEP_T), np.clip(n, 0, SEP_NIFFT + 1)
        with np.errstate(invalid="ignore"):
            f = frx[(np.arange(B)[:, None] * SEP_T + tc[None, :]), nc[None, :]].astype(dtype)
            wv = wx[nc][None, :]
            p = f * wv
            acc = acc + np.where(live[None, :], p, z)
            wss = wss + np.where(live[None, :], wv * wv, z)
            q = q + np.where(live[None, :], p * p, z)
    return acc, wss, q


def ola_values(fr, w, dtype, mutant=None):
    """(v, s_ola) [B, 16000]: the segment's inverse transform and, in float64, its error scale."""
    acc, wss, q = ola_core(fr, w, dtype, mutant)
    div = wss > dtype(TINY)
    with np.errstate(all="ignore"):
        v = np.where(div, acc / np.where(div, wss, dtype(1)), acc).astype(dtype)
    if dtype is F32:
        return v, None
    return v, np.sqrt(q) / np.where(div, wss, 1.0) + np.abs(v)


def frames_per_sample():
    """How many frames cover sample j of a segment (1 or 2), from the kernel's loop."""
    _, wss, _ = ola_core(np.ones((1, SEP_T, SEP_LD)), np.ones(SEP_NIFFT), np.float64)
    return wss[0].astype(int)


def _ola_row(name, R, end, calls, origin=0, cap=None, wzero=False):
    win = cap is not None
    return dict(id="ola." + name, family="ola", R=R, end=end, calls=calls, origin=origin, cap=cap if win else end, win=win, wzero=wzero)


OLA_ROWS = [
    _ola_row("R2.L32000", 2, 32000, ((0, 2),)),
    _ola_row("R3.L32001.two_calls", 3, 32001, ((0, 1), (1, 2))),
    _ola_row("R2.L17002", 2, 17002, ((0, 2),)),
    _ola_row("R2.L4003", 2, 4003, ((0, 1),)),
    _ola_row("R2.win.o16000.cap16010.end31999", 2, 31999, ((1, 1),), origin=16000, cap=16010),
    _ola_row("R1.L16000.wzero", 1, 16000, ((0, 1),), wzero=True),
    _ola_row("R1049.L16000.big", 1049, 16000, ((0, 1),)),
]


def ola_total(row, call):
    return call[1] * row["R"] * (SEP_SEG // 4)


def _ola_reaches_t1_clamp(row):
    return any(row["end"] - (s0 + nseg - 1) * SEP_SEG > SEP_T * SEP_HOP - SEP_NIFFT // 2 or nseg > 1 for s0, nseg in row["calls"])


def ola_cells(row):
    end, cap, R = row["end"], row["cap"], row["R"]
    out = {"L %% 4 = %d" % (end % 4), "samples one frame covers", "samples two frames cover",
           "second pass of the grid-stride loop" if any(second_pass(ola_total(row, c)) for c in row["calls"]) else "one item per thread"}
    if R > 1 and cap % 4:
        out.add("scalar store path on rows r >= 1")
    if end % 4:
        out.add("the quad that straddles L")
    if len(row["calls"]) > 1 and row["calls"][-1][0] > 0:
        out.add("s0 > 0 in a second call")
    if row["wzero"]:
        out.add("the wss guard")
    if row["win"] and row["origin"] > 0:
        out.add("window form with origin > 0")
    if _ola_reaches_t1_clamp(row):
        out.add("t1 clamped")
    return out


def ola_all_cells():
    return {"L % 4 = 0", "L % 4 = 1", "L % 4 = 2", "L % 4 = 3", "samples one frame covers", "samples two frames cover", "second pass of the grid-stride loop",
            "one item per thread", "scalar store path on rows r >= 1", "the quad that straddles L", "s0 > 0 in a second call", "the wss guard",
            "window form with origin > 0", "t1 clamped"}


def hann_window_inv(wzero=False):
    w = Fk.hann_periodic(SEP_NIFFT)
    if wzero:
        w[510], w[511] = 1e-20, 0.0
    return w


def _inverse_rows(g, B):
    """The inverse GEMM's rows [B, 32, 1024]; columns 1022 and 1023 are not the kernel's to read."""
    fr = np.full((B, SEP_T, SEP_LD), np.nan, dtype=F32)
    fr[:, :, :SEP_NIFFT] = g.standard_normal((B, SEP_T, SEP_NIFFT), dtype=F32)
    return fr


def ola_inputs(row):
    g = _rng(row)
    return dict(frames=[_inverse_rows(g, nseg * row["R"]) for _, nseg in row["calls"]], window=hann_window_inv(row["wzero"]))


def _ola_place(row, call, v, y, mutant=None):
    """Writes the call's segments v [nseg, nr, 16000] into y [nr, cap] as the kernel's stores do."""
    s0, nseg = call
    end, origin, cap = row["end"], row["origin"], row["cap"]
    nr = y.shape[0]
    flat = np.concatenate((y.reshape(-1), np.full(4, np.nan, dtype=y.dtype)))
    for sl in range(nseg):
        start = (sl if mutant == OLA_MUTANTS[2] else s0 + sl) * SEP_SEG
        stop = min(start + SEP_SEG, start + cdiv(max(end - start, 0), 4) * 4 if mutant == OLA_MUTANTS[3] else end)
        if stop <= start:
            continue
        pos = np.arange(start, stop) - (0 if mutant == OLA_MUTANTS[4] else origin)
        ok = (pos >= 0) & (pos < cap + 4)
        for r in range(nr):
            at = r * cap + pos[ok]
            at_ok = at < flat.size
            flat[at[at_ok]] = v[sl, r, :stop - start][ok][at_ok]
    y[...] = flat[:nr * cap].reshape(nr, cap)


def _ola_run(row, inp, dtype, mutant=None, rsel=None):
    R = row["R"]
    rsel = slice(0, R) if rsel is None else rsel
    nr = len(range(*rsel.indices(R)))
    y, s = np.full((nr, row["cap"]), np.nan, dtype=dtype), np.full((nr, row["cap"]), np.nan)
    for call, fr in zip(row["calls"], inp["frames"]):
        fr = fr.reshape(call[1], R, SEP_T, SEP_LD)[:, rsel].reshape(call[1] * nr, SEP_T, SEP_LD)
        v, sv = ola_values(fr, inp["window"], dtype, mutant)
        _ola_place(row, call, v.reshape(call[1], nr, SEP_SEG), y, mutant)
        if sv is not None:
            _ola_place(row, call, sv.reshape(call[1], nr, SEP_SEG), s)
    return y, s


def ola_reference(row, inp, rsel=None):
    y, s = _ola_run(row, inp, np.float64, None, rsel)
    return {"y": (y, np.where(np.isnan(s), 0.0, s))}


def ola_fp32(row, inp, mutant=None, rsel=None):
    return {"y": _ola_run(row, inp, F32, mutant, rsel)[0]}


# ----------------------------------------------------------------------------------------------------------------------------------
# xfade (sep_istft_xfade_kernel: m2h_sep_istft_xfade, _win)
# ----------------------------------------------------------------------------------------------------------------------------------
XF_MUTANTS = ("W over the chunk's segments only", "b unclamped", "prior partial ignored", "prior partial always read", "xwin without the division")


def _xf_row(name, R, hop, calls, cap=None):
    """calls: (s0, nseg, origin, end) in ascending order; a whole-recording row has origin 0 and one `end` = L = cap."""
    win = cap is not None
    return dict(id="xfade." + name, family="xfade", R=R, hop=hop, calls=calls, cap=cap if win else calls[0][3], win=win)


XF_ROWS = [
    _xf_row("R2.hop8000.L24001.two_chunks", 2, 8000, ((0, 2, 0, 24001), (2, 2, 0, 24001))),
    _xf_row("R1.hop4000.L13003.two_chunks", 1, 4000, ((0, 3, 0, 13003), (3, 1, 0, 13003))),
    _xf_row("R3.hop4000.L13003.three_chunks", 3, 4000, ((0, 1, 0, 13003), (1, 2, 0, 13003), (3, 1, 0, 13003))),
    _xf_row("R2.hop8000.L5002", 2, 8000, ((0, 1, 0, 5002),)),
    _xf_row("R2.hop4000.L3999", 2, 4000, ((0, 1, 0, 3999),)),
    _xf_row("R2.win.hop8000.cap24006.feed", 2, 8000, ((0, 2, 0, 24000), (2, 2, 8000, 30001)), cap=24006),
    _xf_row("R1049.hop4000.L16000.big", 1049, 4000, ((0, 1, 0, 16000),)),
]


def xf_span(row, call):
    s0, nseg, origin, L = call
    return s0 * row["hop"], min((s0 + nseg - 1) * row["hop"] + SEP_SEG, L)


def xf_total(row, call):
    lo, hi = xf_span(row, call)
    return cdiv(hi - lo, 4) * row["R"]


def _xf_cover(row, call, n):
    hop, L = row["hop"], call[3]
    a = np.where(n < SEP_SEG, 0, (n - SEP_SEG) // hop + 1)
    return a, n // hop, cdiv(L, hop)


def xf_cells(row):
    hop = row["hop"]
    out = {"hop %d" % hop, "second pass of the grid-stride loop" if any(second_pass(xf_total(row, c)) for c in row["calls"]) else "one item per thread"}
    for ci, call in enumerate(row["calls"]):
        lo, hi = xf_span(row, call)
        n = np.arange(lo, hi)
        a, b, S = _xf_cover(row, call, n)
        for c in np.unique(np.minimum(b, S - 1) - a + 1):
            out.add("a sample covered by %d segments" % c)
        if (a < call[0]).any():
            out.add("a < s0 reads the prior partial")
        if (a >= call[0]).any():
            out.add("a >= s0 must not read (NaN sentinel)")
        if call[3] % 4:
            out.add("L % 4 != 0")
        if call[3] < hop:
            out.add("L < hop: one segment")
        if cdiv(call[3], hop) * hop - call[3] > 0 and (call[0] + call[1]) == cdiv(call[3], hop) and call[3] - (call[0] + call[1] - 1) * hop < SEP_SEG:
            out.add("a short last segment")
        if row["win"] and ci > 0 and call[2] > row["calls"][ci - 1][2]:
            out.add("window form keeping partial sums across two calls with the origin advanced")
    if row["R"] > 1 and row["cap"] % 4:
        out.add("scalar path on rows r >= 1")
    return out


def xf_all_cells():
    return {"hop 8000", "hop 4000", "second pass of the grid-stride loop", "one item per thread", "a < s0 reads the prior partial", "a >= s0 must not read (NaN sentinel)",
            "L % 4 != 0", "L < hop: one segment", "a short last segment", "window form keeping partial sums across two calls with the origin advanced",
            "scalar path on rows r >= 1"} | {"a sample covered by %d segments" % c for c in (1, 2, 3, 4)}


def crossfade_window():
    from m2h.separate import crossfade_window as cw
    return np.ascontiguousarray(cw(), dtype=F32)


def xf_inputs(row):
    g = _rng(row)
    return dict(frames=[_inverse_rows(g, c[1] * row["R"]) for c in row["calls"]], window=hann_window_inv(), xwin=crossfade_window())


def xf_prior(row, ci, y_prev):
    """The y [.., cap] handed to call ci, from what call ci - 1 left: NaN before the first call; shifted where the window's origin advanced
    (the feed's own move: sample n stays at n - origin), NaN in what the shift uncovers."""
    if ci == 0:
        return np.full(np.shape(y_prev), np.nan, dtype=F32)
    shift = row["calls"][ci][2] - row["calls"][ci - 1][2]
    if shift == 0:
        return np.array(y_prev, dtype=F32)
    out = np.full(np.shape(y_prev), np.nan, dtype=F32)
    out[:, :row["cap"] - shift] = np.asarray(y_prev)[:, shift:]
    return out


def _xf_call(row, inp, ci, y_prior, dtype, mutant=None, rsel=None):
    """One call on y_prior [nr, cap] (float32 values) -> (y, s) [nr, cap] in `dtype`, the kernel's order of additions."""
    R, hop, cap = row["R"], row["hop"], row["cap"]
    s0, nseg, origin, L = row["calls"][ci]
    rsel = slice(0, R) if rsel is None else rsel
    nr = len(range(*rsel.indices(R)))
    lo, hi = xf_span(row, row["calls"][ci])
    n = np.arange(lo, hi)
    a, b, S = _xf_cover(row, row["calls"][ci], n)
    if mutant != XF_MUTANTS[1]:
        b = np.minimum(b, S - 1)
    xw = inp["xwin"].astype(dtype)
    z = np.zeros((), dtype=dtype)
    W = np.zeros(n.size, dtype=dtype)
    for s in range(int(a.min()), int(b.max()) + 1):
        m = (a <= s) & (s <= b)
        if mutant == XF_MUTANTS[0]:
            m = m & (s0 <= s) & (s < s0 + nseg)
        W = W + np.where(m, xw[np.clip(n - s * hop, 0, SEP_SEG - 1)], z)
    fr = inp["frames"][ci].reshape(nseg, R, SEP_T, SEP_LD)[:, rsel].reshape(nseg * nr, SEP_T, SEP_LD)
    v, sv = ola_values(fr, inp["window"], dtype)
    v = v.reshape(nseg, nr, SEP_SEG)
    prior = np.asarray(y_prior)[:, n - origin].astype(dtype)
    read = np.zeros(n.size, bool) if mutant == XF_MUTANTS[2] else np.ones(n.size, bool) if mutant == XF_MUTANTS[3] else a < s0
    with np.errstate(all="ignore"):
        acc = np.where(read[None], prior, z)
        sc = np.where(read[None], np.abs(prior), 0.0).astype(np.float64)
        for s in range(s0, s0 + nseg):
            m = (np.maximum(a, s0) <= s) & (s <= np.minimum(b, s0 + nseg - 1))
            j = np.clip(n - s * hop, 0, SEP_SEG - 1)
            wgt = xw[j] if mutant == XF_MUTANTS[4] else (xw[j] / W).astype(dtype)
            acc = acc + np.where(m[None], (v[s - s0][:, j] * wgt[None]).astype(dtype), z)
            if sv is not None:
                sc = sc + np.where(m[None], sv.reshape(nseg, nr, SEP_SEG)[s - s0][:, j] * wgt[None], 0.0)
    y = np.asarray(y_prior).astype(dtype).copy()
    s_out = np.zeros(y.shape)
    y[:, n - origin] = acc
    s_out[:, n - origin] = sc + np.abs(acc.astype(np.float64))
    return y, s_out


def xf_reference_call(row, inp, ci, y_prior, rsel=None):
    """{"y": (r, s)} of call ci from the float32 y it was handed: what the call does not write keeps its value (s = 0) or its NaN."""
    y, s = _xf_call(row, inp, ci, y_prior, np.float64, None, rsel)
    return {"y": (y, np.where(np.isnan(y), 0.0, s))}


def xf_fp32_call(row, inp, ci, y_prior, mutant=None, rsel=None):
    return {"y": _xf_call(row, inp, ci, y_prior, F32, mutant, rsel)[0]}


# ----------------------------------------------------------------------------------------------------------------------------------
# resample (resample_tile_kernel<NPT, UP1>, resample_direct_kernel: m2h_resample_poly, _win)
# ----------------------------------------------------------------------------------------------------------------------------------
RS_MUTANTS = ("one tap dropped", "taps shifted by one", "half omitted from t", "j < end missing", "row isolation missing", "cnt off by one at the seam",
              "lead count wrong", "origin ignored")


def rs_table_floats(up, T):
    return 0 if up == 1 else T * (up | 1)


def rs_span_floats(tile, up, down, T):
    span = ((tile - 1) * down + up - 1) // up + T
    return (span + 3 + 3) // 4 * 4


def rs_choice(up, down, T):
    """rs_run's search: (outputs per tile, LDS bytes) of the largest tile whose table and span fit, 8 -> 1 outputs per thread; (0, 0): direct."""
    table_floats = (rs_table_floats(up, T) + 3) // 4 * 4
    for c in (8, 4, 2, 1):
        tile = RS_THREADS * c
        f = max(table_floats + rs_span_floats(tile, up, down, T), tile)
        if f * 4 <= RS_LDS_BYTES:
            return tile, f * 4
    return 0, 0


def rs_design(f_in, f_out):
    """(up, down, half, T, G float32 [up, T]) as m2h.audio.resample.Resampler builds them."""
    from m2h.audio import resample as R
    up, down, half, h = R.design(f_in, f_out)
    return up, down, half, R.taps_per_output(up, down), R.polyphase_table(h.astype(F32), up)


def rs_kernel(row):
    up, down, half, T, _ = rs_design(row["f_in"], row["f_out"])
    tile, _ = rs_choice(up, down, T)
    return ("direct" if tile == 0 else "tile %d" % tile, "one phase" if up == 1 else "table")


def _rs_row(name, f_in, f_out, rows, L_in, xoff=0, yoff=0, win=None, nan_rows=False):
    """win: (origin, cap, end, n_first, count)"""
    from m2h.audio import resample as R
    up, down = R.ratio(f_in, f_out)
    if win is None:
        origin, cap, end, n_first, count = 0, L_in, L_in, 0, R.output_length(L_in, up, down)
    else:
        origin, cap, end, n_first, count = win
    return dict(id="resample.%d-%d.%s" % (f_in, f_out, name), family="resample", f_in=f_in, f_out=f_out, rows=rows, origin=origin, cap=cap, end=end, n_first=n_first,
                count=count, xoff=xoff, yoff=yoff, win=win is not None, nan_rows=nan_rows)


def _rs_two_tiles(f_in, f_out, extra, rows=2, **kw):
    """A row whose L_out is two tiles and `extra` outputs (direct kernel, which has no tile and no seam: one block of 256 and `extra`)."""
    from m2h.audio import resample as R
    up, down = R.ratio(f_in, f_out)
    tile = rs_choice(up, down, R.taps_per_output(up, down))[0]
    want = 2 * tile + extra if tile else RS_THREADS + extra
    L_in = ((want - 1) * down) // up + 1
    while R.output_length(L_in, up, down) < want:
        L_in += 1
    assert R.output_length(L_in, up, down) == want, (f_in, f_out, L_in, want)
    return _rs_row("two_tiles+%d%s" % (extra, "".join(".%s%s" % (k, v) for k, v in sorted(kw.items()))), f_in, f_out, rows, L_in, **kw)


# every tile size with one phase and with a table, and the direct kernel (tests/test_separator_kernels_cpu.py proves the choice from rs_choice)
RS_KERNEL_RATIOS = {("tile 2048", "one phase"): (48000, 16000), ("tile 1024", "one phase"): (128000, 16000), ("tile 512", "one phase"): (256000, 16000),
                    ("tile 256", "one phase"): (512000, 16000), ("tile 2048", "table"): (44100, 16000), ("tile 1024", "table"): (32000, 3000),
                    ("tile 512", "table"): (64000, 3000), ("tile 256", "table"): (128000, 3000), ("direct", "one phase"): (1000, 1), ("direct", "table"): (1023, 1000)}


def _rs_rows():
    rows = []
    for i, (k, (f_in, f_out)) in enumerate(sorted(RS_KERNEL_RATIOS.items())):
        rows.append(_rs_two_tiles(f_in, f_out, 1 + i % 3, xoff=i % 4, yoff=(i + 1) % 4))         # cnt of the last tile in 1..3, views off the 16-byte grid
    rows += [
        _rs_two_tiles(44100, 16000, 7, rows=3, nan_rows=True),
        _rs_two_tiles(48000, 16000, 5, rows=3, nan_rows=True, xoff=1, yoff=3),
        _rs_two_tiles(16000, 44100, 6, rows=2, xoff=2, yoff=1),
        _rs_two_tiles(1000, 1023, 2, rows=3, nan_rows=True, yoff=2),
        _rs_row("tiny.rows1.L5", 48000, 16000, 1, 5, xoff=1),                                     # rows * L_in < 8: no wide slot; L_in < T
        _rs_row("tiny.rows2.L3", 44100, 16000, 2, 3, xoff=3, yoff=1),                             # (one whole slot: have_wide, both ends clamped)
        _rs_row("tiny.rows2.L3.nowide", 44100, 16000, 2, 3, xoff=1, yoff=2),
        _rs_row("short.rows3.L30", 44100, 16000, 3, 30, yoff=3),                                  # L_in < T = 56
        _rs_row("win", 44100, 16000, 2, None, xoff=1, yoff=2, win=(5000, 9001, 13003, 2500, 2218)),
        _rs_row("win", 48000, 16000, 3, None, xoff=2, yoff=1, win=(3001, 7000, 9002, 1100, 1901), nan_rows=True),
        _rs_row("win", 1000, 1023, 2, None, yoff=1, win=(700, 1203, 1500, 900, 635)),
    ]
    return rows


def rs_have_wide(row):
    """resample_tile_kernel's have_wide: a whole 16-byte slot of the address grid lies inside the buffer (the view starts xoff floats past the
    grid: an allocation starts on it)."""
    fmin, fmax = (row["xoff"] + 3) >> 2, ((row["xoff"] + row["rows"] * row["cap"]) >> 2) - 1
    return fmin <= fmax


def rs_lead(row, r, tile):
    """The scalar head of row r's last tile before cnt cuts it: floats up to the destination's next 16-byte boundary."""
    last0 = (cdiv(row["count"], tile) - 1) * tile
    return (4 - (row["yoff"] + r * row["count"] + last0) % 4) % 4


def rs_cells(row):
    up, down, half, T, _ = rs_design(row["f_in"], row["f_out"])
    tile = rs_choice(up, down, T)[0]
    out = {rs_kernel(row)}
    if tile:
        tiles = cdiv(row["count"], tile)
        last = row["count"] - (tiles - 1) * tile
        if tiles >= 3:
            out.add("outputs TILE-1 and TILE and a last tile with cnt < TILE")
        if last <= 3 and any(rs_lead(row, r, tile) > last for r in range(row["rows"])):
            out.add("cnt in 1..3, below the store lead")
        if not rs_have_wide(row):
            assert row["rows"] * row["cap"] < 8
            out.add("rows * L_in < 8: no wide slot")
        if row["xoff"] % 4 or row["yoff"] % 4:
            out.add("views off the 16-byte grid")
    if row["cap"] % 4 and row["count"] % 4 and row["rows"] >= 2:
        out.add("L_in % 4 != 0 and L_out % 4 != 0 with at least 2 rows")
    if row["end"] < T:
        out.add("L_in shorter than T")
    if row["win"]:
        assert row["origin"] > 0 and row["n_first"] > 0 and row["end"] < row["origin"] + row["cap"]
        out.add("window form: origin > 0, n_first > 0%s, end < origin + cap over NaN" % (" and no multiple of the tile" if tile and row["n_first"] % tile else ""))
    if row["nan_rows"]:
        out.add("NaN neighbour rows")
    return out


def rs_all_cells():
    return set(RS_KERNEL_RATIOS) | {"outputs TILE-1 and TILE and a last tile with cnt < TILE", "cnt in 1..3, below the store lead", "rows * L_in < 8: no wide slot", "views off the 16-byte grid",
                                    "L_in % 4 != 0 and L_out % 4 != 0 with at least 2 rows", "L_in shorter than T", "NaN neighbour rows",
                                    "window form: origin > 0, n_first > 0 and no multiple of the tile, end < origin + cap over NaN",
                                    "window form: origin > 0, n_first > 0, end < origin + cap over NaN"}


RS_PAD = 8      # floats of the allocation after the view


def rs_inputs(row):
    """x_alloc [xoff + rows cap + RS_PAD]: the view x = x_alloc[xoff : xoff + rows cap]; NaN around the view, at or past `end`, and in the
    neighbour rows (0 and 2 of 3) of an isolation row."""
    g = _rng(row)
    up, down, half, T, G = rs_design(row["f_in"], row["f_out"])
    rows, cap, held = row["rows"], row["cap"], row["end"] - row["origin"]
    x = np.full((rows, cap), np.nan, dtype=F32)
    x[:, :min(cap, held)] = g.standard_normal((rows, min(cap, held))).astype(F32)
    if row["nan_rows"]:
        x[0::2] = np.nan
    alloc = np.full(row["xoff"] + rows * cap + RS_PAD, np.nan, dtype=F32)
    alloc[row["xoff"]:row["xoff"] + rows * cap] = x.reshape(-1)
    return dict(x_alloc=alloc, G=G, up=up, down=down, half=half, T=T)


def _rs_sum(row, inp, dtype, mutant=None):
    """y [rows, count] and sum (g x)^2: the k = 0 .. T-1 chain (fmaf: the product is exact in float64, one rounding of the sum)."""
    up, down, half, T, G = inp["up"], inp["down"], inp["half"], inp["T"], inp["G"]
    rows, cap, origin, end = row["rows"], row["cap"], row["origin"], row["end"]
    x = inp["x_alloc"][row["xoff"]:row["xoff"] + rows * cap].astype(np.float64)
    n = row["n_first"] + np.arange(row["count"])
    t = n * down + (0 if mutant == RS_MUTANTS[2] else half)
    p, j0 = t % up, t // up
    G64 = np.concatenate((G.astype(np.float64), np.zeros((up, 1))), 1)
    acc = np.zeros((rows, n.size), dtype=dtype)
    q = np.zeros((rows, n.size))
    rbase = (np.arange(rows) * cap)[:, None]
    for k in range(T):
        if mutant == RS_MUTANTS[0] and k == half // up:      # (the centre tap h[half] and its neighbours)
            continue
        j = j0 - k
        jr = j - (0 if mutant == RS_MUTANTS[7] else origin)
        if mutant == RS_MUTANTS[4]:
            valid = np.ones(n.size, bool)
            at = np.clip(rbase + jr[None], 0, x.size - 1)
        else:
            valid = (j >= 0) & (jr >= 0) & (jr < cap)
            if mutant != RS_MUTANTS[3]:
                valid = valid & (j < end)
            at = rbase + np.clip(jr, 0, cap - 1)[None]
        gk = G64[p, k + 1 if mutant == RS_MUTANTS[1] else k]
        with np.errstate(invalid="ignore"):
            term = np.where(valid[None], gk[None] * x[at], 0.0)
            acc = (acc.astype(np.float64) + term).astype(dtype)
            q += term * term
    return acc, q


def rs_place(row, inp, y, mutant=None):
    """y [rows, count] -> the output allocation [yoff + rows count + RS_PAD], NaN around the view, by the kernels' stores."""
    rows, count, yoff = row["rows"], row["count"], row["yoff"]
    out = np.full(yoff + rows * count + RS_PAD, np.nan, dtype=y.dtype)
    tile = rs_choice(inp["up"], inp["down"], inp["T"])[0]
    for r in range(rows):
        base = yoff + r * count
        out[base:base + count] = y[r]
        if not tile:
            continue
        tiles = cdiv(count, tile)
        last0 = (tiles - 1) * tile
        cnt = count - last0
        if mutant == RS_MUTANTS[5]:                       # the last tile stores cnt - 1 outputs
            out[base + count - 1] = np.nan
        if mutant == RS_MUTANTS[6]:                       # the lead not cut at cnt: the scalar head runs on with the clamped output's value
            lead = (4 - (base + last0) % 4) % 4           # (the allocation itself starts on the 16-byte grid)
            if lead > cnt:
                out[base + count:base + last0 + lead] = y[r, -1]
    return out


def rs_lead_exceeds_cnt(row):
    up, down, half, T, _ = rs_design(row["f_in"], row["f_out"])
    tile = rs_choice(up, down, T)[0]
    if not tile:
        return False
    r = row["rows"] - 1                                   # the last row: what the head writes past it lands in the allocation's NaN
    return rs_lead(row, r, tile) > row["count"] - (cdiv(row["count"], tile) - 1) * tile


def rs_reference(row, inp):
    acc, q = _rs_sum(row, inp, np.float64)
    y = rs_place(row, inp, acc)
    return {"y": (y, np.where(np.isnan(y), 0.0, rs_place(row, inp, np.sqrt(q))))}


def rs_fp32(row, inp, mutant=None):
    return {"y": rs_place(row, inp, _rs_sum(row, inp, F32, mutant)[0], mutant)}


RS_ROWS = _rs_rows()

# ----------------------------------------------------------------------------------------------------------------------------------
# slice (layout.hip: sep_slice_input_c2_kernel, sep_slice_input_kernel, sep_slice_input_plane_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
SL_MUTANTS = ("s * Hs + h as h * 16 + s", "c / s order swapped", "clamp missing", "mask applied to the log value", "plane at channel 16 C - 1",
              "tail frames of a 64-tile dropped")
SL_GRID_CAP, SL_BLOCK, SL_TT = 256 * 16, 256, 64       # grid_for(total, 256, 4096); the tiled kernel's 64 frames per block


def sl_kernel(row):
    """m2h_sep_slice_input_fmt's rule: the tiled kernel for C == 2 and an even T, the generic one otherwise; the plane kernel is its own entry."""
    return "plane" if row["form"] == "plane" else "tiled" if row["C"] == 2 and row["T"] % 2 == 0 else "generic"


def sl_total(row):
    """Work items of the generic and plane kernels' grid-stride launch (None: the tiled kernel has one block per (b, h, 64 frames))."""
    k = sl_kernel(row)
    if k == "tiled":
        return None
    return row["B"] * (row["F"] // 16) * row["T"] * ((row["ldo"] if k == "plane" else 16 * row["C"]) // 4)


def sl_second_pass(row):
    t = sl_total(row)
    return t is not None and t > max(1, min(cdiv(t, SL_BLOCK), SL_GRID_CAP)) * SL_BLOCK


def _sl_row(B, F, T, C, masks="none", split=False, form="fmt", ldo=0, big=False):
    name = "B%d.F%d.T%d.C%d.%s%s%s%s" % (B, F, T, C, masks, ".split32" if split else "", ".plane%d" % ldo if form == "plane" else "", ".big" if big else "")
    return dict(id="slice." + name, family="slice", B=B, F=F, T=T, C=C, masks=masks, split=split, form=form, ldo=ldo)


SL_ROWS = [
    _sl_row(2, 512, 32, 2, "mixed"), _sl_row(2, 512, 32, 2, "mixed", split=True), _sl_row(1, 16, 64, 2), _sl_row(2, 32, 66, 2, "mixed", split=True),
    _sl_row(3, 16, 2, 2, "mixed"), _sl_row(1, 32, 66, 2, split=True), _sl_row(2, 32, 5, 1, "mixed"), _sl_row(2, 16, 7, 3, "mixed"), _sl_row(2, 32, 33, 2, "mixed"),
    _sl_row(1, 512, 3, 1), _sl_row(2, 512, 4, 2, form="plane", ldo=36), _sl_row(3, 16, 5, 1, form="plane", ldo=20),
    _sl_row(52429, 16, 5, 1, big=True), _sl_row(52429, 16, 4, 1, form="plane", ldo=20, big=True),
]


def sl_cells(row):
    k = sl_kernel(row)
    out = {k, "F = 16 (Hs = 1)" if row["F"] == 16 else "F = %d" % row["F"], "split32 output" if row["split"] else "float32 output",
           "masks " + row["masks"]}
    if k == "tiled":
        out.add("tiled T = %d" % row["T"])
    if k == "generic":
        out.add("generic C = %d%s" % (row["C"], " odd T" if row["C"] == 2 else ""))
    if k == "plane":
        out.add("plane ldo = %d C = %d" % (row["ldo"], row["C"]))
        out.add("the class value in channel 16 C and zeros after it")
    if sl_second_pass(row):
        out.add(k + " second pass of the grid-stride loop")
    if row["masks"] == "mixed" and not is_big(row):
        inp = sl_inputs(row)
        if (inp["masks"] < 0).any() and (inp["masks"] == 0).any():
            out.add("negative and zero masks")
        if float(inp["mix"][inp["mix"] > 0].min()) <= 1e-6 and float(inp["mix"].max()) == 12.0:
            out.add("x from 1e-6 to 12")
    return out


def sl_all_cells():
    return {"tiled", "generic", "plane", "F = 16 (Hs = 1)", "F = 32", "F = 512", "split32 output", "float32 output", "masks none", "masks mixed", "tiled T = 32",
            "tiled T = 64", "tiled T = 66", "tiled T = 2", "generic C = 1", "generic C = 3", "generic C = 2 odd T", "plane ldo = 36 C = 2", "plane ldo = 20 C = 1",
            "the class value in channel 16 C and zeros after it", "generic second pass of the grid-stride loop", "plane second pass of the grid-stride loop",
            "negative and zero masks", "x from 1e-6 to 12"}


def sl_inputs(row):
    g = _rng(row)
    shape = (row["B"], row["F"], row["T"], row["C"])
    n = int(np.prod(shape))
    mix = np.exp(g.uniform(np.log(1e-6), np.log(12.0), n)).astype(F32)
    mix[:3] = (0.0, 1e-6, 12.0)
    mix[-3:] = (12.0, 0.0, 1e-6)
    out = dict(mix=mix.reshape(shape), masks=None, cls=None)
    if row["masks"] == "mixed":
        m = g.standard_normal(n).astype(F32)
        m[:6] = (1.5, 0.0, -0.0, 2.0, -1.0, 3.0)
        out["masks"] = m.reshape(shape)
    if row["form"] == "plane":
        out["cls"] = (1.0 + g.integers(0, 102, row["B"])).astype(F32)
    return out


def _sl_layout(a, mutant=None):
    """[B, F, T, C] -> [B, Hs, T, 16 C]: out[b][h][t][c 16 + s] = a[b][s Hs + h][t][c]"""
    B, F, T, C = a.shape
    Hs = F // 16
    if mutant == SL_MUTANTS[0]:
        v = a.reshape(B, Hs, 16, T, C).transpose(0, 1, 3, 4, 2)
    else:
        v = a.reshape(B, 16, Hs, T, C).transpose(0, 2, 3, 4, 1)          # [B, Hs, T, C, 16]
    if mutant == SL_MUTANTS[1]:
        v = v.transpose(0, 1, 2, 4, 3)
    return np.ascontiguousarray(v).reshape(B, Hs, T, 16 * C)


def _sl_plane(row, v, cls, mutant=None):
    """[B, Hs, T, 16 C] -> [B, Hs, T, ldo]: the class value in channel 16 C, zeros after it"""
    nc = 16 * row["C"]
    out = np.zeros(v.shape[:3] + (row["ldo"],), dtype=v.dtype)
    out[..., :nc] = v
    out[..., nc - 1 if mutant == SL_MUTANTS[4] else nc] = cls.astype(v.dtype)[:, None, None]
    return out


def sl_reference(row, inp):
    """(r, s) of the float32 values [B, Hs, T, 16 C or ldo]; a split32 row: of hi + lo."""
    x = inp["mix"].astype(np.float64)
    if inp["masks"] is None:
        r, s = x, np.zeros(x.shape)
    else:
        m = inp["masks"].astype(np.float64)
        e = np.exp(x)
        arg = m * (e - 1.0)
        z = np.maximum(arg, 0.0)
        r = np.log1p(z)
        s = np.where(arg <= 0, 0.0, np.abs(m) * e * (1 + np.abs(x)) / (1 + z) + r)
    r, s = _sl_layout(r), _sl_layout(s)
    if row["form"] == "plane":
        r, s = _sl_plane(row, r, inp["cls"]), _sl_plane(row, s, np.zeros(row["B"]))
    if row["split"] and inp["masks"] is None:      # an exact value has an exact split: hi + lo of it, s = 0
        hi = bf16_round(r.astype(F32))
        r = hi.astype(np.float64) + bf16_round(r.astype(F32) - hi).astype(np.float64)
    elif row["split"]:                             # hi + lo keeps 16 to 17 bits: the output's own rounding, 2^-17 |r|, joins s
        s = s + 2.0 ** -17 * np.abs(r)
    return {"out": (r, s)}


def bf16_round(v):
    """float32 -> the nearest bfloat16 (ties to even), as a float32"""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(F32)


def unsplit32(buf):
    """A split32 buffer (float32 storage, groups of 32 values: 32 bfloat16 hi, then 32 bfloat16 lo) -> hi + lo in float64, the shape of buf."""
    h = np.ascontiguousarray(buf).view(np.uint16).reshape(-1, 64).astype(np.uint32) << np.uint32(16)
    f = h.view(F32).astype(np.float64)
    return (f[:, :32] + f[:, 32:]).reshape(buf.shape)


def sl_fp32(row, inp, mutant=None):
    x, m = inp["mix"], inp["masks"]
    k = sl_kernel(row)
    with np.errstate(all="ignore"):
        if m is None:
            v = x
        elif mutant == SL_MUTANTS[3]:
            v = np.maximum(m * x, F32(0))
        elif k == "tiled":      # masked_log_mag: exp2 / log2 / rcp, log1p by the (log u) z / (u - 1) form
            e = np.exp2((x * F32(1.44269504088896341)).astype(F32)).astype(F32)
            z = m * (e - F32(1))
            if mutant != SL_MUTANTS[2]:
                z = np.maximum(z, F32(0))
            u = F32(1) + z
            d = u - F32(1)
            v = np.where(d == 0, z, (np.log2(u).astype(F32) * F32(0.693147180559945309)) * (z * (F32(1) / d)))
        else:
            z = m * (np.exp(x).astype(F32) - F32(1))
            if mutant != SL_MUTANTS[2]:
                z = np.maximum(z, F32(0))
            v = np.log1p(z).astype(F32)
    v = _sl_layout(v.astype(F32), mutant)
    if mutant == SL_MUTANTS[5]:
        v[:, :, (row["T"] // SL_TT) * SL_TT:] = np.nan
    if row["form"] == "plane":
        v = _sl_plane(row, v, inp["cls"], mutant)
    if row["split"]:
        hi = bf16_round(v)
        v = hi.astype(np.float64) + bf16_round(v - hi).astype(np.float64)
    return {"out": v}



# ----------------------------------------------------------------------------------------------------------------------------------
ROWS = {"frames": FRAMES_ROWS, "post": POST_ROWS, "pre": PRE_ROWS, "bin_rows": BIN_ROWS, "ola": OLA_ROWS, "xfade": XF_ROWS, "resample": RS_ROWS, "slice": SL_ROWS}
ROWS_BY_ID = {r["id"]: r for rows in ROWS.values() for r in rows}
CELLS = {"frames": frames_cells, "post": post_cells, "pre": pre_cells, "bin_rows": bin_cells, "ola": ola_cells, "xfade": xf_cells, "resample": rs_cells,
         "slice": sl_cells}
_ALL = {"frames": frames_all_cells, "post": post_all_cells, "pre": pre_all_cells, "bin_rows": bin_all_cells, "ola": ola_all_cells, "xfade": xf_all_cells,
        "resample": rs_all_cells, "slice": sl_all_cells}
INPUTS = {"frames": frames_inputs, "post": post_inputs, "pre": pre_inputs, "bin_rows": bin_inputs, "ola": ola_inputs, "xfade": xf_inputs, "resample": rs_inputs,
          "slice": sl_inputs}
# (xfade goes call by call: xf_reference_call / xf_fp32_call)
REFERENCE = {"frames": frames_reference, "post": post_reference, "pre": pre_reference, "bin_rows": bin_reference, "ola": ola_reference, "resample": rs_reference,
             "slice": sl_reference}
FP32 = {"frames": frames_fp32, "post": post_fp32, "pre": pre_fp32, "bin_rows": bin_fp32, "ola": ola_fp32, "resample": rs_fp32, "slice": sl_fp32}


def is_big(row):
    return row["id"].endswith(".big")


def cells(row):
    return CELLS[row["family"]](row)


def all_cells(family):
    return _ALL[family]()


def inputs(row):
    return INPUTS[row["family"]](row)


def reference(row, inp):
    return REFERENCE[row["family"]](row, inp)


def _ola_past_quad(r):
    return r["win"] and r["cap"] > r["end"] - r["origin"] and r["end"] % 4 != 0


# (family, mutant) -> predicate on the row: the rows the bound must reject the mutant on; the .big rows carry no mutants (they are there for the
# second pass of the grid-stride loop alone)
MUTANT_ROWS = {
    ("frames", FRAMES_MUTANTS[0]): lambda r: True,
    ("frames", FRAMES_MUTANTS[1]): lambda r: True,
    ("frames", FRAMES_MUTANTS[2]): lambda r: any(0 <= r["end"] - s * r["hop"] < SEP_SEG for s in range(r["s0"], r["s0"] + r["nseg"])),
    ("frames", FRAMES_MUTANTS[3]): lambda r: r["hop"] != SEP_SEG and r["s0"] + r["nseg"] > 1,
    ("frames", FRAMES_MUTANTS[4]): lambda r: r["origin"] > 0,
    ("frames", FRAMES_MUTANTS[5]): lambda r: r["win"] and r["cap"] != r["end"],
    ("post", POST_MUTANTS[0]): lambda r: True,
    ("post", POST_MUTANTS[1]): lambda r: True,
    ("post", POST_MUTANTS[2]): lambda r: True,
    ("post", POST_MUTANTS[3]): lambda r: True,
    ("post", POST_MUTANTS[4]): lambda r: True,
    ("pre", PRE_MUTANTS[0]): lambda r: True,
    ("pre", PRE_MUTANTS[1]): lambda r: True,
    ("pre", PRE_MUTANTS[2]): lambda r: True,
    ("bin_rows", BIN_MUTANTS[0]): lambda r: True,
    ("bin_rows", BIN_MUTANTS[1]): lambda r: True,
    ("bin_rows", BIN_MUTANTS[2]): lambda r: True,
    ("ola", OLA_MUTANTS[0]): _ola_reaches_t1_clamp,
    ("ola", OLA_MUTANTS[1]): lambda r: r["end"] - r["calls"][-1][0] * SEP_SEG > 512,
    ("ola", OLA_MUTANTS[2]): lambda r: any(s0 > 0 for s0, _ in r["calls"]) and not r["win"],
    ("ola", OLA_MUTANTS[3]): _ola_past_quad,
    ("ola", OLA_MUTANTS[4]): lambda r: r["origin"] > 0,
    ("xfade", XF_MUTANTS[0]): lambda r: len(r["calls"]) > 1,
    ("xfade", XF_MUTANTS[2]): lambda r: len(r["calls"]) > 1,
    ("xfade", XF_MUTANTS[3]): lambda r: True,
    ("xfade", XF_MUTANTS[4]): lambda r: True,
    ("resample", RS_MUTANTS[0]): lambda r: r["end"] > 8,
    ("resample", RS_MUTANTS[1]): lambda r: r["end"] > 8,
    ("resample", RS_MUTANTS[2]): lambda r: r["end"] > 8,
    ("resample", RS_MUTANTS[3]): lambda r: r["win"],
    ("resample", RS_MUTANTS[4]): lambda r: r["nan_rows"],
    ("resample", RS_MUTANTS[5]): lambda r: rs_kernel(r)[0] != "direct",
    ("resample", RS_MUTANTS[6]): rs_lead_exceeds_cnt,
    ("resample", RS_MUTANTS[7]): lambda r: r["origin"] > 0,
    ("slice", SL_MUTANTS[0]): lambda r: r["F"] > 16,
    ("slice", SL_MUTANTS[1]): lambda r: r["C"] > 1,
    ("slice", SL_MUTANTS[2]): lambda r: r["masks"] == "mixed",
    ("slice", SL_MUTANTS[3]): lambda r: r["masks"] == "mixed",
    ("slice", SL_MUTANTS[4]): lambda r: r["form"] == "plane",
    ("slice", SL_MUTANTS[5]): lambda r: sl_kernel(r) == "tiled" and r["T"] % SL_TT != 0,
}
