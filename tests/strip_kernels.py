"""The strip-walker kernels (csrc/conv_strip.hip: conv1_strip_kernel<MASKED, HI>, convT_last_strip_kernel<N, HI>) held to float64 element by
element, on every path and job round: the table of rows, the float64 references with the bound's scale beside them, restatements of the
host's launch arithmetic and of the bin2mono pre-op, and the named mutants -- shared by tests/test_gpu_strip_kernels.py (every row on the GPU)
and tests/test_strip_kernels_cpu.py (the rows reach every cell, the bound discriminates; no GPU).

References (float64, from the values the kernel reads)
  first stage   x[b, c*16+s, h, w] = mix[b, s*32+h, w, c] (restated here), z = conv2d(x, w, 2, 1) from the fp32 x and w (the kernel splits
                both itself); the class plane cls_val[b] is a real 33rd channel; r = leaky(z scale + shift, 0.2),
                s = sqrt(conv(x^2, w^2)) |scale| + |shift| + 2^-17 |r| (the output is a split32 tensor: its own rounding joins the scale).
  masked        p = log1p(max(m expm1(x), 0)) replaces x.  The pre-op's fp32 error is not relative to p (a correct fp32 evaluation of a
                quiet input is off by 100 % of p) but to u = |m| exp(x) + p; the bound becomes tau s + TAU_PRE s_pre with
                s_pre = sqrt(conv(u^2, w^2)) |scale|.  TAU_PRE = 8 x PRE_RESTATEMENT_WORST, the ceiling over the table's own masked rows of
                |p32 - p64| / u for preop32, a numpy float32 restatement of masked_log_mag's own steps (csrc/m2h_internal.h).
  last stage    x, skip and the weight as hi + lo of split32; z = conv_transpose2d(cat(x, skip), w, 2, 1), y = relu(z scale + shift) with
                s_y = sqrt(convT(x^2, w^2)) |scale| + |shift|; r_j = sum_n hw[j][n] y_n + hb[j], de-sliced.  The strip kernel runs the head
                in bf16x3 on Y's hi / lo records, so the head's own products join: s_j = sqrt(sum_n hw[j][n]^2 (s_y,n^2 + y_n^2)) + |hb[j]|.
  HI (M2H_MATH_BF16)  the reference starts from the operands rounded to bf16: the kernel's products are then exact and only the fp32
                accumulation is left (TAU_FP32).  An intermediate rounded to bf16 inside the kernel (Y; the pre-op's result) comes from an
                fp32 value that differs from the reference's: an element within its own bound delta (TAU_FP32 s_y; TAU_PRE u) of a
                rounding boundary is FLAGGED and may land on the other neighbour; f = sum |coefficient| ulp_bf16 over the flagged terms
                of an output is allowed beside the bound.  FLAG_SHARE_MAX and CLEAN_SHARE_MIN keep the allowance from hiding a failure.
Every bound |g - r| <= tau s + extra goes through elem_bound.bound(g, r, s + extra / tau, tau): check() below.

Rows are the smallest shapes that reach each cell of the restated launch arithmetic (cells()).  A multi-round row has more job slots than
the grid cap (512 workgroups; 256 for N = 32), reached with a real batch: its images whose job runs in a second round, the images that
share a workgroup with one and a seeded sample (COMPARED_CAP in all) are compared with float64, and EVERY image must be bit-identical to
the same image run in a batch of at most 8 (its job then runs in the first round: a job's arithmetic depends on its own image alone).

Mutants are applied to the float64 reference (M_D0 to the float32 pre-op restatement inside the CPU stand-in) and named only for rows on
which they can show:
  * the seam mutants (halo column as zeros, halo records without lo, seam given the border's class) need two strips: T >= 128;
  * "the d == 0 branch returning 0" differs from the kernel only where 0 < z < 2^-24.  The `quiet` row (mix * 1e-5) does NOT get there:
    z = m (e - 1) ~ 1e-5 is far above 2^-24, and its d == 0 elements are the clamped ones, where z = 0 is what both return.  The
    `tiny_mask` row (masks * 1e-8, shift 0 so that the output keeps the pre-op's scale) takes that branch with z > 0 on every element
    that is not clamped, and the mutant is named for it alone;
  * "the clamp dropped" leaves NaN wherever m expm1(x) <= -1 (counted as an infinite margin, as tests/acoustics_kernels.py does);
  * "row q - 1 read where q + 1 is due" needs H >= 2 (at H = 1 both are padding), "the row past the image replicated" shows at any H;
  * the job-map mutants are asserted on the restated map (map_faults), not numerically.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import forward_ref as FR
from elem_bound import TAU_BF16X3, TAU_FP32

# ---- the source's constants (tests/test_strip_kernels_cpu.py reads them from csrc/conv_strip.hip) ----
SW, PX = 32, 34
GRID_CAP = {"conv1": 512, "conv1m": 512, "last32": 256, "last16": 512}
RING = {"conv1": 4, "last": 3}
LABEL = {"conv1": "strip_conv1", "conv1m": "strip_conv1<masked>", "last32": "strip_convT_last<32>", "last16": "strip_convT_last<16>"}
REV_KNOB = 39

MIN_MARGIN = 4.0
PRE_RESTATEMENT_WORST = 2.8e-7       # ceiling of |preop32 - p64| / u over the masked rows (measured: 2.59e-7, tiny_mask; tests/test_strip_kernels_cpu.py pins it)
TAU_PRE = 8 * PRE_RESTATEMENT_WORST
FLAG_SHARE_MAX, CLEAN_SHARE_MIN = 0.05, 0.25
COMPARED_CAP = 48
OUT_ROUNDING = 2.0 ** -17


# ---------------------------------------------------------------------------------------------------------------------------------
# The launch arithmetic restated: jobs_padded, grid, the slot a workgroup's iteration takes, strip_job
# ---------------------------------------------------------------------------------------------------------------------------------
M_ROUND = "the second round's image index taken from the first round"
M_REV_OFF = "the reversed order off by one group of 8"
MAP_MUTANTS = (M_ROUND, M_REV_OFF)


def jobs_padded(B, strips):
    return (B + 7) // 8 * 8 * strips


def strip_job(linear, strips, jobs):
    xcd, y = linear & 7, linear >> 3
    job = ((y // strips) * 8 + xcd) * strips + y % strips
    return job if job < jobs else -1


def job_map(B, strips, cap, rev, mutant=None):
    """(jobs_padded, grid, per workgroup the list of (slot, job) of its iterations in order; job -1 = an empty slot, skipped)."""
    jp = jobs_padded(B, strips)
    grid = min(jp, cap)
    wgs = []
    for wg in range(grid):
        seq = []
        for rnd, lin in enumerate(range(wg, jp, grid)):
            src = wg if (mutant == M_ROUND and rnd) else lin
            slot = jp - (16 if mutant == M_REV_OFF else 8) - (src & ~7) + (src & 7) if rev else src
            seq.append((slot, strip_job(slot, strips, B * strips) if 0 <= slot < jp else -1))
        wgs.append(seq)
    return jp, grid, wgs


def map_faults(B, strips, cap, rev, mutant=None):
    """What is wrong with the map: a slot outside [0, jobs_padded), a job taken twice or never.  Empty for a sound map."""
    jp, grid, wgs = job_map(B, strips, cap, rev, mutant)
    faults, taken = [], {}
    if grid % 8:
        faults.append("grid %d is no multiple of 8" % grid)
    for seq in wgs:
        for slot, job in seq:
            if not 0 <= slot < jp:
                faults.append("slot %d outside [0, %d)" % (slot, jp))
            elif job >= 0:
                taken[job] = taken.get(job, 0) + 1
    faults += ["job %d taken %d times" % (j, n) for j, n in taken.items() if n != 1]
    faults += ["job %d never taken" % j for j in range(B * strips) if j not in taken]
    return faults


def strips_of(row):
    return (row["T"] // 2 if row["kernel"].startswith("conv1") else row["W"]) // SW


def knob(row, rev):
    """The value of knob 39 that makes the row's kernel walk in direction rev (bit 0 masked first stage, bit 2 unmasked: 1 = reversed;
    bit 1 last stage: 1 = forward, the default is reversed)."""
    k = row["kernel"]
    return (1 if rev else 0) if k == "conv1m" else (4 if rev else 0) if k == "conv1" else (0 if rev else 2)


def default_rev(row):
    return 1 if row["kernel"].startswith("last") else 0


def directions(row):
    return (0, 1) if row["multi"] else (default_rev(row),)


def compared_images(row):
    """Images of a multi-round row compared with float64: those with a second-round job, those that share a workgroup with one (either
    direction), then a seeded sample up to COMPARED_CAP."""
    strips, B = strips_of(row), row["B"]
    pick = set()
    for rev in directions(row):
        for seq in job_map(B, strips, GRID_CAP[row["kernel"]], rev)[2]:
            if any(job >= 0 for _, job in seq[1:]):
                pick |= {job // strips for _, job in seq if job >= 0}
    assert len(pick) <= COMPARED_CAP, (row["id"], len(pick))
    rest = [b for b in np.random.RandomState(zlib.crc32(row["id"].encode()) & 0x7FFFFFFF).permutation(B) if b not in pick]
    return sorted(pick | set(int(b) for b in rest[:COMPARED_CAP - len(pick)]))


ALL_CELLS = {
    "conv1": {"strips 1", "strips 2", "strips >= 3", "halo none", "halo right only", "halo left only", "halo both", "empty slot skipped",
              "second-round job", "empty then live", "live then empty", "forward", "reversed", "class plane on", "class plane off"}
             | {"class border %d" % i for i in range(9)},
    "conv1m": {"strips 1", "strips 2", "strips >= 3", "halo none", "halo right only", "halo left only", "halo both", "empty slot skipped",
               "second-round job", "empty then live", "live then empty", "forward", "reversed", "class plane off",
               "pre-op clamped", "pre-op d == 0 with z > 0", "pre-op quotient"},
}
for _k in ("last32", "last16"):
    ALL_CELLS[_k] = {"strips 1", "strips 2", "strips >= 3", "empty slot skipped", "second-round job", "empty then live", "live then empty",
                     "forward", "reversed", "H 1", "H 2", "H 3", "H >= 4", "N %s" % _k[4:]}
PRE_SHARE_MIN = 0.05    # a pre-op branch counts as reached by a row that sends at least this share of its elements there


def cells(row, pre_shares=None):
    """The cells the row reaches, from the restated launch arithmetic (and, for a masked row, pre_shares = preop32's branch shares)."""
    k, strips, B = row["kernel"], strips_of(row), row["B"]
    out = {"strips %s" % (strips if strips < 3 else ">= 3")}
    for rev in directions(row):
        out.add("reversed" if rev else "forward")
        for seq in job_map(B, strips, GRID_CAP[k], rev)[2]:
            live = [job >= 0 for _, job in seq]
            if not all(live):
                out.add("empty slot skipped")
            if any(live[1:]):
                out.add("second-round job")
            for a, b in zip(live, live[1:]):
                out.add("live then empty" if a and not b else "empty then live" if b and not a else "live then live")
            for _, job in seq:
                if job >= 0 and k.startswith("conv1"):
                    r0 = (job % strips) * SW
                    has_l, has_r = r0 > 0, r0 + SW < strips * SW
                    out.add("halo " + ("both" if has_l and has_r else "left only" if has_l else "right only" if has_r else "none"))
                    if row["cls"]:
                        for q in range(16):
                            ch = 0 if q == 0 else 2 if q == 15 else 1
                            for m in range(16):
                                out.add("class border %d" % (ch * 3 + (0 if m == 0 and not has_l else 1)))
                                out.add("class border %d" % (ch * 3 + (2 if m == 15 and not has_r else 1)))
    out.discard("live then live")
    if k.startswith("conv1"):
        out.add("class plane on" if row["cls"] else "class plane off")
        if row["masked"] and pre_shares is not None:
            out |= {"pre-op " + name for name, share in pre_shares.items() if share >= PRE_SHARE_MIN}
    else:
        H = row["H"]
        out |= {"H %s" % (H if H < 4 else ">= 4"), "N %d" % row["N"]}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _c1(tag, B, T, masked, cls=None, multi=False, **kw):
    fam = "msk" if masked else "cls" if cls in (None, True) else "plain"
    row = dict(id="c1.%s%s.b%d.t%d" % (fam, "." + tag if tag else "", B, T), kernel="conv1m" if masked else "conv1", B=B, T=T, masked=masked,
               cls=(not masked) if cls is None else cls, multi=multi, hi=False, bn="unit", mix="normal", mask="normal", family=tag or "shape")
    row.update(kw)
    return row


def _last(tag, N, B, H, W, multi=False, **kw):
    row = dict(id="last%d%s.b%d.h%d.w%d" % (N, "." + tag if tag else "", B, H, W), kernel="last%d" % N, N=N, B=B, H=H, W=W, multi=multi, hi=False,
               bn="unit", head="random", family=tag or "shape")
    row.update(kw)
    return row


CONV1_ROWS = [_c1("", B, T, masked) for B, T in ((3, 64), (2, 128), (1, 192), (9, 256)) for masked in (False, True)]
CONV1_ROWS += [_c1("", 2, 128, False, cls=False), _c1("wide", 2, 128, False, bn="wide"), _c1("wide", 2, 128, True, bn="wide")]
CONV1_ROWS += [_c1("quiet", 2, 128, True, mix="quiet"), _c1("loud", 2, 128, True, mix="loud"), _c1("zero_mix", 2, 128, True, mix="zero"),
               _c1("zero_mask", 2, 128, True, mask="zero"), _c1("neg_mix", 2, 128, True, mix="neg"), _c1("one_mask", 2, 128, True, mask="one"),
               _c1("tiny_mask", 2, 128, True, mask="tiny", bn="noshift")]
CONV1_ROWS += [_c1("", 513, 64, False, multi=True, family="multi"), _c1("", 513, 64, True, multi=True, family="multi"),
               _c1("", 129, 256, False, multi=True, family="multi"), _c1("", 129, 256, True, multi=True, family="multi")]

LAST_ROWS = []
for _N in (32, 16):
    LAST_ROWS += [_last("", _N, 3, H, 64) for H in (1, 2, 3, 4, 16)] + [_last("", _N, 2, 2, W) for W in (32, 96, 128)] + [_last("", _N, 9, 2, 64)]
    LAST_ROWS += [_last("wide", _N, 3, 3, 64, bn="wide")]
LAST_ROWS += [_last("identity", 32, 2, 3, 64, head="identity")]
LAST_ROWS += [_last("", 32, 257, 2, 32, multi=True, family="multi"), _last("", 32, 65, 2, 128, multi=True, family="multi"),
              _last("", 16, 513, 2, 32, multi=True, family="multi"), _last("", 16, 260, 2, 64, multi=True, family="multi")]


def _hi(row):
    """(a masked HI row's mix is uniform in 0.5 to 2: with |randn| * 1.5 the many inputs near 0, where u / p grows like 1 / x, are flagged
    almost surely, 0.33 % of the 512 terms of an output are, and only 20 % of the outputs carry no allowance -- CLEAN_SHARE_MIN could not
    hold; at 0.5 to 2, u / p stays near its minimum of 3.7 and 0.18 % are flagged)"""
    return dict(row, id="hi." + row["id"], hi=True, family="hi", **({"mix": "mid"} if row.get("masked") else {}))


_BY_ID = {r["id"]: r for r in CONV1_ROWS + LAST_ROWS}
HI_ROWS = [_hi(_BY_ID[i]) for i in ("c1.cls.b3.t64", "c1.cls.b513.t64", "c1.msk.b3.t64", "c1.msk.b513.t64",
                                    "last32.b3.h3.w64", "last32.b257.h2.w32", "last16.b3.h3.w64", "last16.b513.h2.w32")]
ROWS = {r["id"]: r for r in CONV1_ROWS + LAST_ROWS + HI_ROWS}
assert len(ROWS) == len(CONV1_ROWS) + len(LAST_ROWS) + len(HI_ROWS)
SMALL_ROWS = [i for i, r in ROWS.items() if not r["multi"]]


# ---------------------------------------------------------------------------------------------------------------------------------
# Data: torch.randn from a generator seeded with crc32 of the row's id
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(row):
    return torch.Generator().manual_seed(zlib.crc32(row["id"].encode()))


def _bn(row, n, g):
    """Folded BatchNorm: scale = rand + 0.5 (`wide`: 0.05 .. 2 spread over the channels, shuffled), shift = randn * 0.1 (`noshift`: 0)."""
    scale = torch.rand(n, generator=g) + 0.5
    shift = torch.randn(n, generator=g) * 0.1
    if row["bn"] == "wide":
        scale = torch.linspace(0.05, 2.0, n)[torch.randperm(n, generator=g)].contiguous()
    if row["bn"] == "noshift":
        shift = torch.zeros(n)
    return scale, shift


def conv1_data(row):
    """dict(mix, masks | None, w [64, 32 | 33, 4, 4], scale, shift, cls_val | None) of a first-stage row, fp32, in the layouts the caller holds."""
    g, B, T = _gen(row), row["B"], row["T"]
    mix = torch.randn(B, 512, T, 2, generator=g).abs_().mul_(1.5)
    if row["mix"] == "quiet":
        mix.mul_(1e-5)
    elif row["mix"] == "loud":
        mix = torch.rand(B, 512, T, 2, generator=g) * 6.0 + 5.0
    elif row["mix"] == "mid":
        mix = torch.rand(B, 512, T, 2, generator=g) * 1.5 + 0.5
    elif row["mix"] == "zero":
        mix.zero_()
    elif row["mix"] == "neg":
        mix.neg_()
    masks = None
    if row["masked"]:
        masks = torch.randn(B, 512, T, 2, generator=g).mul_(0.7).add_(0.3)
        if row["mask"] == "zero":
            masks.zero_()
        elif row["mask"] == "one":
            masks.fill_(1.0)
        elif row["mask"] == "tiny":
            masks.mul_(1e-8)
    w = torch.randn(64, 33 if row["cls"] else 32, 4, 4, generator=g) * (2.0 / 512) ** 0.5
    scale, shift = _bn(row, 64, g)
    cls_val = torch.randint(1, 4, (B,), generator=g).float() if row["cls"] else None
    return dict(mix=mix, masks=masks, w=w, scale=scale, shift=shift, cls_val=cls_val)


def last_data(row):
    """dict(x, skip [B, 64, H, W] NCHW, w [128, N, 4, 4] (torch ConvTranspose2d layout), scale, shift, hw [N, N], hb [N]) of a last-stage row."""
    g, B, H, W, N = _gen(row), row["B"], row["H"], row["W"], row["N"]
    x = torch.randn(B, 64, H, W, generator=g)
    skip = torch.randn(B, 64, H, W, generator=g)
    w = torch.randn(128, N, 4, 4, generator=g) * (2.0 / 512) ** 0.5
    scale, shift = _bn(row, N, g)
    hw, hb = torch.randn(N, N, generator=g) * (2.0 / N) ** 0.5, torch.randn(N, generator=g) * 0.1
    if row["head"] == "identity":
        hw, hb = torch.eye(N), torch.zeros(N)
    return dict(x=x, skip=skip, w=w, scale=scale, shift=shift, hw=hw, hb=hb)


def take(d, idx):
    """The data of images idx alone (a job's values depend on its own image alone)."""
    idx = torch.as_tensor(idx, dtype=torch.long)
    return {k: (v[idx].contiguous() if k in ("mix", "masks", "cls_val", "x", "skip") and v is not None else v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# Number formats
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16(t):
    """Round to bf16 (nearest even), as float64."""
    return t.float().to(torch.bfloat16).double()


def seen32(t):
    """hi + lo of the split32 layout, as float64."""
    hi, lo = FR.hi_lo(t.float())
    return hi.double() + lo.double()


def unsplit32(t):
    """split32 tensor (fp32-typed storage; every 32 values = 32 bf16 hi + 32 bf16 lo) -> the fp32 values hi + lo."""
    b = t.contiguous().view(torch.bfloat16).reshape(-1, 64)
    return (b[:, :32].float() + b[:, 32:].float()).reshape(t.shape)


def bf16_flags(v, delta):
    """(rounded value, flagged, ulp) of the float64 values v >= 0 on their way to bf16: flagged = within delta of the midpoint between two
    neighbouring bf16 values, where an fp32 evaluation that is off by delta may land on the other neighbour; ulp = the step to it."""
    a = v.clamp(min=0)
    vb = a.float().to(torch.bfloat16)
    bits = vb.view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(torch.bfloat16).double()
    dn = (bits - 1).clamp(min=0).to(torch.int16).view(torch.bfloat16).double()
    yb = vb.double()
    near = torch.minimum((a - (yb + up) / 2).abs(), (a - (yb + dn) / 2).abs()) <= delta
    return yb, near & (v > 0), up - yb


# ---------------------------------------------------------------------------------------------------------------------------------
# The bin2mono pre-op: float64 definition and the float32 restatement of masked_log_mag
# ---------------------------------------------------------------------------------------------------------------------------------
M_CLAMP = "the clamp dropped"
M_D0 = "the d == 0 branch returning 0"
M_EXP = "exp(x) for exp(x) - 1"


def preop64(x, m, mutant=None):
    """(p, u): p = log1p(max(m expm1(x), 0)) and the scale u = |m| exp(x) + p of its fp32 error, float64."""
    x, m = x.double(), m.double()
    p = torch.log1p((m * torch.expm1(x)).clamp(min=0))
    u = m.abs() * torch.exp(x) + p
    if mutant == M_CLAMP:
        p = torch.log1p(m * torch.expm1(x))
    elif mutant == M_EXP:
        p = torch.log1p((m * torch.exp(x)).clamp(min=0))
    return p, u


def preop32(x, m, mutant=None):
    """masked_log_mag's own steps in numpy float32: e = exp2(x log2 e), z = max(m (e - 1), 0), u = 1 + z, d = u - 1,
    r = (log2(u) ln 2) (z rcp(d)), z where d == 0.  Returns (p32, shares of the three branches)."""
    f = np.float32
    x, m = x.numpy().astype(f), m.numpy().astype(f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.exp2(x * f(1.44269504088896341))
        z = np.maximum(m * (e - f(1)), f(0))
        u = f(1) + z
        d = u - f(1)
        r = (np.log2(u) * f(0.693147180559945309)) * (z * (f(1) / d))
    p = np.where(d == 0, f(0) if mutant == M_D0 else z, r).astype(f)
    n = float(p.size)
    shares = {"clamped": float((z == 0).sum()) / n, "d == 0 with z > 0": float(((d == 0) & (z > 0)).sum()) / n, "quotient": float((d != 0).sum()) / n}
    return torch.from_numpy(p), shares


def pre_ratio(row, d):
    """Worst |preop32 - p64| / u over the row's elements (0 where both are 0), and preop32's branch shares."""
    p64, u = preop64(d["mix"], d["masks"])
    p32, shares = preop32(d["mix"], d["masks"])
    err = (p32.double() - p64).abs()
    nz = u > 0
    assert bool((err[~nz] == 0).all())
    return (float((err[nz] / u[nz]).max()) if bool(nz.any()) else 0.0), shares


# ---------------------------------------------------------------------------------------------------------------------------------
# First stage
# ---------------------------------------------------------------------------------------------------------------------------------
M_HALO_ZERO = "the left halo column read as zeros"
M_HALO_HI = "the halo records without their lo half"
M_SEAM_CLASS = "an interior seam given the image border's class"
M_TOP_REPL = "the top padding row replicated"
M_GROUP_HI = "one (tap, 32-channel) group hi-only"
M_BANDS = "two frequency bands of the slice swapped"
M_LO_IN = "the lo products left in (bf16x3 passed off as HI)"


def slice_freq(t):
    """[B, 512, T, 2] -> [B, 32, 32, T]: x[b, c*16+s, h, w] = t[b, s*32+h, w, c]."""
    B, _, T, _ = t.shape
    return t.reshape(B, 16, 32, T, 2).permute(0, 4, 1, 2, 3).reshape(B, 32, 32, T)


def leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


def _col_tap(xc, w, kw):
    """What kernel column kw adds to ONE output column from the input column xc [B, C, 32, 1] it reads there: [B, 64, 16, 1]."""
    return F.conv2d(xc, w[:, :, :, kw:kw + 1], None, stride=(2, 1), padding=(1, 0))


def _tap(x, w, kh, kw):
    """What kernel tap (kh, kw) adds to the stride-2 pad-1 conv of x."""
    xp = F.pad(x, (1, 1, 1, 1))
    Ho, Wo = x.shape[2] // 2, x.shape[3] // 2
    return F.conv2d(xp[:, :, kh:kh + 2 * (Ho - 1) + 1:2, kw:kw + 2 * (Wo - 1) + 1:2], w[:, :, kh:kh + 1, kw:kw + 1])


def conv1_reference(row, d, mutant=None):
    """dict(r, s, extra, tau, ...) of a first-stage row, NHWC [B, 16, T/2, 64] float64 (module docstring): |g - r| <= tau s + extra."""
    hi, masked, Wq = row["hi"], row["masked"], row["T"] // 2
    info = {}
    w = d["w"].double()
    w32 = bf16(w[:, :32]) if hi else w[:, :32]
    s_pre = flag_ulp = None
    if masked:
        p, u = preop64(d["mix"], d["masks"], mutant)
        x32, u32 = slice_freq(p), slice_freq(u)
        if hi:
            pb, flagged, ulp = bf16_flags(x32, TAU_PRE * u32)
            info["flagged"] = float(flagged.double().mean())
            x32, flag_ulp = pb, flagged.double() * ulp
        else:
            s_pre = F.conv2d(u32 * u32, w32 * w32, None, 2, 1).sqrt()
    else:
        x32 = slice_freq(d["mix"].double())
        if hi:
            x32 = bf16(x32)
    if mutant == M_BANDS:
        x32 = x32.clone()
        for c in (0, 1):
            x32[:, [c * 16 + 3, c * 16 + 4]] = x32[:, [c * 16 + 4, c * 16 + 3]]
    xin, win = x32, w32
    if row["cls"]:   # (the kernel adds the plane from a table of the fp32 weights' sums: the plane's weights are not rounded in HI)
        plane = d["cls_val"].double().view(-1, 1, 1, 1).expand(-1, 1, 32, row["T"])
        xin, win = torch.cat((x32, plane), 1), torch.cat((w32, w[:, 32:33]), 1)
    z = F.conv2d(xin, win, None, 2, 1)
    q = F.conv2d(xin * xin, win * win, None, 2, 1).sqrt()
    seams = range(SW, Wq, SW)
    if mutant == M_HALO_ZERO:
        for r0 in seams:
            z[..., r0:r0 + 1] -= _col_tap(x32[..., 2 * r0 - 1:2 * r0], w32, 0)
    elif mutant == M_HALO_HI:
        lo = x32 - bf16(x32)
        for r0 in seams:   # the seam's two halo columns: the left one of the strip at r0, the right one of the strip before it
            z[..., r0:r0 + 1] -= _col_tap(lo[..., 2 * r0 - 1:2 * r0], w32, 0)
            z[..., r0 - 1:r0] -= _col_tap(lo[..., 2 * r0:2 * r0 + 1], w32, 3)
    elif mutant == M_SEAM_CLASS:
        for r0 in seams:
            z[..., r0:r0 + 1] -= _col_tap(plane[..., 2 * r0 - 1:2 * r0], w[:, 32:33], 0)
    elif mutant == M_TOP_REPL:
        z[:, :, 0:1] += F.conv2d(F.pad(x32[:, :, 0:1], (1, 1, 0, 0)), w32[:, :, 0:1], None, stride=(1, 2))
    elif mutant == M_GROUP_HI:
        z -= _tap(x32, w32, 1, 1) - _tap(bf16(x32), bf16(w32), 1, 1)
    sc, sh = d["scale"].double().view(1, -1, 1, 1), d["shift"].double().view(1, -1, 1, 1)
    r = leaky(z * sc + sh, 0.2)
    s = q * sc.abs() + sh.abs()
    if not hi:      # the output's split32 rounding joins the scale, as for the dst_split form of tests/test_gpu_forward_fp64.py
        tau = TAU_BF16X3
        s = s + OUT_ROUNDING * r.abs()
        extra = TAU_PRE * s_pre * sc.abs() if masked else torch.zeros_like(r)
    else:           # at TAU_FP32 that rounding is of the bound's size: it stands beside it
        tau = TAU_FP32
        f = F.conv2d(flag_ulp, w32.abs(), None, 2, 1) * sc.abs() if masked else torch.zeros_like(r)
        info["clean"] = float((f == 0).double().mean())
        extra = OUT_ROUNDING * r.abs() + f
    return dict(info, r=FR.nhwc(r), s=FR.nhwc(s), extra=FR.nhwc(extra), tau=tau)


def conv1_stand_in(row, d, kind, mutant=None):
    """CPU stand-in of the kernel, NHWC fp32: kind `fp32` a plain fp32 conv, `x3` the three split products summed in fp32; a masked row's
    input is the float32 pre-op restatement; the output is rounded as a split32 tensor."""
    x = slice_freq(preop32(d["mix"], d["masks"], mutant)[0] if row["masked"] else d["mix"])
    w = d["w"]
    if row["cls"]:
        x = torch.cat((x, d["cls_val"].view(-1, 1, 1, 1).expand(-1, 1, 32, row["T"])), 1)
    if kind == "fp32":
        z = F.conv2d(x, w, None, 2, 1)
    else:
        (xh, xl), (wh, wl) = FR.hi_lo(x), FR.hi_lo(w)
        z = F.conv2d(xh, wh, None, 2, 1) + F.conv2d(xh, wl, None, 2, 1) + F.conv2d(xl, wh, None, 2, 1)
    y = leaky(z * d["scale"].view(1, -1, 1, 1) + d["shift"].view(1, -1, 1, 1), 0.2)
    return FR.nhwc(seen32(y).float())


# ---------------------------------------------------------------------------------------------------------------------------------
# Last stage
# ---------------------------------------------------------------------------------------------------------------------------------
M_PAST_REPL = "the row past the image replicated"
M_ROW_BELOW = "row q - 1 read where q + 1 is due"
M_SOURCES = "the two sources' chunks swapped"
M_HEAD_HI = "the head reading Y's hi half only"
M_PARITY = "the row parity swapped in the de-slice"
M_BIAS_TWICE = "the head bias added twice"


def deslice(t):
    """[B, c*16, H, W] -> [B, 16*H, W, c] (m2h_oracle.deslice_freq's map)."""
    import m2h_oracle as O
    return O.deslice_freq(t).contiguous()


def _convT_kh0(x, w):
    """What kernel row 0 adds to conv_transpose2d(x, w, 2, 1): output row 2i - 1 reads input row i (i = 1 .. H; i = H is past the image).
    Returns the rows for i = 0 .. H - 1 as [B, N, H, 2W] (row i belongs at output row 2i - 1)."""
    t = F.conv_transpose2d(x, w[:, :, 0:1, :], None, stride=2, padding=(0, 1))   # [B, N, 2H - 1, 2W]: row 2i from input row i
    return t[:, :, 0::2]


def last_reference(row, d, mutant=None):
    """dict(r, s, extra, tau, ...) of a last-stage row, de-sliced [B, 32 H, 2 W, N / 16] float64 (module docstring)."""
    hi, H, N = row["hi"], row["H"], row["N"]
    rd = bf16 if hi else seen32
    x, skip, w = rd(d["x"]), rd(d["skip"]), rd(d["w"])
    xx = torch.cat((skip, x) if mutant == M_SOURCES else (x, skip), 1)
    z = F.conv_transpose2d(xx, w, None, 2, 1)
    q = F.conv_transpose2d(xx * xx, w * w, None, 2, 1).sqrt()
    if mutant == M_PAST_REPL:      # output row 2H - 1 reads input row H through kernel row 0
        z[:, :, 2 * H - 1] += _convT_kh0(xx, w)[:, :, H - 1]
    elif mutant == M_ROW_BELOW:    # odd output row 2q + 1 reads row q + 1 through kernel row 0: row q - 1 instead (zeros above the image)
        shifted = torch.zeros_like(xx)
        shifted[:, :, 2:] = xx[:, :, :H - 2]
        t = _convT_kh0(shifted - xx, w)   # row i: what input row i adds at output row 2i - 1
        for i in range(1, H):
            z[:, :, 2 * i - 1] += t[:, :, i]
        assert H >= 2
        z[:, :, 2 * H - 1] += _convT_kh0(xx, w)[:, :, H - 2]   # (q = H - 1: the zeros past the image give way to row H - 2)
    sc, sh = d["scale"].double().view(1, -1, 1, 1), d["shift"].double().view(1, -1, 1, 1)
    y = torch.relu(z * sc + sh)
    s_y = q * sc.abs() + sh.abs()
    info = {}
    hw, hb = (bf16(d["hw"]) if hi else d["hw"].double()), d["hb"].double()
    f = None
    y_head = y
    if hi:
        yb, flagged, ulp = bf16_flags(y, TAU_FP32 * s_y)
        info["flagged"] = float(flagged.double().mean())
        y_head = yb
        f = torch.einsum("jn,bnhw->bjhw", hw.abs(), flagged.double() * ulp)
        info["clean"] = float((f == 0).double().mean())
    elif mutant == M_HEAD_HI:
        y_head = bf16(y)
    r = torch.einsum("jn,bnhw->bjhw", hw, y_head) + hb.view(1, -1, 1, 1) * (2.0 if mutant == M_BIAS_TWICE else 1.0)
    s = torch.einsum("jn,bnhw->bjhw", hw * hw, s_y * s_y + y * y).sqrt() + hb.abs().view(1, -1, 1, 1)
    tau = TAU_FP32 if hi else TAU_BF16X3
    r, s, extra = deslice(r), deslice(s), deslice(f if hi else torch.zeros_like(r))
    if mutant == M_PARITY:
        B, R, W2, c = r.shape
        r = r.reshape(B, R // 2, 2, W2, c).flip(2).reshape(B, R, W2, c)
    return dict(info, r=r, s=s, extra=extra, tau=tau)


def last_stand_in(row, d, kind):
    """CPU stand-in of the kernel, de-sliced fp32: `fp32` plain fp32 convT and head; `x3` the three split products in both."""
    x, w = torch.cat((seen32(d["x"]).float(), seen32(d["skip"]).float()), 1), seen32(d["w"]).float()
    sc, sh = d["scale"].view(1, -1, 1, 1), d["shift"].view(1, -1, 1, 1)
    hw, hb = d["hw"], d["hb"].view(1, -1, 1, 1)
    if kind == "fp32":
        y = torch.relu(F.conv_transpose2d(x, w, None, 2, 1) * sc + sh)
        return deslice(torch.einsum("jn,bnhw->bjhw", hw, y) + hb)
    (xh, xl), (wh, wl) = FR.hi_lo(x), FR.hi_lo(w)
    y = torch.relu((F.conv_transpose2d(xh, wh, None, 2, 1) + F.conv_transpose2d(xh, wl, None, 2, 1) + F.conv_transpose2d(xl, wh, None, 2, 1)) * sc + sh)
    (yh, yl), (hh, hl) = FR.hi_lo(y), FR.hi_lo(hw)
    e = lambda a, b: torch.einsum("jn,bnhw->bjhw", a, b)   # noqa: E731
    return deslice(e(hh, yh) + e(hh, yl) + e(hl, yh) + hb)


# ---------------------------------------------------------------------------------------------------------------------------------
# One entry for both kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def data(row):
    return conv1_data(row) if row["kernel"].startswith("conv1") else last_data(row)


def reference(row, d, mutant=None):
    return conv1_reference(row, d, mutant) if row["kernel"].startswith("conv1") else last_reference(row, d, mutant)


def stand_in(row, d, kind, mutant=None):
    return conv1_stand_in(row, d, kind, mutant) if row["kernel"].startswith("conv1") else last_stand_in(row, d, kind)


def hi_stand_in(row, d):
    """fp32 stand-in of an HI kernel: the operands rounded to bf16, plain fp32 arithmetic, the intermediate rounded to bf16 on the way."""
    b = lambda t: t.to(torch.bfloat16).float()   # noqa: E731
    if row["kernel"].startswith("conv1"):
        x = b(slice_freq(preop32(d["mix"], d["masks"])[0] if row["masked"] else d["mix"]))
        w = d["w"].clone()
        w[:, :32] = b(w[:, :32])
        if row["cls"]:
            x = torch.cat((x, d["cls_val"].view(-1, 1, 1, 1).expand(-1, 1, 32, row["T"])), 1)
        y = leaky(F.conv2d(x, w, None, 2, 1) * d["scale"].view(1, -1, 1, 1) + d["shift"].view(1, -1, 1, 1), 0.2)
        return FR.nhwc(seen32(y).float())
    x, w = torch.cat((b(d["x"]), b(d["skip"])), 1), b(d["w"])
    y = b(torch.relu(F.conv_transpose2d(x, w, None, 2, 1) * d["scale"].view(1, -1, 1, 1) + d["shift"].view(1, -1, 1, 1)))
    return deslice(torch.einsum("jn,bnhw->bjhw", b(d["hw"]), y) + d["hb"].view(1, -1, 1, 1))


def check(g, ref, margin=1.0):
    """elem_bound.bound of g against a reference dict, with tau / margin in tau's place (the additive terms stay as they are):
    (worst (|g - r| - extra) / s in units of the row's tau, least-squares scale, holds)."""
    from elem_bound import bound
    tau = ref["tau"] / margin
    worst, scale, ok = bound(g, ref["r"], ref["s"] + ref["extra"] / tau, tau)
    return worst / ref["tau"], scale, ok


def excess(g, ref):
    """Worst (|g - r| - extra)+ / s in units of the row's tau: what the additive terms (pre-op, output rounding, flagged roundings) do
    not cover, against the summation bound alone.  A report figure; check() is what a row asserts."""
    d = ((g.double() - ref["r"]).abs() - ref["extra"]).clamp(min=0)
    nz = ref["s"] > 0
    return float((d[nz] / ref["s"][nz]).max()) / ref["tau"]


def _ids(pred):
    return [i for i in SMALL_ROWS if not ROWS[i]["hi"] and pred(ROWS[i])]


_c1r = lambda r: r["kernel"].startswith("conv1")          # noqa: E731
_lastr = lambda r: r["kernel"].startswith("last")         # noqa: E731
_normal = lambda r: r["mix"] == "normal" and r["mask"] == "normal"   # noqa: E731
MUTANT_ROWS = {
    M_HALO_ZERO: _ids(lambda r: _c1r(r) and r["T"] >= 128 and r["mix"] != "zero" and r["mask"] != "zero"),
    M_HALO_HI: _ids(lambda r: _c1r(r) and r["T"] >= 128 and _normal(r)),
    M_SEAM_CLASS: _ids(lambda r: _c1r(r) and r["cls"] and r["T"] >= 128),
    M_TOP_REPL: _ids(lambda r: _c1r(r) and _normal(r)),
    M_GROUP_HI: _ids(lambda r: _c1r(r) and _normal(r)),
    M_BANDS: _ids(lambda r: _c1r(r) and _normal(r)),
    M_CLAMP: _ids(lambda r: _c1r(r) and r["masked"] and r["mask"] == "normal" and r["mix"] in ("normal", "loud")),
    M_D0: ["c1.msk.tiny_mask.b2.t128"],
    M_EXP: _ids(lambda r: _c1r(r) and r["masked"] and r["mask"] in ("normal", "one") and r["mix"] in ("normal", "zero", "quiet")),
    M_PAST_REPL: _ids(_lastr),
    M_ROW_BELOW: _ids(lambda r: _lastr(r) and r["H"] >= 2),
    M_SOURCES: _ids(_lastr),
    M_HEAD_HI: _ids(lambda r: _lastr(r) and r["head"] == "random"),
    M_PARITY: _ids(_lastr),
    M_BIAS_TWICE: _ids(lambda r: _lastr(r) and r["head"] == "random"),
    M_LO_IN: [i for i in SMALL_ROWS if ROWS[i]["hi"]],
}
