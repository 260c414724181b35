"""The image-row 3x3 kernels of update_sep (csrc/wgrad_row3x3.hip: wgrad3x3_row_kernel<16 | 32>, wgrad3x3_row_bf16x3_kernel<16 | 32>,
wgrad3x3_row_dgrad_bf16x3_kernel; csrc/conv_row3x3.hip: conv3x3_row_kernel<FR, C>, conv3x3_row_bf16x3_kernel<FR, C>, the fused L1 epilogue and
l1_partials_sum_kernel) held to float64 element by element on every path (TEST INFRASTRUCTURE, no tests): the tables of rows, restatements
of the host's launch arithmetic, the float64 references with the bound's scale beside them, float32 stand-ins of the kernels and the named
mutants -- shared by tests/test_gpu_row3x3_kernels.py (every row on the GPU) and tests/test_row3x3_kernels_cpu.py (the rows reach every
cell, the restated arithmetic is the source's, the bound discriminates; no GPU).

Data: torch.randn from a generator seeded with train_kernels.seed_of(row id); a gate is relu(randn) (half of it exactly 0: the `> 0` side).
References (float64, from the fp32 values the kernel reads; scale rule of tests/train_kernels.py: mixed-sign sum sqrt(sum t^2), same-sign
sum sum |t|, function of sums sum |df / dsigma| s(sigma) + the final terms)
  weight gradient   dz = gate > 0 ? dy : dy * slope (one fp32 product, the kernel's own); r = wgrad64(x, dz), s = sqrt(wgrad64(x^2, dz^2)),
                    packed [N][(ty, tx, c)] or nn.Conv2d's [N][ci][3][3]
  fused             dh = dgrad64(dy2, w2), s_dh = sqrt(dgrad64(dy2^2, w2^2)); dz = dh select; r = wgrad64(x, dz),
                    s = sqrt(wgrad64(x^2, dz^2)) + wgrad64(|x|, s_dh |select|): the outer sum's own scale plus the inner error carried through.
                    The second term is a same-sign sum over all pixels: it grows like n where the first grows like sqrt(n), so the fused
                    bound is loose at many pixels (measured ratios fall with n) and a relative error of the INNER operands (w2 hi only:
                    2^-9) stays inside it but on the single-row row; that mutant is named for that row alone.  So a fused row holds a SECOND,
                    tighter bound as well: the inner errors are roundings of different sums, and x times them is a mixed-sign sum like
                    any other, s_rms = sqrt(wgrad64(x^2, dz^2)) + sqrt(wgrad64(x^2, (s_dh select)^2)), at the same tau.  Against it a
                    hi-only w2 and a dropped lo * hi term of the outer sum leave tau on EVERY fused row (MUTANT_ROWS_RMS).
  forward           forward_ref's z = conv2d(x, w, 1, 1), r = act(z + bias), s = sqrt(conv(x^2, w^2)) + |bias|; the mirrored direction
                    (functional.conv_dgrad) is conv_transpose2d(dy, w, 1, 1) built the same way
  L1                y, s_y of the conv; loss r = inv sum |y - g|, s = inv (sum |y - g| + sum s_y); the stored gradient is EXACT (+-inv, 0 where
                    y = g) on every element with |y - g| > tau s_y; the others (flagged) may carry either sign but must be one of
                    {-inv, 0, +inv}; the flagged share is held under FLAG_CAP.  y = g exactly cannot be planted from outside (y is never stored
                    and is a sum of 288 products), so the `0` value of the gradient is admitted, never demanded.
tau: elem_bound.TAU_FP32 / TAU_BF16X3 (the fused kernel too), least-squares scale included, denormal slack train_kernels.FLUSH: check().

Mutants are applied to the float64 reference (the value a kernel with that defect would give, up to its own rounding) and named only for rows
on which they can show; margins (worst |mutant - r| / s in units of tau, smallest over the rows named) are in tests/test_row3x3_kernels_cpu.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

import forward_ref as FR
import train_kernels as TK
from elem_bound import TAU_BF16X3, TAU_FP32
from rollout_kernels import MIN_MARGIN   # noqa: F401  (4x: the margin a named mutant leaves tau by)

W = C = 32
KPAD = 384                      # K = 288 padded to whole 128-wide k sub-tiles: a slab is N x KPAD floats
WG_TARGET, WG_MIN_CHUNKS, WG_SMAX = 768, 4, 1024
FW_ROWS, FW_MIN_CHUNKS, FW_CAP, FW_CAP_NARROW = 4, 512, 512, 768
KNOB_BLOCKS, KNOB_WG_ROW, KNOB_FW_ROW = 11, 21, 22
TAU = {"fp32": TAU_FP32, "x3": TAU_BF16X3}
FLAG_CAP = {"fp32": 5e-5, "x3": 5e-4}
WG_LABEL = {True: "conv_wgrad reduce (torch layout)", False: "conv_wgrad reduce"}    # (the reduce is the call's last launch: the same for the tiled kernel)
FW_LABEL = {"fp32": "conv_igemm_f32 (image-row 3x3)", "x3": "conv_igemm_bf16x3 (image-row 3x3)"}
L1_LABEL = {"fp32": "conv_igemm_f32 (image-row 3x3 + L1 loss)", "x3": "conv_igemm_bf16x3 (image-row 3x3 + L1 loss)"}


# ---------------------------------------------------------------------------------------------------------------------------------
# The launch arithmetic restated (tests/test_row3x3_kernels_cpu.py holds it against the source text and the library's size function)
# ---------------------------------------------------------------------------------------------------------------------------------
def wg_S(B, H, knob11=0):
    """Split count of a weight-gradient launch: one image row is one chunk; at least 4 chunks per split."""
    chunks = B * H
    return max(1, min(knob11 if knob11 > 0 else WG_TARGET, chunks // WG_MIN_CHUNKS, WG_SMAX))


def wg_splits(B, H, S):
    chunks = B * H
    return [(chunks * s // S, chunks * (s + 1) // S) for s in range(S)]


def wg_rule(N, ldy, knob21=0):
    """wgrad_row3x3_rule(p, true) on a 3x3 / 1 / 1 conv over [B, H, 32, 32]."""
    return N <= 32 and N % 4 == 0 and ldy % 4 == 0 and knob21 >= 0


def wg_kernel(row):
    if row["fused"]:
        return "fused"
    return "%s<%d>" % (row["math"], 16 if row["N"] <= 16 else 32)


def fw_chunks(B, H):
    return B * (H // FW_ROWS)


def fw_kernel(math, N, C0, B, H, deslice=False):
    """The instantiation launch_row3x3 takes, None where the shape is not this engine's."""
    if H % FW_ROWS or fw_chunks(B, H) < FW_MIN_CHUNKS or N > 32 or N % 4 or (deslice and N % 16) or C0 not in (16, 32):
        return None
    if math == "x3" and C0 == 16 and N <= 16:
        return None
    fr = 16 if N <= 16 else 32
    return "%s<%d,%d>" % (math, fr, C0)


def fw_grid(math, N, C0, B, H):
    cap = FW_CAP if (math == "fp32" or (N > 16 and C0 == 32)) else FW_CAP_NARROW
    return min(fw_chunks(B, H), cap)


def fw_walk(math, N, C0, B, H):
    """Per block, the chunks it walks in order: c = block, block + grid, ..."""
    grid, chunks = fw_grid(math, N, C0, B, H), fw_chunks(B, H)
    return [list(range(j, chunks, grid)) for j in range(grid)]


def fw_halo(c, H):
    """(image, first row, top halo row inside the image, bottom halo row inside the image) of forward chunk c."""
    cpi = H // FW_ROWS
    b, q0 = c // cpi, (c % cpi) * FW_ROWS
    return b, q0, q0 > 0, q0 + FW_ROWS < H


# ---------------------------------------------------------------------------------------------------------------------------------
# Weight-gradient rows
# ---------------------------------------------------------------------------------------------------------------------------------
WG_KERNELS = ("fp32<16>", "fp32<32>", "x3<16>", "x3<32>", "fused")
# (B, H, knob 11): single row; H = 1 over images; H = 2 at S = 1 and at S = 2 by default; H = 3, S = 4 with mid-image starts; S = 17; S = 16;
# B = 3, H = 7 at the default S = 5, forced S = 1 and S = 2; H = 8; B = 3, H = 32 at S = 24
WG_SHAPES = ((1, 1, 0), (5, 1, 0), (3, 2, 0), (5, 2, 0), (6, 3, 0), (17, 4, 0), (13, 5, 0), (3, 7, 0), (3, 7, 1), (3, 7, 2), (5, 8, 0), (3, 32, 0))
FUSED_SHAPES = ((1, 1, 0), (5, 1, 0), (3, 2, 0), (6, 3, 0), (13, 5, 0), (3, 7, 0), (3, 7, 1), (3, 32, 0))
WG_HEIGHTS = {k: (1, 2, 3, 4, 5, 7, 8, 32) for k in WG_KERNELS[:4]}
WG_HEIGHTS["fused"] = (1, 2, 3, 5, 7, 32)
WG_N = {"fp32<16>": (4, 8, 12, 16), "x3<16>": (4, 8, 12, 16), "fp32<32>": (20, 24, 28, 32), "x3<32>": (20, 24, 28, 32), "fused": (32,)}


def _wg_row(math, N, B, H, knob11, ldy=None, gate=None, ci=None, fused=False):
    ldy = ldy or N
    rid = "wg.%s.n%d.b%dh%d%s%s%s%s" % ("fused" if fused else math, N, B, H, ".k%d" % knob11 if knob11 else "", ".ld%d" % ldy if ldy != N else "",
                                      "" if gate is None else ".g%g" % gate, "" if ci is None else ".t%d" % ci)
    return dict(id=rid, math=math, N=N, B=B, H=H, knob11=knob11, ldy=ldy, gate=gate, ci=ci, fused=fused)


def _wg_rows():
    rows = []
    for math in ("fp32", "x3"):
        for wide in (16, 32):
            ns = WG_N["%s<%d>" % (math, wide)]
            for i, (B, H, k11) in enumerate(WG_SHAPES):
                N = ns[(i + 3) % 4]                                   # (i = 0: the full width; every N three times)
                ldy = (36 if wide == 16 else 48) if (i // 2) % 2 else N
                gate = (None, 0.0, 0.2)[i % 3]
                ci = (None, 32, 29)[(i + i // 3) % 3]
                rows.append(_wg_row(math, N, B, H, k11, ldy, gate, ci))
    for i, (B, H, k11) in enumerate(FUSED_SHAPES):
        rows.append(_wg_row("x3", 32, B, H, k11, None, (0.0, 0.2)[i % 2], (32, 29)[(i // 2) % 2], fused=True))
    return rows


WG_ROWS = {r["id"]: r for r in _wg_rows()}


def wg_cells(row):
    k, B, H = wg_kernel(row), row["B"], row["H"]
    S = wg_S(B, H, row["knob11"])
    splits = wg_splits(B, H, S)
    out = {"H %d" % H, "N %d" % row["N"]}
    if B * H == 1:
        out.add("a single row")
    if S == 1 and row["knob11"] == 1 and B > 1 and wg_S(B, H) > 1:
        out.add("S = 1 forced over several images")
    if S == 2:
        out.add("S = 2")
    if row["knob11"] == 0 and S > 1 and any(c0 % H for c0, _ in splits):
        out.add("default S, a split starts mid-image")
    if S >= 16:
        out.add("S >= 16, S % 4 == 0" if S % 4 == 0 else "S >= 16, S % 4 != 0")
    if (B, H, S) == (3, 32, 24):
        out.add("B 3, H 32: S = 24")
    if not row["fused"]:
        out.add("ldy = N" if row["ldy"] == row["N"] else "ldy > N")
        out.add("gate none" if row["gate"] is None else "gate slope %g" % row["gate"])
        out.add("packed" if row["ci"] is None else "torch ci %d" % row["ci"])
    else:
        out.add("gate slope %g" % row["gate"])
    return {(k, c) for c in out}


def wg_all_cells():
    out = set()
    for k in WG_KERNELS:
        cells = {"H %d" % h for h in WG_HEIGHTS[k]} | {"N %d" % n for n in WG_N[k]}
        cells |= {"a single row", "S = 1 forced over several images", "default S, a split starts mid-image", "gate slope 0", "gate slope 0.2"}
        if k == "fused":
            cells |= {"S >= 16, S % 4 == 0", "B 3, H 32: S = 24"}
        else:
            cells |= {"S = 2", "S >= 16, S % 4 == 0", "S >= 16, S % 4 != 0", "B 3, H 32: S = 24", "ldy = N", "ldy > N", "gate none", "packed",
                      "torch ci 32", "torch ci 29"}
        out |= {(k, c) for c in cells}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Forward / input-gradient rows and L1 rows
# ---------------------------------------------------------------------------------------------------------------------------------
FP32_INST = ((16, 32), (16, 16), (32, 32), (32, 16), (4, 32), (12, 16), (20, 32), (28, 16))
X3_INST = ((16, 32), (32, 32), (32, 16), (8, 32), (24, 32), (20, 16))
X3_OTHER = ((16, 16), (12, 16))                     # C0 = 16 with N <= 16 in bf16x3: not this engine's
FW_BASE = ((512, 4), (256, 8), (65, 32))
EPILOGUES = ("bias, slope 0", "slope 0.2", "slope 1, no bias", "de-slice", "ldc > N")
_EPI_FP32 = ("de-slice", "bias, slope 0", "de-slice", "ldc > N", "slope 0.2", "slope 1, no bias", "bias, slope 0", "slope 0.2")
_EPI_X3 = ("de-slice", "ldc > N", "bias, slope 0", "slope 1, no bias", "slope 0.2", "bias, slope 0")


def _fw_row(dir_, math, N, C0, B, H, epi="slope 1, no bias"):
    rid = "%s.%s.n%dc%d.b%dh%d%s" % (dir_, math, N, C0, B, H, {"bias, slope 0": ".bias", "slope 0.2": ".leaky", "slope 1, no bias": "", "de-slice": ".deslice",
                                                                "ldc > N": ".ldc"}[epi])
    return dict(id=rid, dir=dir_, math=math, N=N, C0=C0, B=B, H=H, epi=epi, bias=epi == "bias, slope 0", slope={"bias, slope 0": 0.0, "slope 0.2": 0.2}.get(epi, 1.0),
                deslice=epi == "de-slice", ldc=(N + 16) if epi == "ldc > N" else None)


def _fw_rows():
    rows = []
    for math, insts, epis in (("fp32", FP32_INST, _EPI_FP32), ("x3", X3_INST, _EPI_X3)):
        for i, (N, C0) in enumerate(insts):
            rows.append(_fw_row("fwd", math, N, C0, *FW_BASE[i % 3], epi=epis[i]))
            rows.append(_fw_row("dgrad", math, N, C0, *FW_BASE[(i + 1) % 3]))
    rows.append(_fw_row("fwd", "x3", 32, 32, 512, 4, "de-slice"))
    # blocks that walk more than one chunk: the prefetch under the MFMAs with its carried validity mask
    rows += [_fw_row("fwd", "fp32", 32, 32, 513, 4, "bias, slope 0"), _fw_row("fwd", "x3", 32, 32, 513, 4, "slope 0.2"),
             _fw_row("dgrad", "fp32", 32, 16, 513, 4), _fw_row("dgrad", "x3", 32, 16, 769, 4), _fw_row("fwd", "x3", 16, 32, 769, 4, "de-slice"),
             _fw_row("fwd", "fp32", 16, 32, 1100, 4, "slope 0.2"), _fw_row("dgrad", "fp32", 16, 16, 1100, 4),
             # H = 20: five chunks per image, and 512 = 2, 768 = 3 (mod 5): a block's second chunk sits elsewhere in its image than the
             # first (at H = 4, 8 and 32 the grid is a multiple of the chunks per image, and a stale validity mask would be the right one)
             _fw_row("fwd", "fp32", 32, 32, 103, 20), _fw_row("dgrad", "fp32", 16, 32, 103, 20), _fw_row("fwd", "x3", 32, 32, 103, 20),
             _fw_row("fwd", "x3", 16, 32, 154, 20), _fw_row("dgrad", "x3", 32, 16, 154, 20)]
    return rows


FW_ROWS_TABLE = {r["id"]: r for r in _fw_rows()}
OTHER_ROWS = {r["id"]: r for r in (_fw_row("fwd", "x3", N, C0, 512, 4) for N, C0 in X3_OTHER)}
L1_ROWS = {"l1.%s.b%d" % (m, B): dict(id="l1.%s.b%d" % (m, B), math=m, B=B) for m in ("fp32", "x3") for B in (64, 65, 97)}


def fw_rounds(row):
    return max(len(w) for w in fw_walk(row["math"], row["N"], row["C0"], row["B"], row["H"]))


def fw_stale_chunks(row):
    """Chunks (after a block's first) whose halo validity differs from that of the chunk the block walked before: [(chunk, previous chunk)]."""
    out = []
    for walk in fw_walk(row["math"], row["N"], row["C0"], row["B"], row["H"]):
        for prev, c in zip(walk, walk[1:]):
            if fw_halo(prev, row["H"])[2:] != fw_halo(c, row["H"])[2:]:
                out.append((c, prev))
    return out


def fw_cells(row):
    math, N, C0, B, H = (row[k] for k in ("math", "N", "C0", "B", "H"))
    k = fw_kernel(math, N, C0, B, H, row["deslice"])
    walk = fw_walk(math, N, C0, B, H)
    grid, rounds = len(walk), max(len(w) for w in walk)
    out = {(k, row["dir"]), (math, "B %d, H %d" % (B, H))}
    if rounds == 2:
        out.add((math, "two chunks in a block, grid %d" % grid))
        out.add((k, row["dir"], "two chunks"))
    elif rounds > 2:
        assert len(walk[-1]) < rounds
        out.add((math, "three rounds, the last partial"))
    if fw_stale_chunks(row):
        out.add((math, "second chunk elsewhere in its image, grid %d" % grid))
    if row["dir"] == "fwd":
        out.add((math, row["epi"] + (", N %d" % N if row["deslice"] else "")))
    return out


def fw_all_cells():
    out = set()
    for math, insts in (("fp32", FP32_INST), ("x3", X3_INST)):
        for N, C0 in insts:
            out |= {(fw_kernel(math, N, C0, 512, 4), d) for d in ("fwd", "dgrad")}
        out |= {(math, "B %d, H %d" % bh) for bh in FW_BASE + ((513, 4),)} | {(math, "two chunks in a block, grid 512")}
        out |= {(math, e) for e in EPILOGUES if e != "de-slice"} | {(math, "de-slice, N 16"), (math, "de-slice, N 32")}
        out |= {(math, "second chunk elsewhere in its image, grid 512")}
    out |= {("x3", "B 769, H 4"), ("fp32", "B 1100, H 4"), ("x3", "two chunks in a block, grid 768"), ("x3", "second chunk elsewhere in its image, grid 768"), ("fp32", "three rounds, the last partial")}
    out |= {("fp32<32,32>", "fwd", "two chunks"), ("x3<32,32>", "fwd", "two chunks"), ("fp32<32,16>", "dgrad", "two chunks"), ("x3<32,16>", "dgrad", "two chunks"),
            ("x3<16,32>", "fwd", "two chunks")}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Data
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(row):
    return torch.Generator().manual_seed(TK.seed_of(row["id"]))


def wg_data(row):
    """x [B, H, 32, 32]; dy, gate [B, H, 32, ldy] (gate None without one) -- or, fused: dy2 [B, H, 32, 16], w2 [16, 32, 3, 3], gate [B, H, 32, 32]."""
    g, B, H = _gen(row), row["B"], row["H"]
    d = dict(x=torch.randn(B, H, W, C, generator=g))
    if row["fused"]:
        d.update(dy2=torch.randn(B, H, W, 16, generator=g), w2=torch.randn(16, C, 3, 3, generator=g) * (2.0 / 288) ** 0.5,
                 gate=torch.randn(B, H, W, C, generator=g).relu_())
    else:
        d.update(dy=torch.randn(B, H, W, row["ldy"], generator=g), gate=None if row["gate"] is None else torch.randn(B, H, W, row["ldy"], generator=g).relu_())
    return d


def fw_data(row):
    """x NCHW [B, C0, H, 32], w [N, C0, 3, 3] (dgrad: the conv's own weight [C0, N, 3, 3], x its output gradient), bias [N] or None."""
    g, N, C0 = _gen(row), row["N"], row["C0"]
    x = torch.randn(row["B"], C0, row["H"], W, generator=g)
    w = torch.randn((N, C0, 3, 3) if row["dir"] == "fwd" else (C0, N, 3, 3), generator=g) * (2.0 / (9 * C0)) ** 0.5
    return dict(x=x, w=w, bias=torch.randn(N, generator=g) * 0.1 if row["bias"] else None)


def l1_data(row):
    """h NHWC [B, 32, 32, 32] = relu(randn), w [16, 32, 3, 3] = randn * 0.06, g [B, 512, 32, 1] = rand * 2."""
    g, B = _gen(row), row["B"]
    return dict(h=torch.randn(B, 32, W, C, generator=g).relu_(), w=torch.randn(16, C, 3, 3, generator=g) * 0.06, g=torch.rand(B, 512, W, 1, generator=g) * 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# Weight gradient: one walk over image rows for the float64 reference, its scale, the float32 stand-ins and the mutants
# ---------------------------------------------------------------------------------------------------------------------------------
M_PREV_IMAGE = "the row above an image's first row taken from the previous image"
M_SPLIT_FIRST = "a split's first row dropped"
M_MIRROR = "the column shift mirrored (tx <-> 2 - tx)"
M_WRAP = "no zero at pixel column -1 / 32 (wraps into the neighbouring row)"
M_GATE_STRIDE = "the gate read at stride N where ldy > N"
M_GATE_GE = "the gate compared >= 0"
M_SLOPE = "the slope ignored (0 in its place)"
M_LOHI = "the bf16x3 lo * hi term dropped"
M_F_UNGATED = "fused: the inner gradient ungated"
M_F_NOMIRROR = "fused: the inner taps not mirrored"
M_F_NEXT_IMAGE = "fused: the ring row at an image's last row taken from the next image"
M_F_W2HI = "fused: w2 hi only"
M_F_LOHI = "fused: the outer sum's lo * hi term dropped"


def wgrad(x, dz, H, mutant=None):
    """dW[n][(ty, tx, c)] = sum over rows r, pixels p of dz[r][p][n] x[row r + ty - 1 of the same image][p + tx - 1][c], in the dtype given.
    x [R, 32, C], dz [R, 32, N]: R = B H image rows."""
    R = x.shape[0]
    rows, px = torch.arange(R), torch.arange(W)
    q = rows % H
    flat = x.reshape(R * W, -1)
    taps = []
    for ty in range(3):
        ok = (q + ty - 1 >= 0) & (q + ty - 1 < H)
        if mutant == M_PREV_IMAGE and ty == 0:
            ok = rows >= 1
        src = (rows + ty - 1).clamp(0, R - 1)
        for tx in range(3):
            sx = (2 - tx) if mutant == M_MIRROR else tx
            idx = src[:, None] * W + px[None, :] + (sx - 1)
            col = px[None, :] + (sx - 1)
            valid = ((idx >= 0) & (idx < R * W)) if mutant == M_WRAP else ((col >= 0) & (col < W)).expand(R, W)
            xs = flat[idx.clamp(0, R * W - 1)] * (valid & ok[:, None]).to(x.dtype)[..., None]
            taps.append(torch.einsum("rpn,rpc->nc", dz, xs))
    return torch.stack(taps, 1).reshape(dz.shape[2], -1)


def _select(row, d, mutant=None):
    """The gate's select per element of dz [R, 32, N], fp32: 1 where gate > 0, the slope elsewhere (None without a gate)."""
    if d["gate"] is None:
        return None
    N, slope = row["N"], row["gate"]
    gate = d["gate"].reshape(-1, W, d["gate"].shape[-1])
    if mutant == M_GATE_STRIDE:
        gate = d["gate"].reshape(-1)[:gate.shape[0] * W * N].reshape(-1, W, N)
    gate = gate[..., :N]
    if mutant == M_SLOPE:
        slope = 0.0
    return torch.where((gate >= 0) if mutant == M_GATE_GE else (gate > 0), torch.ones(()), torch.full((), slope))


def _layout(row, packed):
    """packed [N][(ty, tx, c)] -> the row's layout: as it is, or nn.Conv2d's [N][ci][3][3]."""
    if row["ci"] is None:
        return packed
    return packed.reshape(packed.shape[0], 3, 3, C).permute(0, 3, 1, 2)[:, :row["ci"]].contiguous()


def _dz32(row, d, mutant=None):
    """dz in fp32 as the kernel's load makes it: dy where the gate is > 0, the fp32 product dy * slope elsewhere."""
    dy = d["dy"].reshape(-1, W, row["ldy"])[..., :row["N"]]
    sel = _select(row, d, mutant)
    dz = dy if sel is None else torch.where(sel == 1, dy, dy * sel)
    if mutant == M_SPLIT_FIRST:
        dz = dz.clone()
        for c0, _ in wg_splits(row["B"], row["H"], wg_S(row["B"], row["H"], row["knob11"]))[1:]:
            dz[c0] = 0
    return dz


def dgrad64(dy2, w2, B, H, mutant=None):
    """(dh, s_dh) [R, 32, 32] float64: the input gradient of the next conv, conv_transpose2d(dy2, w2, 1, 1), and its scale."""
    y = dy2.double().reshape(B, H, W, 16).permute(0, 3, 1, 2)
    w = w2.double()
    if mutant == M_F_W2HI:
        w = w2.to(torch.bfloat16).double()
    if mutant == M_F_NOMIRROR:
        dh = F.conv2d(y, w.permute(1, 0, 2, 3).contiguous(), None, 1, 1)
    else:
        dh = F.conv_transpose2d(y, w, None, 1, 1)
    s = F.conv_transpose2d(y * y, w * w, None, 1, 1).sqrt()
    dh, s = (t.permute(0, 2, 3, 1).reshape(B * H, W, C) for t in (dh, s))
    if mutant == M_F_NEXT_IMAGE:     # kernel row 0 reads d loss / d y of row r + 1: the next image's first row at an image's last row
        tall = dy2.double().reshape(1, B * H, W, 16).permute(0, 3, 1, 2)
        leak = F.conv_transpose2d(tall, w[:, :, 0:1, :], None, 1, (0, 1))[0].permute(1, 2, 0)     # [R, 32, 32]: what row i gives to row i - 1
        dh = dh.clone()
        for b in range(B - 1):
            dh[b * H + H - 1] += leak[(b + 1) * H]
    return dh, s


def wg_reference(row, d, mutant=None):
    """dict(r, s, tau) of a weight-gradient row in the row's layout (module docstring)."""
    B, H = row["B"], row["H"]
    x = d["x"].double().reshape(B * H, W, C)
    if row["fused"]:
        dh, s_dh = dgrad64(d["dy2"], d["w2"], B, H, mutant)
        sel = torch.where(d["gate"].reshape(B * H, W, C) > 0, 1.0, float(np.float32(row["gate"]))).double()
        if mutant == M_F_UNGATED:
            sel = torch.ones_like(sel)
        dz = dh * sel
        r = wgrad(x, dz, H)
        if mutant == M_F_LOHI:
            r = r - wgrad(x - x.float().to(torch.bfloat16).double(), dz.float().to(torch.bfloat16).double(), H)
        own = wgrad(x * x, dz * dz, H).sqrt()
        s = own + wgrad(x.abs(), s_dh * sel.abs(), H)
        s_rms = own + wgrad(x * x, (s_dh * sel) ** 2, H).sqrt()
        return dict(r=_layout(row, r), s=_layout(row, s), s_rms=_layout(row, s_rms), tau=TAU[row["math"]])
    else:
        dz = _dz32(row, d, mutant).double()
        r = wgrad(x, dz, H, mutant)
        if mutant == M_LOHI:
            r = r - wgrad(x - x.float().to(torch.bfloat16).double(), dz.float().to(torch.bfloat16).double(), H)
        s = wgrad(x * x, dz * dz, H).sqrt()
    return dict(r=_layout(row, r), s=_layout(row, s), tau=TAU[row["math"]])


def _wgrad_x3(x, dz, H):
    (xh, xl), (zh, zl) = FR.hi_lo(x), FR.hi_lo(dz)
    return wgrad(xl, zh, H) + wgrad(xh, zl, H) + wgrad(xh, zh, H)


def wg_stand_in(row, d, kind):
    """float32 stand-in of the kernel: `fp32` plain fp32 sums, `x3` three products of bf16-split operands with an fp32 sum (the fused
    kernel: in the inner gradient too, whose result is split again)."""
    B, H = row["B"], row["H"]
    x = d["x"].reshape(B * H, W, C)
    if row["fused"]:
        y = d["dy2"].permute(0, 3, 1, 2)
        (yh, yl), (wh, wl) = FR.hi_lo(y), FR.hi_lo(d["w2"])
        ct = lambda a, b: F.conv_transpose2d(a, b, None, 1, 1)   # noqa: E731
        dh = (ct(yl, wh) + ct(yh, wl) + ct(yh, wh)) if kind == "x3" else ct(y, d["w2"])
        dh = dh.permute(0, 2, 3, 1).reshape(B * H, W, C)
        dz = torch.where(d["gate"].reshape(B * H, W, C) > 0, dh, dh * row["gate"])
    else:
        dz = _dz32(row, d)
    return _layout(row, _wgrad_x3(x, dz, H) if kind == "x3" else wgrad(x, dz, H))


# ---------------------------------------------------------------------------------------------------------------------------------
# Forward and input gradient
# ---------------------------------------------------------------------------------------------------------------------------------
M_HALO_IMAGE = "the halo row of the neighbouring image at an image's first chunk"
M_STALE_MASK = "a block's later chunk staged with the previous chunk's validity mask"
M_TAPS_FORWARD = "the mirrored taps walked forward"
M_DESLICE_SWAP = "de-slice band and row swapped"
M_BIAS_AFTER = "the bias added after the activation"


def _conv_w(row, w):
    """The weight of the plain conv2d(., w, 1, 1) the row's launch computes: w itself, or (mirrored direction) w transposed and flipped."""
    return w if row["dir"] == "fwd" else w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def _out_layout(row, t, mutant=None):
    """NCHW -> the row's output layout: NHWC, or de-sliced [B, 16 H, 32, N / 16]."""
    if not row["deslice"]:
        return FR.nhwc(t)
    B, N, H, _ = t.shape
    v = t.reshape(B, N // 16, 16, H, W)
    if mutant == M_DESLICE_SWAP:
        return v.permute(0, 3, 2, 4, 1).reshape(B, 16 * H, W, N // 16).contiguous()      # frequency row h * 16 + s
    return v.permute(0, 2, 3, 4, 1).reshape(B, 16 * H, W, N // 16).contiguous()          # frequency row s * H + h (memory_nets.py:62-67)


def _epilogue(row, z, bias, mutant=None):
    if bias is None:
        return FR.act(z, row["slope"])
    b = bias.to(z.dtype).view(1, -1, 1, 1)
    return FR.act(z, row["slope"]) + b if mutant == M_BIAS_AFTER else FR.act(z + b, row["slope"])


def fw_reference(row, d, mutant=None):
    """dict(r, s, tau) of a forward / input-gradient row in its output layout, float64."""
    x, H = d["x"].double(), row["H"]
    w = _conv_w(row, d["w"].double())
    if mutant == M_TAPS_FORWARD:
        w = d["w"].double().permute(1, 0, 2, 3).contiguous()
    z = FR.conv(dict(kind="c3"), x, w)
    q = FR.conv(dict(kind="c3"), x * x, w * w).sqrt()
    if mutant == M_HALO_IMAGE:          # the rows of all images as one tall image: its row b H reads row b H - 1 through the top taps
        tall = FR.conv(dict(kind="c3"), x.permute(1, 0, 2, 3).reshape(1, x.shape[1], -1, W), w)[0].reshape(z.shape[1], -1, H, W).permute(1, 0, 2, 3)
        z = z.clone()
        z[1:, :, 0] = tall[1:, :, 0]
    elif mutant == M_STALE_MASK:
        z = z.clone()
        garbage = x[0, :, 0, 0]        # (a load the mask calls invalid is made at offset 0 of the source)
        for c, prev in fw_stale_chunks(row):
            b, q0, top, bot = fw_halo(c, H)
            _, _, ptop, pbot = fw_halo(prev, H)
            patch = torch.zeros(x.shape[1], FW_ROWS + 2, W + 2, dtype=torch.float64)
            patch[:, 1:FW_ROWS + 1, 1:W + 1] = x[b, :, q0:q0 + FW_ROWS]
            for pr, ih, real, stale in ((0, q0 - 1, top, ptop), (FW_ROWS + 1, q0 + FW_ROWS, bot, pbot)):
                if stale:
                    patch[:, pr, 1:W + 1] = x[b, :, ih] if real else garbage[:, None]
            z[b, :, q0:q0 + FW_ROWS] = F.conv2d(patch[None], w)[0]
    bias = d["bias"]
    r = _epilogue(row, z, None if bias is None else bias.double(), mutant)
    s = q if bias is None else q + bias.double().abs().view(1, -1, 1, 1)
    return dict(r=_out_layout(row, r, mutant), s=_out_layout(row, s), tau=TAU[row["math"]])


def fw_stand_in(row, d, kind):
    x, w = d["x"], _conv_w(row, d["w"])
    cv = lambda a, b: F.conv2d(a, b, None, 1, 1)   # noqa: E731
    if kind == "x3":
        (xh, xl), (wh, wl) = FR.hi_lo(x), FR.hi_lo(w)
        z = cv(xl, wh) + cv(xh, wl) + cv(xh, wh)
    else:
        z = cv(x, w)
    return _out_layout(row, _epilogue(row, z, d["bias"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# Fused L1
# ---------------------------------------------------------------------------------------------------------------------------------
M_L1_COUNT = "L1: inv with a wrong count (B 32 H T)"
M_L1_PARTIALS = "L1: partials beyond block 511 dropped"
M_L1_SIGN = "L1: the gradient's sign reversed"


def l1_inv(B):
    """The kernel's 1.f / ((float)B * 16.f * 32.f * 32.f)."""
    return np.float32(1.0) / np.float32(B * 16 * 32 * 32)


def l1_reference(row, d, mutant=None):
    """dict(loss, s_loss, grad [B, 32, 32, 16] = sign(y - g) inv in fp32, flagged, share, inv, tau); a mutant changes loss / grad only."""
    B, tau = row["B"], TAU[row["math"]]
    h, w = d["h"].double().permute(0, 3, 1, 2), d["w"].double()
    y = F.conv2d(h, w, None, 1, 1)
    s_y = F.conv2d(h * h, w * w, None, 1, 1).sqrt()
    diff = y - d["g"].double().reshape(B, 16, 32, W)            # band n, row q -> frequency row n * 32 + q
    inv = l1_inv(B)
    scale = float(inv) * (2.0 if mutant == M_L1_COUNT else 1.0)
    terms = diff.abs()
    if mutant == M_L1_PARTIALS:      # block j sums the image rows q0 + wave of its chunks j, j + grid, ...: blocks 512 .. grid - 1 lost
        keep = torch.zeros(B * 8, dtype=torch.bool)
        for j, walk in enumerate(fw_walk(row["math"], 16, 32, B, 32)):
            keep[walk] = j < 512
        terms = terms * keep.reshape(B, 1, 8, 1, 1).expand(B, 16, 8, 4, W).reshape(B, 16, 32, W)
    grad = torch.sign(diff) * (-1.0 if mutant == M_L1_SIGN else 1.0)
    flagged = diff.abs() <= tau * s_y
    return dict(loss=scale * float(terms.sum()), s_loss=float(inv) * float(diff.abs().sum() + s_y.sum()), grad=(FR.nhwc(grad).float() * np.float32(scale)),
                flagged=FR.nhwc(flagged), share=float(flagged.double().mean()), inv=inv, tau=tau)


def l1_stand_in(row, d, kind):
    """(loss, grad) in float32: the conv as fw_stand_in makes it, the loss summed in fp32."""
    y = fw_stand_in(dict(dir="fwd", deslice=False, slope=1.0), dict(x=d["h"].permute(0, 3, 1, 2), w=d["w"], bias=None), kind)      # NHWC
    diff = y - FR.nhwc(d["g"].reshape(row["B"], 16, 32, W))
    inv = l1_inv(row["B"])
    return float(diff.abs().sum(dtype=torch.float32) * inv), torch.sign(diff) * inv


def l1_check(loss, grad, ref, margin=1.0):
    """(worst |loss - r| / s in units of tau, wrong unflagged gradient elements, gradient elements outside {-inv, 0, +inv}, holds) with
    tau / margin in tau's place for the loss; the flagged set is the reference's own (at tau)."""
    tau = ref["tau"] / margin
    worst = abs(float(loss) - ref["loss"]) / (ref["s_loss"] + TK.FLUSH / tau)
    grad = grad.float().cpu()
    inv = float(ref["inv"])
    wrong = int(((grad != ref["grad"]) & ~ref["flagged"]).sum())
    outside = int(((grad != inv) & (grad != -inv) & (grad != 0)).sum())      # (NaN is outside)
    return worst / ref["tau"], wrong, outside, worst <= tau and wrong == 0 and outside == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# The bound, and the rows each mutant is named for
# ---------------------------------------------------------------------------------------------------------------------------------
def check(g, ref, margin=1.0):
    """train_kernels.check (elem_bound.bound + FLUSH) with tau / margin in tau's place: (worst |g - r| / s in units of tau, scale, holds)."""
    worst, scale, ok = TK.check(g, ref["r"], ref["s"], ref["tau"] / margin)
    return worst / ref["tau"], scale, ok


def _wg(pred):
    return [i for i, r in WG_ROWS.items() if pred(r)]


def _fw(pred):
    return [i for i, r in FW_ROWS_TABLE.items() if pred(r)]


_plain = lambda r: not r["fused"]                                   # noqa: E731
_S = lambda r: wg_S(r["B"], r["H"], r["knob11"])                     # noqa: E731
MUTANT_ROWS = {
    # (a forced S = 1 or a large H puts many rows between two image edges: the edge's share of the sum is smallest there, and still shows)
    M_PREV_IMAGE: _wg(lambda r: _plain(r) and r["B"] >= 2),
    M_SPLIT_FIRST: _wg(lambda r: _plain(r) and _S(r) >= 2),
    M_MIRROR: _wg(_plain),
    M_WRAP: _wg(lambda r: _plain(r) and r["B"] * r["H"] >= 2),
    M_GATE_STRIDE: _wg(lambda r: _plain(r) and r["gate"] is not None and r["ldy"] > r["N"]),
    M_GATE_GE: _wg(lambda r: _plain(r) and r["gate"] is not None),
    M_SLOPE: _wg(lambda r: _plain(r) and r["gate"] == 0.2),
    M_LOHI: _wg(lambda r: _plain(r) and r["math"] == "x3"),
    M_F_UNGATED: _wg(lambda r: r["fused"]),
    M_F_NOMIRROR: _wg(lambda r: r["fused"]),
    M_F_NEXT_IMAGE: _wg(lambda r: r["fused"] and r["B"] >= 2),
    M_F_W2HI: _wg(lambda r: r["fused"] and r["B"] * r["H"] == 1),
    M_HALO_IMAGE: _fw(lambda r: True),
    M_STALE_MASK: _fw(lambda r: bool(fw_stale_chunks(r))),
    M_TAPS_FORWARD: _fw(lambda r: r["dir"] == "dgrad"),
    M_DESLICE_SWAP: _fw(lambda r: r["deslice"]),
    M_BIAS_AFTER: _fw(lambda r: r["bias"]),
    M_L1_COUNT: list(L1_ROWS),
    M_L1_PARTIALS: ["l1.x3.b97"],
    M_L1_SIGN: list(L1_ROWS),
}
# against the fused kernel's second, tighter scale (wg_reference's s_rms), on every fused row
MUTANT_ROWS_RMS = {M_F_W2HI: _wg(lambda r: r["fused"]), M_F_LOHI: _wg(lambda r: r["fused"])}


def rms(ref):
    """The fused row's reference with s_rms in the scale's place."""
    return dict(ref, s=ref["s_rms"])
