"""The training kernels beyond the convolutions (TEST INFRASTRUCTURE): csrc/bn.hip and the training units csrc/rnn.hip,
policy_heads.hip, losses.hip and optim.hip -- their
restated dispatch, the table of test rows, the float64 reference of every row with its element-wise error scale, float32 numpy
restatements of each kernel's algorithm, and mutants of those restatements that the bound must reject.

tests/test_gpu_train_kernels.py runs every row on the GPU against ``reference`` by ``elem_bound.bound``; tests/test_train_kernels_cpu.py
checks without a GPU that the rows reach every cell of ``all_cells()``, that every float32 restatement stays inside the family's tau on
every row, and that every mutant leaves it on the rows named for it (so the scales are anchored before any GPU run).

The scale s of a reference element, under one rule:
  * a sum of mixed-sign products t_m:                     s = sqrt(sum t_m^2)   (elem_bound's scale)
  * a sum of same-sign terms (loss sums, sums of squares): s = sum |t_m|
  * an output f(sigma_1 .. sigma_p) of such sums:          s = sum_i |df/dsigma_i| s(sigma_i) + the magnitudes of the terms of the final
    expression (derivatives from float64 autograd with the sums as leaves, or written out where they are one line)
  * BatchNorm: y: |gamma| invstd (|x| + |mean|) + |beta|;  mean: sqrt(sum x^2) / M;  invstd: relative, against sqrt(1 + mean^2 / (var + eps))
Checks are LOCAL: a kernel that consumes another kernel's output (a backward its forward's saved tensors, Adam step k the state step k - 1
left) is referenced in float64 from the float32 values it was handed, so an error is charged to the kernel that made it.
"""
import zlib

import numpy as np
import torch

from elem_bound import TAU_FP32, bound

F32 = np.float32
# A float32 intermediate below the smallest normal 2^-126 may flush to zero (a saturated gate is 1e-38 or less); it reaches an output through
# factors of the inputs' size, below 16 in these kernels: an absolute slack of 16 * 2^-126 on every inexact element.
FLUSH = 16 * 2.0 ** -126
FAMILIES = ("bn", "gru", "gru_seq", "lstm", "heads", "loss", "adam")
# The family bounds (the header of tests/test_gpu_train_kernels.py records the ratios measured on an MI355X).  TAU_FP32 for every family of
# single kernels: their worst ratios sit at 1.3e-6 and below, but for BatchNorm's mean at 5.5e-6 -- the rounding of a mean near 100 to float32
# (half an ulp: 3.8e-6) against a scale 100 / sqrt(M) that the issue's rule lets shrink with M; it stays under TAU_FP32 for the M <= 5000 of
# the rows, so the family keeps the stricter constant.  gru_seq: its outputs are held against the scale of the step that makes them, which
# leaves out the error of that step's inputs (a bias gradient over T N = 1 rows is ONE gate gradient: s = |t|, its own cancellation unseen);
# measured worst 2.56e-5 (g_wih, T N = 1 and 2), times 8.
TAU = {f: TAU_FP32 for f in FAMILIES}
TAU["gru_seq"] = 2e-4


def cdiv(a, b):
    return (a + b - 1) // b


def check(g, r, s, tau, lsq=None):
    """elem_bound.bound, with the least-squares scale taken over the last-axis columns `lsq` only where given: BatchNorm's y on a large-mean
    channel carries, by its stated scale, an error of cond * eps RELATIVE to y that one mean error gives to every row alike, which the
    element bound admits and a least-squares scale within tau cannot."""
    g, r, s = (torch.as_tensor(t).double() for t in (g, r, s))
    s = torch.where(s > 0, s + FLUSH / tau, s)        # (s = 0 still asks for the exact value)
    worst, scale, ok = bound(g, r, s, tau)
    if lsq is not None:
        scale = bound(g[..., lsq], r[..., lsq], s[..., lsq], tau)[1]
        ok = worst <= tau and abs(scale - 1.0) <= tau
    return worst, scale, ok


def seed_of(row_id):
    return zlib.crc32(row_id.encode())


def _gen(row_id):
    return torch.Generator().manual_seed(seed_of(row_id))


def _np(t):
    return t.detach().cpu().numpy().astype(F32)


def _t64(a):
    return torch.as_tensor(np.asarray(a)).double()


def grid_for(total, cap=4096):
    """rl_common.h grid_for: blocks of 256 threads, capped."""
    return max(1, min(cdiv(total, 256), cap))


def enters_grid_stride_loop(total, cap):
    """A thread of the launch takes more than one element (the grid-stride loop's second iteration)."""
    return total > grid_for(total, cap) * 256


# ----------------------------------------------------------------------------------------------------------------------------------
# ordered float32 sums of the reductions (numpy restatements)
# ----------------------------------------------------------------------------------------------------------------------------------
def wave_tree(v):
    """Lane 0 of a 64-lane shuffle tree (offsets 32 .. 1; __shfl_down and the __shfl_xor butterfly pair the same way for lane 0).  v [64, ...]."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:off] + v[off:2 * off]
    return v[0]


def block_sum256(v):
    """rl_common.h block_sum: per-wave tree, then the four waves left to right.  v [256, ...]."""
    w = [wave_tree(v[64 * i:64 * i + 64]) for i in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def grid_sum(terms, cap, final_threads=64):
    """l1_loss / bin_l1 / sumsq: grid-stride thread sums, block_sum per block, then the partials lane-strided over one wave and a tree."""
    terms = np.asarray(terms, dtype=F32).reshape(-1)
    n = terms.size
    G = grid_for(n, cap)
    T = G * 256
    it = cdiv(n, T)
    pad = np.zeros(it * T, dtype=F32)
    pad[:n] = terms
    pad = pad.reshape(it, T)
    s = np.zeros(T, dtype=F32)
    for i in range(it):
        s = s + pad[i]
    parts = np.stack([block_sum256(s[256 * b:256 * b + 256]) for b in range(G)]).astype(F32)
    return lane_strided_sum(parts, final_threads)


def lane_strided_sum(parts, threads=64):
    """sum_partials / clip_coef (64 lanes + tree) and sum_partials_wide (1024 threads: 16 wave trees, then the waves in order)."""
    k = cdiv(parts.size, threads)
    pad = np.zeros(k * threads, dtype=F32)
    pad[:parts.size] = parts
    pad = pad.reshape(k, threads)
    s = np.zeros(threads, dtype=F32)
    for i in range(k):
        s = s + pad[i]
    if threads == 64:
        return F32(wave_tree(s))
    t = F32(0)
    for w in range(threads // 64):
        t = F32(t + wave_tree(s[64 * w:64 * w + 64]))
    return t


# ----------------------------------------------------------------------------------------------------------------------------------
# BatchNorm (csrc/bn.hip)
# ----------------------------------------------------------------------------------------------------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
BN_NT, BN_RMAX = 256, 16           # bn.hip BNS_NT, BNS_RMAX


def bn_route(M, C, knob37=0):
    """bn.hip bn_small_rows / bn_splits / m2h_bn_train_fwd: the label, rows per thread R of the one-launch kernels (0: the three-launch
    path), and the three-launch path's split geometry."""
    lim = knob37 if knob37 > 0 else 256
    R = 0
    if knob37 >= 0 and C % 4 == 0 and M <= lim and M <= BN_RMAX * BN_NT:
        R = 1 if M <= BN_NT else 4 if M <= 4 * BN_NT else 16
    colblocks = cdiv(C, 64)
    splits = max(1, min(cdiv(1024, colblocks), cdiv(M, 32)))
    rps = cdiv(M, splits)
    empty = splits - cdiv(M, rps)
    return dict(label="one launch" if R else "three launches", R=R, splits=splits, rps=rps, empty=empty, colblocks=colblocks,
                workspace=splits * C * 3 * 4, kernel="bn_train_%s (one launch)" if R else "bn_train_%s")


BN_CELLS = ("one launch, R=1", "one launch, R=4", "one launch, R=16", "three launches", "default limit: 256 rows, one launch",
            "default limit: 257 rows, three launches", "three launches, M=2", "three launches, two splits",
            "three launches, final lane loop wraps (splits > 64)", "three launches, ragged second column block",
            "three launches, empty trailing splits", "three launches beyond the one-launch kernels' 4096 rows (knob 4096)",
            "knob 37 = -1 forces three launches", "one launch, M=2", "slope 0.0", "slope 0.2")


def _bn_row(M, C, knob, slope):
    return dict(id="bn.M%d.C%d.k%d.s%s" % (M, C, knob, slope), family="bn", M=M, C=C, knob=knob, slope=slope)


BN_SHAPES = [(2, 4, 0), (255, 12, 0), (256, 64, 0), (257, 64, 4096), (1024, 8, 4096), (1025, 4, 4096), (4096, 16, 4096), (257, 64, 0),
             (2, 4, -1), (33, 4, -1), (2081, 68, 0), (5000, 512, 0), (4097, 4, 4096)]
BN_ROWS = [_bn_row(M, C, k, s) for (M, C, k) in BN_SHAPES for s in (0.0, 0.2)]


def bn_cells(row):
    rt = bn_route(row["M"], row["C"], row["knob"])
    M, C, knob = row["M"], row["C"], row["knob"]
    out = {"slope %s" % row["slope"]}
    if rt["R"]:
        out.add("one launch, R=%d" % rt["R"])
        if M == 2:
            out.add("one launch, M=2")
        if M == 256 and knob == 0:
            out.add(BN_CELLS[4])
        return out
    out.add("three launches")
    if M == 257 and knob == 0:
        out.add(BN_CELLS[5])
    if M == 2:
        out.add(BN_CELLS[6])
    if rt["splits"] == 2:
        out.add(BN_CELLS[7])
    if rt["splits"] > 64:
        out.add(BN_CELLS[8])
    if C > 64 and C % 64:
        out.add(BN_CELLS[9])
    if rt["empty"] > 0:
        out.add(BN_CELLS[10])
    if knob > 0 and M > BN_RMAX * BN_NT:
        out.add(BN_CELLS[11])
    if knob < 0 and M <= 256:
        out.add(BN_CELLS[12])
    return out


def bn_channel_kinds(C):
    """Channel kinds inside one row: 'large' (mean 100, std 0.01: where a one-pass variance cancels), one 'const' channel, ordinary ones."""
    return ["const" if c == 2 else "large" if c % 4 == 1 else "plain" for c in range(C)]


def bn_lsq(name, C):
    """Columns of an output that take part in the least-squares scale (see check): all, but for y the channels that are not large-mean."""
    return [c for c, k in enumerate(bn_channel_kinds(C)) if k != "large"] if name == "y" else None


def bn_inputs(row):
    g = _gen(row["id"])
    M, C = row["M"], row["C"]
    z = torch.randn(M, C, generator=g) * 1.7 + 0.4
    for c, kind in enumerate(bn_channel_kinds(C)):
        if kind == "large":
            z[:, c] = 100.0 + 0.01 * torch.randn(M, generator=g)
        elif kind == "const":
            z[:, c] = 3.0
    return dict(z=z, gamma=1.0 + 0.3 * torch.randn(C, generator=g), beta=0.2 * torch.randn(C, generator=g),
                running_mean=torch.randn(C, generator=g), running_var=1.0 + torch.rand(C, generator=g), dy=torch.randn(M, C, generator=g))


def bn_reference(row, inp, state):
    """state: the float32 y, mean, invstd the backward under test was handed (its own forward's).  -> {name: (r, s)} in float64."""
    M, slope = row["M"], row["slope"]
    z, ga, be = inp["z"].double(), inp["gamma"].double(), inp["beta"].double()
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    cond = torch.sqrt(1.0 + mean * mean / (var + BN_EPS))
    s_mean = torch.sqrt((z * z).sum(0)) / M
    v = (z - mean) * invstd * ga + be
    var_u = var * M / (M - 1)
    rm, rv = inp["running_mean"].double(), inp["running_var"].double()
    out = {"mean": (mean, s_mean), "invstd": (invstd, invstd * cond),
           "y": (torch.where(v > 0, v, v * slope), ga.abs() * invstd * (z.abs() + mean.abs()) + be.abs()),
           "running_mean": ((1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean, BN_MOMENTUM * s_mean + (1 - BN_MOMENTUM) * rm.abs() + BN_MOMENTUM * mean.abs()),
           "running_var": ((1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var_u,
                           BN_MOMENTUM * 2 * (var_u + BN_EPS) * cond + (1 - BN_MOMENTUM) * rv.abs() + BN_MOMENTUM * var_u)}
    # backward, from the float32 y / mean / invstd it was handed: g = dy act'(y), xh = (z - mean) invstd
    y32, mu, isd = state["y"].double(), state["mean"].double(), state["invstd"].double()
    g = torch.where(y32 > 0, inp["dy"].double(), inp["dy"].double() * slope)
    xh = (z - mu) * isd
    dbeta, s_db = g.sum(0), torch.sqrt((g * g).sum(0))
    dgamma, s_dg = (g * xh).sum(0), torch.sqrt(((g * xh) ** 2).sum(0))
    k = (ga * isd).abs()
    dz = ga * isd * (g - dbeta / M - xh * dgamma / M)
    s_dz = k * (s_db / M + xh.abs() * s_dg / M + g.abs() + dbeta.abs() / M + (xh * dgamma).abs() / M)
    out.update({"dbeta": (dbeta, s_db), "dgamma": (dgamma, s_dg), "dz": (dz, s_dz)})
    return out


def _wf_combine(a, b):
    """bn.hip wf_combine on (n, mean, m2) float32 arrays."""
    with np.errstate(all="ignore"):
        n = a[0] + b[0]
        d = b[1] - a[1]
        mean = a[1] + d * (b[0] / n)
        m2 = a[2] + b[2] + d * d * (a[0] * b[0] / n)
    ea, eb = a[0] == 0, b[0] == 0
    return tuple(np.where(eb, xa, np.where(ea, xb, x)).astype(F32) for x, xa, xb in ((n, a[0], b[0]), (mean, a[1], b[1]), (m2, a[2], b[2])))


def _split_rows(M, splits, rps, NW):
    """Row index [splits][NW][k] and validity of the partial kernels' loops: wave w of split s takes rows s rps + w, + NW, ... in order."""
    steps = cdiv(rps, NW)
    rows = (np.arange(splits)[:, None, None] * rps + np.arange(NW)[None, :, None] + NW * np.arange(steps)[None, None, :])
    end = np.minimum(M, (np.arange(splits) + 1) * rps)[:, None, None]
    return rows, rows < end


def bn_stats_welford(z, rt, drop_row=None):
    """bn_stats_partial_kernel + bn_stats_final_kernel: per-wave streaming Welford in row order, the four waves pairwise, lane l of the
    final stage folds splits l, l + 64, ... in order, then the shuffle tree.  -> (n, mean, m2) per channel."""
    M, C = z.shape
    splits, rps = rt["splits"], rt["rps"]
    rows, ok = _split_rows(M, splits, rps, 4)
    if drop_row is not None:
        ok = ok & (rows != drop_row)
    n = np.zeros((splits, 4, 1), dtype=F32)
    mean = np.zeros((splits, 4, C), dtype=F32)
    m2 = np.zeros((splits, 4, C), dtype=F32)
    for k in range(rows.shape[2]):
        x = z[np.minimum(rows[:, :, k], M - 1)]
        v = ok[:, :, k][:, :, None]
        n1 = (n + F32(1)).astype(F32)
        d = x - mean
        mean1 = mean + d / n1
        m21 = m2 + d * (x - mean1)
        n, mean, m2 = np.where(v, n1, n), np.where(v, mean1, mean).astype(F32), np.where(v, m21, m2).astype(F32)
    n = np.broadcast_to(n, mean.shape).astype(F32)
    w = [(n[:, i], mean[:, i], m2[:, i]) for i in range(4)]
    part = _wf_combine(_wf_combine(w[0], w[1]), _wf_combine(w[2], w[3]))     # [splits][C]
    r = tuple(np.zeros((64, C), dtype=F32) for _ in range(3))
    for s0 in range(0, splits, 64):
        b = tuple(np.zeros((64, C), dtype=F32) for _ in range(3))
        k = min(64, splits - s0)
        for dst, src in zip(b, part):
            dst[:k] = src[s0:s0 + k]
        r = _wf_combine(r, b)
    for off in (32, 16, 8, 4, 2, 1):
        r = _wf_combine(tuple(x[:off] for x in r), tuple(x[off:2 * off] for x in r))
    return tuple(x[0] for x in r)


def _thread_rows(a, R, M):
    """[M][C] -> [R][256][C] as the one-launch kernels hold it (thread t: rows t, t + 256, ...) and the validity mask."""
    C = a.shape[1]
    pad = np.zeros((R * BN_NT, C), dtype=F32)
    pad[:M] = a
    ok = (np.arange(R * BN_NT) < M).reshape(R, BN_NT, 1)
    return pad.reshape(R, BN_NT, C), ok


def _block_sum4(v):
    """bn.hip block_sum4: per-wave shuffle tree, then (w0 + w1) + (w2 + w3).  v [256][C]."""
    w = [wave_tree(v[64 * i:64 * i + 64]) for i in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


def bn_stats_two_pass(z, R, drop_row=None):
    """bn_fwd_small_kernel: the mean, then the centred sum of squares, both over the registers."""
    M, C = z.shape
    x, ok = _thread_rows(z, R, M)
    if drop_row is not None:
        ok = ok & (np.arange(R * BN_NT) != drop_row).reshape(R, BN_NT, 1)
    cnt = F32(M if drop_row is None else M - 1)
    s = np.zeros((BN_NT, C), dtype=F32)
    for j in range(R):
        s = s + np.where(ok[j], x[j], F32(0))
    mu = (_block_sum4(s) * (F32(1) / cnt)).astype(F32)
    q = np.zeros((BN_NT, C), dtype=F32)
    for j in range(R):
        d = x[j] - mu
        q = q + np.where(ok[j], d * d, F32(0))
    return np.full(C, cnt, dtype=F32), mu, _block_sum4(q).astype(F32)


def bn_stats_one_pass(z):
    """MUTANT: var = E[x^2] - E[x]^2 in float32."""
    M = F32(z.shape[0])
    s, q = z.sum(0, dtype=F32), (z * z).sum(0, dtype=F32)
    mu = (s / M).astype(F32)
    return np.full(z.shape[1], M, dtype=F32), mu, np.maximum(q - M * mu * mu, F32(0)).astype(F32)


def _bwd_sums(g, gx, row, rt):
    """The two column sums of the backward in the kernel's order (one launch: thread-sequential + block_sum4; three launches: per-wave row
    order, the waves left to right, lane-strided splits, the shuffle tree)."""
    M, C = g.shape
    out = []
    for t in (g, gx):
        if rt["R"]:
            x, ok = _thread_rows(t, rt["R"], M)
            s = np.zeros((BN_NT, C), dtype=F32)
            for j in range(rt["R"]):
                s = s + np.where(ok[j], x[j], F32(0))
            out.append(_block_sum4(s).astype(F32))
            continue
        rows, ok = _split_rows(M, rt["splits"], rt["rps"], 4)
        s = np.zeros((rt["splits"], 4, C), dtype=F32)
        for k in range(rows.shape[2]):
            s = s + np.where(ok[:, :, k][:, :, None], t[np.minimum(rows[:, :, k], M - 1)], F32(0))
        part = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
        lanes = np.zeros((64, C), dtype=F32)
        for s0 in range(0, rt["splits"], 64):
            k = min(64, rt["splits"] - s0)
            lanes[:k] = lanes[:k] + part[s0:s0 + k]
        out.append(wave_tree(lanes).astype(F32))
    return out


BN_MUTANTS = ("one-pass variance", "one row left out of one split", "biased variance in running_var", "dbeta/M dropped from dz")


def bn_fp32(row, inp, mutant=None):
    """The float32 restatement of m2h_bn_train_fwd + m2h_bn_train_bwd on the row (the backward from the restated forward's y, mean, invstd).
    -> ({name: float32 array}, state for bn_reference)."""
    M, slope = row["M"], F32(row["slope"])
    rt = bn_route(M, row["C"], row["knob"])
    z, ga, be, dy = (_np(inp[k]) for k in ("z", "gamma", "beta", "dy"))
    drop = (M // 2 if M > 2 else 1) if mutant == BN_MUTANTS[1] else None
    if mutant == BN_MUTANTS[0]:
        n, mu, m2 = bn_stats_one_pass(z)
    elif rt["R"]:
        n, mu, m2 = bn_stats_two_pass(z, rt["R"], drop)
    else:
        n, mu, m2 = bn_stats_welford(z, rt, drop)
    eps, mom = F32(BN_EPS), F32(BN_MOMENTUM)
    var_b = (m2 / n).astype(F32)
    isd = (F32(1) / np.sqrt(var_b + eps)).astype(F32)
    var_u = np.where(n > 1, m2 / np.maximum(n - F32(1), F32(1)), var_b).astype(F32)
    if mutant == BN_MUTANTS[2]:
        var_u = var_b
    v = ((z - mu) * isd * ga + be).astype(F32)
    y = np.where(v > 0, v, v * slope).astype(F32)
    out = {"mean": mu, "invstd": isd, "y": y,
           "running_mean": ((F32(1) - mom) * _np(inp["running_mean"]) + mom * mu).astype(F32),
           "running_var": ((F32(1) - mom) * _np(inp["running_var"]) + mom * var_u).astype(F32)}
    g = np.where(y > 0, dy, dy * slope).astype(F32)
    xh = ((z - mu) * isd).astype(F32)
    db, dg = _bwd_sums(g, (g * xh).astype(F32), row, rt)
    invM = F32(1) / F32(M)
    dbm = F32(0) if mutant == BN_MUTANTS[3] else db * invM
    out.update({"dbeta": db, "dgamma": dg, "dz": (ga * isd * (g - dbm - xh * dg * invM)).astype(F32)})
    state = {k: torch.from_numpy(out[k]) for k in ("y", "mean", "invstd")}
    return out, state


# ----------------------------------------------------------------------------------------------------------------------------------
# GRU kernels, one step (rnn.hip: gru_gates, gru_step, gru_cell, gru_gates_bwd, gru_bwd_rec / gru_bwd_step, gru_bwd_combine)
# ----------------------------------------------------------------------------------------------------------------------------------
GRU_STEP_MAX_ROWS = 16
GRU_WAVES = {"gru_step": 8, "gru_cell": 16, "gru_bwd_rec": 16, "gru_bwd_step": 16}    # GS_NW, GC_NW, GB_NW


def gru_route(N, H, T):
    """functional.py GRUSequence: the fused per-step kernels (N <= 16 rows and H % 16 == 0) or GEMM + gates, and the backward's kernels."""
    fused = N <= GRU_STEP_MAX_ROWS and H % 16 == 0
    if fused:
        bwd = ["gru_gates_bwd"] + (["gru_bwd_step"] if T > 1 else []) + ["gru_bwd_rec"]     # gates_bwd at t = T - 1, rec alone at t = 0
    else:
        bwd = ["gru_gates_bwd", "gru_bwd_combine"]
    return dict(fused=fused, forward="gru_step" if fused else "gru.hh GEMM + gru_gates", backward=bwd)


def _gru_row(kernel, M, H, I=0, mask="none", a=True, sat=False):
    rid = "%s.M%d.H%d%s.%s%s%s" % (kernel, M, H, ".I%d" % I if I else "", mask, "" if a else ".noa", ".sat" if sat else "")
    return dict(id=rid, family="gru", kernel=kernel, M=M, H=H, I=I, mask=mask, a=a, sat=sat)


def _gru_rows():
    R = []
    for M in (1, 14, 16):
        for H, I in ((16, 16), (64, 96), (512, 1536)):
            for mask in ("none", "mixed"):
                R.append(_gru_row("gru_step", M, H, mask=mask))
                R.append(_gru_row("gru_cell", M, H, I=I, mask=mask))
            for a in (True, False):
                R.append(_gru_row("gru_bwd_rec", M, H, mask="mixed" if a else "none", a=a))
                R.append(_gru_row("gru_bwd_step", M, H, mask="none" if a else "mixed", a=a))
    for (M, H) in ((17, 20), (14, 512)):
        for mask in ("none", "mixed"):
            R.append(_gru_row("gru_gates", M, H, mask=mask))
            R.append(_gru_row("gru_gates_bwd", M, H, mask=mask))
    R += [_gru_row("gru_bwd_combine", 17, 20, mask="mixed", a=True), _gru_row("gru_bwd_combine", 17, 20, mask="none", a=False)]
    R += [_gru_row(k, 14, 64, I=96 if k == "gru_cell" else 0, mask="mixed", sat=True)
          for k in ("gru_gates", "gru_step", "gru_cell", "gru_gates_bwd", "gru_bwd_step")]
    return R


GRU_ROWS = _gru_rows()


def gru_cells(row):
    k, M, H = row["kernel"], row["M"], row["H"]
    out = {(k, "M=%d" % M, "H=%d" % H), (k, "mask " + row["mask"])}
    if k in GRU_WAVES:
        Ks = {"gru_step": [H], "gru_cell": [row["I"], H], "gru_bwd_rec": [3 * H], "gru_bwd_step": [3 * H]}[k]
        if any(K // 16 < GRU_WAVES[k] for K in Ks):
            out.add((k, "waves with zero k-steps"))
        if M == 1:
            out.add((k, "every tile row is the clamped row 0"))
    if k in ("gru_bwd_rec", "gru_bwd_step", "gru_bwd_combine"):
        out.add((k, "a present" if row["a"] else "a absent"))
    if row["sat"]:
        out.add((k, "saturated pre-activations"))
    return out


def gru_all_cells():
    out = set()
    for k in ("gru_step", "gru_cell", "gru_bwd_rec", "gru_bwd_step"):
        out |= {(k, "M=%d" % M, "H=%d" % H) for M in (1, 14, 16) for H in (16, 64, 512)}
        out |= {(k, "waves with zero k-steps"), (k, "every tile row is the clamped row 0")}
    for k in ("gru_gates", "gru_gates_bwd"):
        out |= {(k, "M=17", "H=20"), (k, "M=14", "H=512")}
    out.add(("gru_bwd_combine", "M=17", "H=20"))
    for k in ("gru_step", "gru_cell", "gru_gates", "gru_gates_bwd", "gru_bwd_rec", "gru_bwd_step", "gru_bwd_combine"):
        out |= {(k, "mask none"), (k, "mask mixed")}
    for k in ("gru_bwd_rec", "gru_bwd_step", "gru_bwd_combine"):
        out |= {(k, "a present"), (k, "a absent")}
    out |= {(k, "saturated pre-activations") for k in ("gru_gates", "gru_step", "gru_cell", "gru_gates_bwd", "gru_bwd_step")}
    return out


def _mask(g, M, kind):
    if kind == "none":
        return None
    m = (torch.rand(M, generator=g) > 0.4).float()
    m[M // 2] = 0.0                                  # at least one zero row
    if M > 1:
        m[0] = 1.0
    return m


def _sat_pattern(H, G):
    """+-90 over the units of G gate blocks, every sign combination of the blocks among the first units."""
    j = torch.arange(H)
    return torch.cat([torch.where((j >> b) % 2 == 0, 90.0, -90.0) for b in range(G)])


def gru_inputs(row):
    g = _gen(row["id"])
    k, M, H, I = row["kernel"], row["M"], row["H"], row["I"]
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(gi=rn(M, 3 * H), gh=rn(M, 3 * H), bhh=0.3 * rn(3 * H), hprev=0.7 * rn(M, H), mask=_mask(g, M, row["mask"]),
             whh=rn(3 * H, H) / H ** 0.5, dh=rn(M, H))
    if k == "gru_cell":
        d.update(x=rn(M, I), wih=rn(3 * H, I) / I ** 0.5, bih=0.3 * rn(3 * H))
    if k in ("gru_bwd_rec", "gru_bwd_step", "gru_bwd_combine"):
        d.update(dpre=rn(M, 3 * H), a=rn(M, H) if row["a"] else None, dhp=rn(M, H), rec=rn(M, H),
                 mask_p=_mask(g, M, row["mask"]), hprev_p=0.7 * rn(M, H))
    if row["sat"]:
        pat = _sat_pattern(H, 3)
        if k == "gru_cell":       # the input projection itself lands near +-90: row 0 of x is 90 on three inputs, which only gate b's weight
            d["x"][0] = 0.0       # rows read (column b: the pattern / 90)
            d["x"][0, :3] = 90.0
            d["wih"][:, :3] = 0.0
            for b in range(3):
                d["wih"][b * H:(b + 1) * H, b] = pat[b * H:(b + 1) * H] / 90.0
        else:
            d["gi"][0] = pat + 0.5 * rn(3 * H)
    return d


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _dot_ref(x, w):
    """x [M,K] . w [R,K]^T in float64 with the mixed-sign scale sqrt(sum t^2)."""
    x, w = x.double(), w.double()
    return x @ w.t(), torch.sqrt((x * x) @ (w * w).t())


def _units(fn, leaves, scales, H):
    """Outputs [M,H] of fn(*leaves) whose element (m, j) depends on the leaves' elements (m, gate, j) only: sum_i |d out / d leaf_i| s_i
    from one float64 backward pass per output (each leaf element feeds one element of the output)."""
    leaves = [l.clone().requires_grad_(True) for l in leaves]
    outs = fn(*leaves)
    res = []
    for o in outs:
        gs = torch.autograd.grad(o.sum(), leaves, retain_graph=True, allow_unused=True)
        s = torch.zeros_like(o)
        for gl, sc in zip(gs, scales):
            if gl is not None:
                t = gl.abs() * sc
                t = torch.where(sc > 0, t, torch.zeros_like(t))
                s = s + t.view(o.shape[0], -1, H).sum(1)
        res.append((o.detach(), s))
    return res


def _gates64(gi, ghb_s, hp, m, H):
    """r, z, n, hn of the GRU gates from gi and the masked, biased recurrent pre-activation ghb = m gh + b (float64 tensors)."""
    r = _sig(gi[:, :H] + ghb_s[:, :H])
    z = _sig(gi[:, H:2 * H] + ghb_s[:, H:2 * H])
    hn = ghb_s[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * hn)
    return r, z, n, hn


def _mcol(mask, M):
    return (torch.ones(M) if mask is None else mask).double().view(M, 1)


def _gru_fwd_ref(gi, s_gi, gh, s_gh, bhh, hprev, mask, H):
    """h' = (1 - z) n + z (m h) with gi and ghb = m gh + b as the sums: -> (h', s)."""
    M = hprev.shape[0]
    m = _mcol(mask, M)
    hp = m * hprev.double()
    ghb = m * gh + bhh.double()
    s_ghb = m * s_gh + (m * gh).abs() + bhh.double().abs()

    def f(a, b):
        r, z, n, _ = _gates64(a, b, hp, m, H)
        return [(1 - z) * n + z * hp]
    (h, s), = _units(f, [gi, ghb], [s_gi, s_ghb], H)
    r, z, n, _ = _gates64(gi, ghb, hp, m, H)
    return h, s + (1 + z) * n.abs() + (z * hp).abs()        # (1 - z: a difference of 1 and a rounded z)


def _gru_gates_bwd_ref(gi, gh, bhh, hprev, mask, dh, s_dh, H):
    """gru_gates_bwd_kernel's outputs from gi, gh_raw (inputs: their sums are the few-term additions) and dh (with its own scale)."""
    M = hprev.shape[0]
    m = _mcol(mask, M)
    hp = m * hprev.double()
    gi, gh = gi.double(), gh.double()
    ghb = m * gh + bhh.double()
    s_ghb = (m * gh).abs() + bhh.double().abs()

    def f(a, b, g):
        r, z, n, hn = _gates64(a, b, hp, m, H)
        dan = g * (1 - z) * (1 - n * n)
        return [dan * hn * r * (1 - r), g * (hp - n) * z * (1 - z), dan, dan * r, g * z]
    res = _units(f, [gi, ghb, dh], [gi.abs(), s_ghb, s_dh], H)
    # the magnitudes of the final expressions' terms: 1 - r, 1 - z, 1 - n^2, hp - n are differences of rounded values
    r, z, n, hn = _gates64(gi, ghb, hp, m, H)
    g = dh.abs()
    mag_dan = g * (1 + z) * (1 + n * n)
    mags = [mag_dan * hn.abs() * r * (1 + r), g * (hp.abs() + n.abs()) * z * (1 + z), mag_dan, mag_dan * r, g * z]
    res = [(o, s + mg) for (o, s), mg in zip(res, mags)]
    (dar, s_r), (daz, s_z), (dan, s_n), (dnr, s_nr), (dhp, s_hp) = res
    return {"dgi": (torch.cat((dar, daz, dan), 1), torch.cat((s_r, s_z, s_n), 1)),
            "dpre": (torch.cat((dar, daz, dnr), 1), torch.cat((s_r, s_z, s_nr), 1)),
            "dhp": (dhp, s_hp), "hpm": (hp, torch.zeros_like(hp))}


def gru_reference(row, inp, state=None):
    k, M, H = row["kernel"], row["M"], row["H"]
    d = inp
    if k == "gru_gates":
        gi, gh = d["gi"].double(), d["gh"].double()
        return {"hout": _gru_fwd_ref(gi, gi.abs(), gh, torch.zeros_like(gh), d["bhh"], d["hprev"], d["mask"], H)}
    if k == "gru_step":
        gi = d["gi"].double()
        gh, s_gh = _dot_ref(d["hprev"], d["whh"])
        return {"gh_raw": (gh, s_gh), "hout": _gru_fwd_ref(gi, gi.abs(), gh, s_gh, d["bhh"], d["hprev"], d["mask"], H)}
    if k == "gru_cell":
        gi, s_gi = _dot_ref(d["x"], d["wih"])
        s_gi = s_gi + gi.abs() + d["bih"].double().abs()
        gh, s_gh = _dot_ref(d["hprev"], d["whh"])
        return {"hout": _gru_fwd_ref(gi + d["bih"].double(), s_gi, gh, s_gh, d["bhh"], d["hprev"], d["mask"], H)}
    if k == "gru_gates_bwd":
        return _gru_gates_bwd_ref(d["gi"], d["gh"], d["bhh"], d["hprev"], d["mask"], d["dh"].double(), torch.zeros(M, H).double(), H)
    if k == "gru_bwd_combine":
        m = _mcol(d["mask"], M)
        a = d["a"].double() if d["a"] is not None else torch.zeros(M, H).double()
        b, c = d["rec"].double(), d["dhp"].double()
        return {"out": (a + m * (b + c), a.abs() + (m * b).abs() + (m * c).abs())}
    # gru_bwd_rec / gru_bwd_step: out = a + m (dpre W_hh + dhp)
    m = _mcol(d["mask"], M)
    rec, s_rec = _dot_ref(d["dpre"], d["whh"].t())
    a = d["a"].double() if d["a"] is not None else torch.zeros(M, H).double()
    dhp = d["dhp"].double()
    out = a + m * (rec + dhp)
    s_out = m * s_rec + a.abs() + (m * rec).abs() + (m * dhp).abs()
    res = {"out": (out, s_out)}
    if k == "gru_bwd_step":     # the previous step's gate backward on dh = out
        ep = _gru_gates_bwd_ref(d["gi"], d["gh"], d["bhh"], d["hprev_p"], d["mask_p"], out, s_out, H)
        res.update({"dgi_p": ep["dgi"], "dpre_p": ep["dpre"], "dhp_new": ep["dhp"], "hpm_p": ep["hpm"]})
    return res


def skinny_dot(X, W, NW, drop_last_wave=False):
    """skinny_dot16 + wave_tile_sum: the K / 16 steps split over NW waves (wave w: steps [steps w / NW, steps (w + 1) / NW)), four MFMAs of
    four k each per step (MFMA j of step s: k = 16 s + 4 kq + j, kq = 0 .. 3), the waves' tiles pairwise.  X [M,K], W [R,K] float32."""
    M, K = X.shape
    steps = K // 16
    parts = []
    for w in range(NW):
        acc = np.zeros((M, W.shape[0]), dtype=F32)
        for s in range(steps * w // NW, steps * (w + 1) // NW):
            for j in range(4):
                for kq in range(4):
                    kk = 16 * s + 4 * kq + j
                    acc = acc + X[:, kk, None] * W[None, :, kk]
        parts.append(acc)
    if drop_last_wave:
        parts[-1] = np.zeros_like(parts[-1])
    while len(parts) > 1:
        parts = [parts[2 * i] + parts[2 * i + 1] for i in range(len(parts) // 2)]
    return parts[0].astype(F32)


def _sig32(x):
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x, dtype=F32))).astype(F32)


def _gates32(gi, gh, bhh, hprev, mask, H, mutant=None):
    M = hprev.shape[0]
    m = np.ones((M, 1), dtype=F32) if mask is None else _np(mask).reshape(M, 1)
    if mutant == "mask applied to gi as well":
        gi = gi * m
    r = _sig32(gi[:, :H] + (m * gh[:, :H] + bhh[:H]))
    z = _sig32(gi[:, H:2 * H] + (m * gh[:, H:2 * H] + bhh[H:2 * H]))
    hn = m * gh[:, 2 * H:] + bhh[2 * H:]
    if mutant == "b_hn added outside the r (...) product":
        n = np.tanh(gi[:, 2 * H:] + r * (m * gh[:, 2 * H:]) + bhh[2 * H:], dtype=F32)
    else:
        n = np.tanh(gi[:, 2 * H:] + r * hn, dtype=F32)
    hp = (m * hprev).astype(F32)
    return r, z, n, hn.astype(F32), hp, m


def _gates_bwd32(gi, gh, bhh, hprev, mask, g, H):
    r, z, n, hn, hp, _ = _gates32(gi, gh, bhh, hprev, mask, H)
    one = F32(1)
    dn, dz = g * (one - z), g * (hp - n)
    dan = dn * (one - n * n)
    dar, daz = dan * hn * r * (one - r), dz * z * (one - z)
    return {"dgi": np.concatenate((dar, daz, dan), 1).astype(F32), "dpre": np.concatenate((dar, daz, dan * r), 1).astype(F32),
            "dhp": (g * z).astype(F32), "hpm": hp}


GRU_MUTANTS = ("mask applied to gi as well", "b_hn added outside the r (...) product", "last wave's partial tile left out of wave_tile_sum",
               "stale dhp in the fused epilogue")


def gru_fp32(row, inp, mutant=None):
    k, M, H = row["kernel"], row["M"], row["H"]
    d = {n: (_np(v) if torch.is_tensor(v) else v) for n, v in inp.items() if n not in ("mask", "mask_p")}
    drop = mutant == GRU_MUTANTS[2]
    one = F32(1)

    def fwd(gi, gh):
        r, z, n, _, hp, _m = _gates32(gi, gh, d["bhh"], d["hprev"], inp["mask"], H, mutant)
        return ((one - z) * n + z * hp).astype(F32)
    if k == "gru_gates":
        return {"hout": fwd(d["gi"], d["gh"])}
    if k == "gru_step":
        gh = skinny_dot(d["hprev"], d["whh"], GRU_WAVES[k], drop)
        return {"gh_raw": gh, "hout": fwd(d["gi"], gh)}
    if k == "gru_cell":
        gi = skinny_dot(d["x"], d["wih"], GRU_WAVES[k], drop) + d["bih"]
        return {"hout": fwd(gi.astype(F32), skinny_dot(d["hprev"], d["whh"], GRU_WAVES[k], drop))}
    if k == "gru_gates_bwd":
        return _gates_bwd32(d["gi"], d["gh"], d["bhh"], d["hprev"], inp["mask"], d["dh"], H)
    m = np.ones((M, 1), dtype=F32) if inp["mask"] is None else _np(inp["mask"]).reshape(M, 1)
    a = d["a"] if d["a"] is not None else np.zeros((M, H), dtype=F32)
    if k == "gru_bwd_combine":
        return {"out": (a + m * (d["rec"] + d["dhp"])).astype(F32)}
    rec = skinny_dot(d["dpre"], np.ascontiguousarray(d["whh"].T), GRU_WAVES[k], drop)
    out = (a + m * (rec + d["dhp"])).astype(F32)
    res = {"out": out}
    if k == "gru_bwd_step":
        ep = _gates_bwd32(d["gi"], d["gh"], d["bhh"], d["hprev_p"], inp["mask_p"], out, H)
        res.update({"dgi_p": ep["dgi"], "dpre_p": ep["dpre"], "dhp_new": d["dhp"] if mutant == GRU_MUTANTS[3] else ep["dhp"], "hpm_p": ep["hpm"]})
    return res


# ----------------------------------------------------------------------------------------------------------------------------------
# GRUSequence end to end (functional.py GRUSequence: forward over T steps, BPTT, the batched parameter / input gradients)
# ----------------------------------------------------------------------------------------------------------------------------------
def _seq_row(T, N, I, H, ghT):
    return dict(id="gru_seq.T%d.N%d.I%d.H%d%s" % (T, N, I, H, ".ghT" if ghT else ""), family="gru_seq", T=T, N=N, I=I, H=H, ghT=ghT)


SEQ_SHAPES = [(T, N, 96, 64) for T in (1, 2, 4) for N in (1, 14, 16, 17)] + [(3, 14, 1536, 512), (2, 14, 96, 20)]
SEQ_ROWS = [_seq_row(T, N, I, H, ghT) for (T, N, I, H) in SEQ_SHAPES for ghT in (False, True)]
SEQ_MUTANTS = GRU_MUTANTS[:2] + GRU_MUTANTS[3:]


def seq_cells(row):
    rt = gru_route(row["N"], row["H"], row["T"])
    out = {("T=%d" % row["T"], "N=%d" % row["N"]) if (row["I"], row["H"]) == (96, 64) else ("T=%d N=%d I=%d H=%d" % (row["T"], row["N"], row["I"], row["H"])),
           "fused" if rt["fused"] else ("unfused by H % 16" if row["H"] % 16 else "unfused by N > 16"),
           "gradient into hT" if row["ghT"] else "no gradient into hT"}
    return out | {"backward: " + k for k in rt["backward"]}


def seq_all_cells():
    return ({("T=%d" % T, "N=%d" % N) for T in (1, 2, 4) for N in (1, 14, 16, 17)} | {"T=3 N=14 I=1536 H=512", "T=2 N=14 I=96 H=20", "fused",
            "unfused by H % 16", "unfused by N > 16", "gradient into hT", "no gradient into hT"} |
            {"backward: " + k for k in ("gru_gates_bwd", "gru_bwd_step", "gru_bwd_rec", "gru_bwd_combine")})


def seq_inputs(row):
    g = _gen(row["id"])
    T, N, I, H = (row[k] for k in ("T", "N", "I", "H"))
    rn = lambda *s: torch.randn(*s, generator=g)
    masks = (torch.rand(T * N, generator=g) > 0.3).float()
    masks[(T - 1) * N + N // 2] = 0.0                 # at least one zero row (in the last step: its recurrent gradient is cut)
    return dict(x=rn(T * N, I), h0=0.5 * rn(N, H), masks=masks, w_ih=rn(3 * H, I) / I ** 0.5, w_hh=rn(3 * H, H) / H ** 0.5, b_ih=0.1 * rn(3 * H),
                b_hh=0.1 * rn(3 * H), g_out=rn(T * N, H), g_hT=rn(N, H) if row["ghT"] else None)


def seq_reference(row, inp):
    """Forward and BPTT in float64 by the kernels' own formulas (tests/test_train_kernels_cpu.py holds them against float64 autograd), each
    output with the scale of the step that makes it: the error the earlier steps handed on is not in s -- the family's tau carries it."""
    T, N, H = row["T"], row["N"], row["H"]
    x, w_ih, w_hh = inp["x"].double(), inp["w_ih"].double(), inp["w_hh"].double()
    gi_dot, s_gi = _dot_ref(inp["x"], inp["w_ih"])
    gi = gi_dot + inp["b_ih"].double()
    s_gi = s_gi + gi_dot.abs() + inp["b_ih"].double().abs()
    h = inp["h0"].double()
    outs, s_outs, ghs, hprevs = [], [], [], []
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        gh, s_gh = h @ w_hh.t(), torch.sqrt((h * h) @ (w_hh * w_hh).t())
        hprevs.append(h)
        ghs.append(gh)
        h, s_h = _gru_fwd_ref(gi[sl], s_gi[sl], gh, s_gh, inp["b_hh"], h, inp["masks"][sl], H)
        outs.append(h)
        s_outs.append(s_h)
    res = {"out": (torch.cat(outs), torch.cat(s_outs)), "hT": (outs[-1], s_outs[-1])}
    g_out = inp["g_out"].double()
    dh = g_out[(T - 1) * N:]
    s_dh = torch.zeros_like(dh)
    if inp["g_hT"] is not None:
        s_dh = dh.abs() + inp["g_hT"].double().abs()
        dh = dh + inp["g_hT"].double()
    dgi, dpre, hpm, s_dgi, s_dpre = ([None] * T for _ in range(5))
    for t in range(T - 1, -1, -1):
        sl = slice(t * N, (t + 1) * N)
        ep = _gru_gates_bwd_ref(gi[sl], ghs[t], inp["b_hh"], hprevs[t], inp["masks"][sl], dh, s_dh, H)
        (dgi[t], s_dgi[t]), (dpre[t], s_dpre[t]), hpm[t] = ep["dgi"], ep["dpre"], ep["hpm"][0]
        m = _mcol(inp["masks"][sl], N)
        rec, s_rec = dpre[t] @ w_hh, torch.sqrt((dpre[t] ** 2) @ (w_hh * w_hh))
        a = g_out[(t - 1) * N:t * N] if t > 0 else torch.zeros_like(dh)
        dh, s_dh = a + m * (rec + ep["dhp"][0]), m * s_rec + a.abs() + (m * rec).abs() + (m * ep["dhp"][0]).abs()
    dgi, dpre, hpm = torch.cat(dgi), torch.cat(dpre), torch.cat(hpm)
    res.update({"g_h0": (dh, s_dh), "g_x": (dgi @ w_ih, torch.sqrt((dgi * dgi) @ (w_ih * w_ih))),
                "g_wih": (dgi.t() @ x, torch.sqrt((dgi * dgi).t() @ (x * x))), "g_whh": (dpre.t() @ hpm, torch.sqrt((dpre * dpre).t() @ (hpm * hpm))),
                "g_bih": (dgi.sum(0), torch.sqrt((dgi * dgi).sum(0))), "g_bhh": (dpre.sum(0), torch.sqrt((dpre * dpre).sum(0)))})
    return res


def seq_autograd64(row, inp):
    """The same quantities from float64 autograd of the plain recurrence (the check of seq_reference's formulas)."""
    T, N, H = row["T"], row["N"], row["H"]
    lv = {k: inp[k].double().requires_grad_(True) for k in ("x", "h0", "w_ih", "w_hh", "b_ih", "b_hh")}
    gi = lv["x"] @ lv["w_ih"].t() + lv["b_ih"]
    h = lv["h0"]
    outs = []
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        hm = h * inp["masks"][sl].double().view(N, 1)
        gh = hm @ lv["w_hh"].t() + lv["b_hh"]
        r, z = _sig(gi[sl, :H] + gh[:, :H]), _sig(gi[sl, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[sl, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * hm
        outs.append(h)
    out = torch.cat(outs)
    loss = (out * inp["g_out"].double()).sum() + ((h * inp["g_hT"].double()).sum() if inp["g_hT"] is not None else 0.0)
    gs = torch.autograd.grad(loss, [lv[k] for k in ("x", "h0", "w_ih", "w_hh", "b_ih", "b_hh")])
    return dict(out=out.detach(), hT=h.detach(), g_x=gs[0], g_h0=gs[1], g_wih=gs[2], g_whh=gs[3], g_bih=gs[4], g_bhh=gs[5])


def seq_fp32(row, inp, mutant=None):
    """GRUSequence in float32 by the restated kernels (the GEMMs of the unfused route and of the batched gradients as plain float32 products: the
    tiled engines' orders are tests/forward_routes.py's and tests/grad_routes.py's)."""
    T, N, H = row["T"], row["N"], row["H"]
    fused = gru_route(N, H, T)["fused"]
    d = {k: _np(v) for k, v in inp.items() if v is not None}
    gi = (d["x"] @ d["w_ih"].T + d["b_ih"]).astype(F32)
    one = F32(1)
    mk = lambda t: inp["masks"][t * N:(t + 1) * N]
    h = d["h0"]
    out, gh = [], []
    for t in range(T):
        ght = skinny_dot(h, d["w_hh"], GRU_WAVES["gru_step"]) if fused else (h @ d["w_hh"].T).astype(F32)
        r, z, n, _, hp, _m = _gates32(gi[t * N:(t + 1) * N], ght, d["b_hh"], h, mk(t), H, mutant)
        gh.append(ght)
        h = ((one - z) * n + z * hp).astype(F32)
        out.append(h)
    dh = d["g_out"][(T - 1) * N:]
    if inp["g_hT"] is not None:
        dh = (dh + d["g_hT"]).astype(F32)
    dgi, dpre, hpm = [None] * T, [None] * T, [None] * T
    whh_t = np.ascontiguousarray(d["w_hh"].T)
    stale = None
    for t in range(T - 1, -1, -1):
        hprev = out[t - 1] if t > 0 else d["h0"]
        ep = _gates_bwd32(gi[t * N:(t + 1) * N], gh[t], d["b_hh"], hprev, mk(t), dh, H)
        dgi[t], dpre[t], hpm[t] = ep["dgi"], ep["dpre"], ep["hpm"]
        dhp = ep["dhp"]
        if mutant == GRU_MUTANTS[3] and fused:
            stale = dhp if stale is None else stale       # the fused epilogue never rewrites dhp: every step reads the last step's
            dhp = stale
        m = _np(mk(t)).reshape(N, 1)
        rec = skinny_dot(dpre[t], whh_t, GRU_WAVES["gru_bwd_rec"]) if fused else (dpre[t] @ d["w_hh"]).astype(F32)
        a = d["g_out"][(t - 1) * N:t * N] if t > 0 else np.zeros((N, H), dtype=F32)
        dh = (a + m * (rec + dhp)).astype(F32)
    dgi, dpre, hpm = np.concatenate(dgi), np.concatenate(dpre), np.concatenate(hpm)
    return {"out": np.concatenate(out), "hT": out[-1], "g_h0": dh, "g_x": (dgi @ d["w_ih"]).astype(F32), "g_wih": (dgi.T @ d["x"]).astype(F32),
            "g_whh": (dpre.T @ hpm).astype(F32), "g_bih": dgi.sum(0, dtype=F32), "g_bhh": dpre.sum(0, dtype=F32)}


# ----------------------------------------------------------------------------------------------------------------------------------
# LSTM cell (rnn.hip lstm_cell_kernel / lstm_cell_bwd_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
def _lstm_row(M, H, variant):
    return dict(id="lstm.M%d.H%d.%s" % (M, H, variant), family="lstm", M=M, H=H, variant=variant)


LSTM_VARIANTS = ("both", "no dh", "no dc", "zero-mask rows", "saturated row")
LSTM_ROWS = [_lstm_row(M, H, v) for (M, H) in ((14, 64), (3, 5)) for v in LSTM_VARIANTS]
LSTM_MUTANTS = ("cell mask left out of dcprev",)


def lstm_cells(row):
    return {("M=%d" % row["M"], "H=%d" % row["H"]), row["variant"]}


def lstm_inputs(row):
    g = _gen(row["id"])
    M, H, v = row["M"], row["H"], row["variant"]
    rn = lambda *s: torch.randn(*s, generator=g)
    mask = torch.ones(M)
    if v == "zero-mask rows":
        mask[0::2] = 0.0
    d = dict(gi=rn(M, 4 * H), gh=rn(M, 4 * H), cprev=rn(M, H), mask=mask, dh=None if v == "no dh" else rn(M, H), dc=None if v == "no dc" else rn(M, H))
    if v == "saturated row":
        d["gi"][M - 1] = _sat_pattern(H, 4)
    return d


def lstm_reference(row, inp, state):
    """state: the float32 gates and c the backward was handed."""
    H = row["H"]
    gi, gh = inp["gi"].double(), inp["gh"].double()
    pre, s_pre = gi + gh, gi.abs() + gh.abs()
    m = inp["mask"].double().view(-1, 1)
    cm = inp["cprev"].double() * m
    sg = _sig(pre)
    ig, fg, og = sg[:, :H], sg[:, H:2 * H], sg[:, 3 * H:]
    gg = torch.tanh(pre[:, 2 * H:3 * H])
    gates = torch.cat((ig, fg, gg, og), 1)
    dact = torch.cat((ig * (1 - ig), fg * (1 - fg), 1 - gg * gg, og * (1 - og)), 1)
    s_gates = dact * s_pre + gates.abs()
    s_i, s_f, s_g, s_o = (s_gates[:, j * H:(j + 1) * H] for j in range(4))
    c = fg * cm + ig * gg
    s_c = cm.abs() * s_f + gg.abs() * s_i + ig * s_g + (fg * cm).abs() + (ig * gg).abs()
    tc = torch.tanh(c)
    h = og * tc
    out = {"gates": (gates, s_gates), "c": (c, s_c), "h": (h, tc.abs() * s_o + og * (1 - tc * tc) * s_c + h.abs())}
    # backward from the float32 gates / c handed to it
    G, c32 = state["gates"].double(), state["c"].double()
    ig, fg, gg, og = (G[:, j * H:(j + 1) * H] for j in range(4))
    tc = torch.tanh(c32)
    dh = inp["dh"].double() if inp["dh"] is not None else torch.zeros_like(c32)
    dc = inp["dc"].double() if inp["dc"] is not None else torch.zeros_like(c32)
    dct = dc + dh * og * (1 - tc * tc)
    s_dct = dc.abs() + (dh * og).abs() * (1 + tc * tc)
    dp = [dct * gg * ig * (1 - ig), dct * cm * fg * (1 - fg), dct * ig * (1 - gg * gg), dh * tc * og * (1 - og)]
    sp = [s_dct * (gg * ig * (1 - ig)).abs() + dp[0].abs(), s_dct * (cm * fg * (1 - fg)).abs() + dp[1].abs(),
          s_dct * (ig * (1 - gg * gg)).abs() + (dct * ig).abs() * (1 + gg * gg), dp[3].abs()]
    out.update({"dpre": (torch.cat(dp, 1), torch.cat(sp, 1)), "dcprev": (dct * fg * m, s_dct * (fg * m).abs() + (dct * fg * m).abs())})
    return out


def lstm_fp32(row, inp, mutant=None):
    H = row["H"]
    pre = (_np(inp["gi"]) + _np(inp["gh"])).astype(F32)
    m = _np(inp["mask"]).reshape(-1, 1)
    cprev = _np(inp["cprev"])
    ig, fg, og = _sig32(pre[:, :H]), _sig32(pre[:, H:2 * H]), _sig32(pre[:, 3 * H:])
    gg = np.tanh(pre[:, 2 * H:3 * H], dtype=F32)
    cm = cprev * m
    c = (fg * cm + ig * gg).astype(F32)
    tc = np.tanh(c, dtype=F32)
    one = F32(1)
    zero = np.zeros_like(c)
    dh = _np(inp["dh"]) if inp["dh"] is not None else zero
    dc = _np(inp["dc"]) if inp["dc"] is not None else zero
    dct = dc + dh * og * (one - tc * tc)
    dpre = np.concatenate((dct * gg * ig * (one - ig), dct * (cprev * m) * fg * (one - fg), dct * ig * (one - gg * gg), dh * tc * og * (one - og)), 1)
    out = {"gates": np.concatenate((ig, fg, gg, og), 1), "c": c, "h": (og * tc).astype(F32), "dpre": dpre.astype(F32),
           "dcprev": (dct * fg * (one if mutant == LSTM_MUTANTS[0] else m)).astype(F32)}
    return out, {"gates": torch.from_numpy(out["gates"]), "c": torch.from_numpy(out["c"])}


# ----------------------------------------------------------------------------------------------------------------------------------
# Policy heads (policy_heads.hip policy_heads_kernel / policy_heads_bwd_kernel / policy_heads_wgrad_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
def heads_route(H, A):
    """policy_heads_kernel's load path, the backward's dz row length, and where functional.PolicyHeads.backward takes the parameter gradients."""
    ZS = (A + 1 + 3) // 4 * 4
    return dict(load="16-byte loads" if H % 256 == 0 else "scalar loads", ZS=ZS,
                wgrad="policy_heads_wgrad" if (H % 64 == 0 and ZS in (4, 8)) else "tiled engine")


HEADS_VARIANTS = ("all", "no g_value", "no g_logp", "no g_ent", "no actions")


def _heads_rows():
    R = []
    i = 0
    for H in (64, 256, 320, 512):
        for A in (1, 3, 8):
            for M in (1, 5, 280):
                R.append(dict(id="heads.H%d.A%d.M%d" % (H, A, M), family="heads", kind="heads", H=H, A=A, M=M, variant=HEADS_VARIANTS[i % 5],
                              sat=(M == 5)))
                i += 1
    for M in (1, 63, 64, 65, 280):
        for ZS, H in ((4, 64), (8, 512), (4, 512), (8, 320)):
            R.append(dict(id="heads_wgrad.M%d.ZS%d.H%d" % (M, ZS, H), family="heads", kind="wgrad", M=M, ZS=ZS, H=H))
    return R


HEADS_ROWS = _heads_rows()
HEADS_MUTANTS = ("entropy term of dlogits dropped", "one staged 64-row round of the weight gradient skipped", "bias gradient taken from one wave only")


def heads_cells(row):
    if row["kind"] == "wgrad":
        return {("wgrad kernel", "M=%d" % row["M"], "ZS=%d" % row["ZS"])}
    rt = heads_route(row["H"], row["A"])
    out = {("H=%d" % row["H"], "A=%d" % row["A"], "M=%d" % row["M"]), rt["load"], "wgrad: " + rt["wgrad"], "variant: " + row["variant"],
           "flat-buffer views (critic row dword-aligned only)" if row["A"] % 4 else "flat-buffer views"}
    if row["sat"]:
        out.add("saturated logits")
    return out


def heads_all_cells():
    out = {("H=%d" % H, "A=%d" % A, "M=%d" % M) for H in (64, 256, 320, 512) for A in (1, 3, 8) for M in (1, 5, 280)}
    out |= {("wgrad kernel", "M=%d" % M, "ZS=%d" % ZS) for M in (1, 63, 64, 65, 280) for ZS in (4, 8)}
    out |= {"16-byte loads", "scalar loads", "wgrad: policy_heads_wgrad", "wgrad: tiled engine", "saturated logits",
            "flat-buffer views (critic row dword-aligned only)", "flat-buffer views"}
    return out | {"variant: " + v for v in HEADS_VARIANTS}


def heads_inputs(row):
    g = _gen(row["id"])
    rn = lambda *s: torch.randn(*s, generator=g)
    M, H = row["M"], row["H"]
    if row["kind"] == "wgrad":
        return dict(feats=rn(M, H), dz=rn(M, row["ZS"]))
    A = row["A"]
    d = dict(feats=rn(M, H), Wa=rn(A, H) / H ** 0.5, ba=0.1 * rn(A), Wc=rn(1, H) / H ** 0.5, bc=0.1 * rn(1),
             actions=torch.randint(0, A, (M,), generator=g), g_value=rn(M), g_logp=rn(M), g_ent=rn(M))
    if row["sat"]:      # one row of logits near +80 (action 0) and -80 (action 1, where there is one)
        u = 80.0 * d["Wa"][0] / (d["Wa"][0] ** 2).sum()
        if A > 1:
            u = u - 80.0 * d["Wa"][1] / (d["Wa"][1] ** 2).sum()
        d["feats"][M - 1] = u
    v = row["variant"]
    if v == "no actions":
        d["actions"] = None
    if v in ("no g_logp", "no actions"):
        d["g_logp"] = None
    if v == "no g_value":
        d["g_value"] = None
    if v == "no g_ent":
        d["g_ent"] = None
    return d


def _rows_prop(out, leaf, s_leaf):
    """out [M,P] whose row m depends on row m of leaf [M,Q]: s[m,p] = sum_q |d out[m,p] / d leaf[m,q]| s_leaf[m,q] (one pass per column)."""
    s = torch.zeros_like(out)
    for p in range(out.shape[1]):
        (gq,) = torch.autograd.grad(out[:, p].sum(), leaf, retain_graph=True)
        s[:, p] = (gq.abs() * s_leaf).sum(1)
    return s.detach()


def heads_reference(row, inp, state):
    """state: the float32 logp_all, probs (forward's) and dz (backward's) the later kernels were handed."""
    if row["kind"] == "wgrad":
        f, dz = inp["feats"].double(), inp["dz"].double()
        return {"dw": (dz.t() @ f, torch.sqrt((dz * dz).t() @ (f * f))), "db": (dz.sum(0), torch.sqrt((dz * dz).sum(0)))}
    M, H, A = row["M"], row["H"], row["A"]
    f, Wa, Wc = inp["feats"].double(), inp["Wa"].double(), inp["Wc"].double()
    dot, s_dot = _dot_ref(inp["feats"], inp["Wa"])
    ba = inp["ba"].double()
    logits = (dot + ba).requires_grad_(True)
    s_l = s_dot + dot.abs() + ba.abs()
    lse = torch.logsumexp(logits, 1, keepdim=True)
    lp = logits - lse
    p = torch.exp(lp)
    ent = -(lp * p).sum(1, keepdim=True)
    out = {"logp_all": (lp.detach(), _rows_prop(lp, logits, s_l) + logits.detach().abs() + lse.detach().abs()),
           "probs": (p.detach(), _rows_prop(p, logits, s_l) + p.detach()),
           "entropy": (ent.detach().view(M), (_rows_prop(ent, logits, s_l) + (lp * p).detach().abs().sum(1, keepdim=True)).view(M))}
    vdot, s_v = _dot_ref(inp["feats"], inp["Wc"])
    out["value"] = (vdot + inp["bc"].double(), s_v + vdot.abs() + inp["bc"].double().abs())
    if inp["actions"] is not None:
        idx = inp["actions"].view(M, 1)
        out["logp_act"] = (out["logp_all"][0].gather(1, idx), out["logp_all"][1].gather(1, idx))
    # backward from the float32 logp_all / probs it was handed
    LP, P = state["logp_all"].double(), state["probs"].double()
    e = -(P * LP).sum(1, keepdim=True)
    s_e = (P * LP).abs().sum(1, keepdim=True)
    zero = torch.zeros(M, 1).double()
    gl = inp["g_logp"].double().view(M, 1) if inp["g_logp"] is not None else zero
    gv = inp["g_value"].double().view(M, 1) if inp["g_value"] is not None else zero
    ge = inp["g_ent"].double().view(M, 1) if inp["g_ent"] is not None else zero
    onehot = torch.zeros(M, A).double()
    if inp["actions"] is not None:
        onehot.scatter_(1, inp["actions"].view(M, 1), 1.0)
    dl = gl * (onehot - P) + ge * (-P * (LP + e))
    s_dl = gl.abs() * (onehot + P) + ge.abs() * P * (LP.abs() + e.abs() + s_e)
    ZS = heads_route(H, A)["ZS"]
    dz = torch.zeros(M, ZS).double()
    dz[:, :A], dz[:, A:A + 1] = dl, gv
    s_dz = torch.zeros(M, ZS).double()
    s_dz[:, :A] = s_dl
    out["dz"] = (dz, s_dz)
    out["dfeats"] = (gv * Wc + dl @ Wa, torch.sqrt((gv * Wc) ** 2 + (dl * dl) @ (Wa * Wa)) + s_dl @ Wa.abs())
    # parameter gradients from the float32 dz the kernel was handed
    DZ = state["dz"].double()
    out["dw"] = (DZ.t() @ f, torch.sqrt((DZ * DZ).t() @ (f * f)))
    out["db"] = (DZ.sum(0), torch.sqrt((DZ * DZ).sum(0)))
    return out


def _heads_wgrad32(feats, dz, mutant=None):
    """policy_heads_wgrad_kernel: rounds of 64 staged rows, wave w takes rows w, w + 4, ... of a round in order, the waves (0 + 1) + (2 + 3)."""
    M, H = feats.shape
    ZS = dz.shape[1]
    acc = np.zeros((4, ZS, H), dtype=F32)
    bs = np.zeros((4, ZS), dtype=F32)
    for m0 in range(0, M, 64):
        if mutant == HEADS_MUTANTS[1] and m0 == (M - 1) // 64 * 64:
            continue                                  # the last round (the ragged one) skipped
        for r in range(min(64, M - m0)):
            w = r % 4
            acc[w] = acc[w] + dz[m0 + r][:, None] * feats[m0 + r][None, :]
            bs[w] = bs[w] + dz[m0 + r]
    db = bs[0] if mutant == HEADS_MUTANTS[2] else (bs[0] + bs[1]) + (bs[2] + bs[3])
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])).astype(F32), db.astype(F32)


def heads_fp32(row, inp, mutant=None):
    if row["kind"] == "wgrad":
        dw, db = _heads_wgrad32(_np(inp["feats"]), _np(inp["dz"]), mutant)
        return {"dw": dw, "db": db}, {}
    M, H, A = row["M"], row["H"], row["A"]
    f, Wa, Wc = _np(inp["feats"]), _np(inp["Wa"]), _np(inp["Wc"])
    W9 = np.concatenate((Wa, Wc), 0)
    if H % 256 == 0:     # lane l: k = 4 l .. 4 l + 3 (+ 256 per pass), (x0 w0 + x1 w1) + (x2 w2 + x3 w3) per load; else lane l: k = l, l + 64, ...
        pr = f[:, None, :] * W9[None, :, :]
        pr = pr.reshape(M, A + 1, H // 256, 64, 4)
        quad = (pr[..., 0] + pr[..., 1]) + (pr[..., 2] + pr[..., 3])
        lanes = np.zeros((M, A + 1, 64), dtype=F32)
        for i in range(H // 256):
            lanes = lanes + quad[:, :, i]
    else:
        pr = (f[:, None, :] * W9[None, :, :]).reshape(M, A + 1, H // 64, 64)
        lanes = np.zeros((M, A + 1, 64), dtype=F32)
        for i in range(H // 64):
            lanes = lanes + pr[:, :, i]
    acc = wave_tree(np.moveaxis(lanes, 2, 0)).astype(F32)      # [M][A+1]
    logits = (acc[:, :A] + _np(inp["ba"])).astype(F32)
    mx = logits.max(1, keepdims=True)
    se = np.zeros((M, 1), dtype=F32)
    for a in range(A):
        se = se + np.exp(logits[:, a:a + 1] - mx, dtype=F32)
    lse = mx + np.log(se, dtype=F32)
    lp = (logits - lse).astype(F32)
    p = np.exp(lp, dtype=F32)
    ent = np.zeros(M, dtype=F32)
    for a in range(A):
        ent = ent - lp[:, a] * p[:, a]
    out = {"logp_all": lp, "probs": p, "entropy": ent.astype(F32), "value": (acc[:, A:] + _np(inp["bc"])).astype(F32)}
    if inp["actions"] is not None:
        out["logp_act"] = np.take_along_axis(lp, inp["actions"].numpy().reshape(M, 1), 1)
    e = np.zeros((M, 1), dtype=F32)
    for a in range(A):
        e = e - p[:, a:a + 1] * lp[:, a:a + 1]
    zero = np.zeros((M, 1), dtype=F32)
    gl = _np(inp["g_logp"]).reshape(M, 1) if inp["g_logp"] is not None else zero
    gv = _np(inp["g_value"]).reshape(M, 1) if inp["g_value"] is not None else zero
    ge = _np(inp["g_ent"]).reshape(M, 1) if inp["g_ent"] is not None else zero
    onehot = np.zeros((M, A), dtype=F32)
    if inp["actions"] is not None:
        onehot[np.arange(M), inp["actions"].numpy()] = 1
    dl = gl * (onehot - p)
    if mutant != HEADS_MUTANTS[0]:
        dl = dl + ge * (-p * (lp + e))
    dl = dl.astype(F32)
    ZS = heads_route(H, A)["ZS"]
    dz = np.zeros((M, ZS), dtype=F32)
    dz[:, :A], dz[:, A:A + 1] = dl, gv
    df = gv * Wc
    for a in range(A):
        df = df + dl[:, a:a + 1] * Wa[a][None, :]
    out.update({"dz": dz, "dfeats": df.astype(F32)})
    if ZS in (4, 8):
        out["dw"], out["db"] = _heads_wgrad32(f, dz, mutant)
    else:                # the tiled engine's order is restated by tests/grad_routes.py: a plain float32 product here
        out["dw"], out["db"] = (dz.T @ f).astype(F32), dz.sum(0, dtype=F32)
    return out, {k: torch.from_numpy(out[k]) for k in ("logp_all", "probs", "dz")}


# ----------------------------------------------------------------------------------------------------------------------------------
# Losses (losses.hip l1_loss_kernel, l1_nhwc16_kernel, bin_l1_kernel, ppo_loss_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
PARTS = 1024      # M2H_PARTS: the block cap of l1_loss / bin_l1_loss / grad_clip_coef
LOSS_MUTANTS = ("1/n in place of 1/(2 npix)", "the tie gradient not zero")


def _loss_rows():
    R = []
    for n, off in ((1, 0), (255, 2), (257, 0), (257, 2), (1024 * 256 + 3, 2)):
        R.append(dict(id="l1.n%d.off%d" % (n, off), family="loss", kernel="l1_loss", n=n, stride=4, off=off))
    R += [dict(id="l1_nhwc16.B%d.T%d" % (B, T), family="loss", kernel="l1_loss_nhwc16", B=B, T=T, stride=2, off=1) for B, T in ((1, 1), (3, 32), (65, 1))]
    R += [dict(id="bin_l1.npix%d.cstep%d" % (n, cs), family="loss", kernel="bin_l1_loss", npix=n, cstep=cs, Cg=2 * cs) for n in (1, 257) for cs in (1, 2)]
    R += [dict(id="ppo.n%d.%s" % (n, "clipped" if c else "unclipped"), family="loss", kernel="ppo_loss", n=n, clipped=c)
          for n in (1, 280, 3000) for c in (True, False)]
    return R


LOSS_ROWS = _loss_rows()
PPO_CLIP, PPO_VCOEF, PPO_ECOEF = 0.1, 0.5, 0.02


def loss_cells(row):
    k = row["kernel"]
    if k == "l1_loss":
        return {(k, "n=%d" % row["n"]), (k, "off=%d" % row["off"]), (k, "ties"),
                (k, "grid-stride loop") if enters_grid_stride_loop(row["n"], PARTS) else (k, "one element per thread")}
    if k == "l1_loss_nhwc16":
        return {(k, "B=%d T=%d" % (row["B"], row["T"])), (k, "(b, row) loop") if row["B"] * 32 > 2048 else (k, "one (b, row) pair per block")}
    if k == "bin_l1_loss":
        return {(k, "npix=%d" % row["npix"]), (k, "cstep=%d" % row["cstep"])}
    out = {(k, "n=%d" % row["n"]), (k, "clipped value loss" if row["clipped"] else "plain value loss")}
    if row["n"] >= 8:
        out.add((k, "ratios on both clip edges"))
    return out


def loss_all_cells():
    out = {("l1_loss", "n=%d" % n) for n in (1, 255, 257, 1024 * 256 + 3)} | {("l1_loss", "off=0"), ("l1_loss", "off=2"), ("l1_loss", "ties"),
                                                                              ("l1_loss", "grid-stride loop"), ("l1_loss", "one element per thread")}
    out |= {("l1_loss_nhwc16", "B=%d T=%d" % bt) for bt in ((1, 1), (3, 32), (65, 1))} | {("l1_loss_nhwc16", "(b, row) loop"),
                                                                                          ("l1_loss_nhwc16", "one (b, row) pair per block")}
    out |= {("bin_l1_loss", "npix=1"), ("bin_l1_loss", "npix=257"), ("bin_l1_loss", "cstep=1"), ("bin_l1_loss", "cstep=2")}
    out |= {("ppo_loss", "n=%d" % n) for n in (1, 280, 3000)} | {("ppo_loss", "clipped value loss"), ("ppo_loss", "plain value loss"),
                                                                 ("ppo_loss", "ratios on both clip edges")}
    return out


def loss_inputs(row):
    g = _gen(row["id"])
    rn = lambda *s: torch.randn(*s, generator=g)
    k = row["kernel"]
    if k == "l1_loss":
        n = row["n"]
        pred, gt = rn(n), rn(n, row["stride"])
        ties = torch.arange(0, n, 7)                  # exact ties: element 0 and every 7th
        pred[ties] = gt[ties, row["off"]]
        return dict(pred=pred, gt=gt)
    if k == "l1_loss_nhwc16":
        B, T = row["B"], row["T"]
        y, gt = rn(B, 32, T, 16), rn(B, 512, T, row["stride"])
        y[:, 5, :, 3] = gt[:, 3 * 32 + 5, :, row["off"]]          # ties: pred_BHWC[b][band * 32 + r][t] = y[b][r][t][band]
        return dict(y=y, gt=gt)
    if k == "bin_l1_loss":
        n = row["npix"]
        return dict(mix=torch.rand(n, 2, generator=g) * 2.0, masks=rn(n, 2), gt=rn(n, row["Cg"]).abs())
    n = row["n"]
    clip = float(F32(PPO_CLIP))
    old_logp = -torch.rand(n, generator=g) * 2.0
    logp = old_logp + 0.15 * rn(n)
    ov = rn(n)
    v = ov + 0.15 * rn(n)
    adv = rn(n)
    if n >= 8:        # ratios on both clip edges (log of the edge: expf lands within a few ulp of it), for both signs of the advantage; value
        for i, (e, a) in enumerate(((1 + clip, 1.0), (1 + clip, -1.0), (1 - clip, 1.0), (1 - clip, -1.0))):   # differences exactly on +-clip
            logp[i] = old_logp[i] + float(np.log(e))
            adv[i] = a * (0.5 + i)
        ov[4:6] = 0.0
        v[4], v[5] = clip, -clip
    return dict(values=v, logp=logp, old_values=ov, returns=rn(n), adv=adv, old_logp=old_logp, entropy=torch.rand(n, generator=g) * 1.5)


def ppo_edge_elements(inp):
    """Elements whose float64 ratio lies within 1e-6 of a clip edge: d loss / d logp jumps there (a one-ulp difference of expf decides the side),
    so either one-sided value is the reference."""
    ratio = torch.exp(inp["logp"].double() - inp["old_logp"].double())
    clip = float(F32(PPO_CLIP))
    return ((ratio - (1 + clip)).abs() < 1e-6) | ((ratio - (1 - clip)).abs() < 1e-6)


def loss_reference(row, inp, got=None):
    """got: the implementation's outputs (used only to pick the side of ppo's gradient at the flagged clip-edge elements)."""
    k = row["kernel"]
    if k in ("l1_loss", "l1_loss_nhwc16"):
        if k == "l1_loss":
            p, gt = inp["pred"].double(), inp["gt"].double()[:, row["off"]]
        else:
            B, T = row["B"], row["T"]
            p = inp["y"].double()
            gt = inp["gt"].double()[..., row["off"]].view(B, 16, 32, T).permute(0, 2, 3, 1)     # [b][band][r][t] -> [b][r][t][band]
        d = p - gt
        n = d.numel()
        r = torch.sign(d) / n
        return {"loss": (d.abs().sum() / n, d.abs().sum() / n), "grad": (r, r.abs())}
    if k == "bin_l1_loss":
        n2 = 2 * row["npix"]
        em = torch.exp(inp["mix"].double())
        e = em - 1
        gt = inp["gt"].double()[:, ::row["cstep"]][:, :2]
        d = e * inp["masks"].double() - gt
        s_d = (em + 1) * inp["masks"].double().abs() + gt.abs()
        r = torch.sign(d) * e / n2
        return {"loss": (d.abs().sum() / n2, s_d.sum() / n2), "grad": (r, torch.where(d == 0, torch.zeros_like(d), (em + 1) / n2))}
    n = row["n"]
    clip = float(F32(PPO_CLIP))
    v, lp, ov, R, a, olp, ent = (inp[x].double() for x in ("values", "logp", "old_values", "returns", "adv", "old_logp", "entropy"))
    ratio = torch.exp(lp - olp)
    s1, s2 = ratio * a, ratio.clamp(1 - clip, 1 + clip) * a
    inside = (ratio >= 1 - clip) & (ratio <= 1 + clip)
    gl = torch.where((s1 <= s2) | inside, -a * ratio, torch.zeros_like(a)) / n
    if got is not None and "g_logp" in got:
        edge = ppo_edge_elements(inp)
        other = torch.where(gl == 0, -a * ratio / n, torch.zeros_like(a))
        gg = torch.as_tensor(got["g_logp"]).double().view(-1)
        gl = torch.where(edge & ((gg - other).abs() < (gg - gl).abs()), other, gl)
    s_gl = torch.where(gl == 0, torch.zeros_like(a), (a * ratio).abs() / n * (1 + lp.abs() + olp.abs()))
    if row["clipped"]:
        dv = v - ov
        vc = ov + dv.clamp(-clip, clip)
        l1, l2 = (v - R) ** 2, (vc - R) ** 2
        vl = torch.maximum(l1, l2)
        gv = torch.where(l1 >= l2, 2 * (v - R), torch.where((dv >= -clip) & (dv <= clip), 2 * (vc - R), torch.zeros_like(v)))
    else:
        vl, gv = (R - v) ** 2, 2 * (v - R)
    gv = 0.5 * gv / n * PPO_VCOEF
    s_gv = torch.where(gv == 0, torch.zeros_like(v), (v.abs() + R.abs() + ov.abs() + clip) * PPO_VCOEF / n)
    t = torch.minimum(s1, s2)
    o0, o1, o2 = 0.5 * vl.sum() / n, -t.sum() / n, ent.sum() / n
    # (v - R)^2 carries the rounding of its difference: 2 |v - R| (|v| + |R|) eps, inside tau of the same-sign sum
    q0, q1, q2 = 0.5 * vl.sum() / n, torch.sqrt((t * t).sum()) / n, ent.abs().sum() / n
    o3 = o0 * PPO_VCOEF + o1 - o2 * PPO_ECOEF
    q3 = q0 * PPO_VCOEF + q1 + q2 * PPO_ECOEF + (o0 * PPO_VCOEF).abs() + o1.abs() + (o2 * PPO_ECOEF).abs()
    return {"out": (torch.stack((o0, o1, o2, o3)), torch.stack((q0, q1, q2, q3))), "g_values": (gv, s_gv), "g_logp": (gl, s_gl)}


def loss_fp32(row, inp, mutant=None):
    k = row["kernel"]
    tie = mutant == LOSS_MUTANTS[1]
    if k == "l1_loss":
        n = row["n"]
        d = (_np(inp["pred"]) - _np(inp["gt"])[:, row["off"]]).astype(F32)
        inv = F32(1) / F32(n)
        grad = np.where(d > 0, inv, np.where(d < 0, -inv, inv if tie else F32(0))).astype(F32)
        return {"loss": F32(grid_sum(np.abs(d), PARTS) * inv), "grad": grad}
    if k == "l1_loss_nhwc16":
        B, T = row["B"], row["T"]
        y = _np(inp["y"])
        gt = np.transpose(_np(inp["gt"])[..., row["off"]].reshape(B, 16, 32, T), (0, 2, 3, 1))
        d = (y - gt).astype(F32)
        n = d.size
        inv = F32(1) / F32(n)
        nrows = B * 32
        blocks = min(nrows, 2048)
        tiles = np.abs(d).reshape(nrows, T * 16)             # a block's threads take elements i, i + 256, ... of each of its (b, row) tiles
        parts = np.zeros(blocks, dtype=F32)
        per = cdiv(T * 16, 256)
        for b in range(blocks):
            s = np.zeros(256, dtype=F32)
            for br in range(b, nrows, blocks):
                pad = np.zeros(per * 256, dtype=F32)
                pad[:T * 16] = tiles[br]
                for i in range(per):
                    s = s + pad[256 * i:256 * i + 256]
            parts[b] = block_sum256(s)
        grad = np.where(d > 0, inv, np.where(d < 0, -inv, inv if tie else F32(0))).astype(F32)
        return {"loss": F32(lane_strided_sum(parts, 1024) * inv), "grad": grad}
    if k == "bin_l1_loss":
        npix = row["npix"]
        e = (np.exp(_np(inp["mix"]), dtype=F32) - F32(1)).astype(F32)
        d = (e * _np(inp["masks"]) - _np(inp["gt"])[:, ::row["cstep"]][:, :2]).astype(F32)
        inv = F32(1) / F32(npix if mutant == LOSS_MUTANTS[0] else 2 * npix)
        return {"loss": F32(grid_sum(np.abs(d), PARTS) * inv), "grad": (np.sign(d).astype(F32) * inv * e).astype(F32)}
    n = row["n"]
    clip = F32(PPO_CLIP)
    v, lp, ov, R, a, olp, ent = (_np(inp[x]) for x in ("values", "logp", "old_values", "returns", "adv", "old_logp", "entropy"))
    ratio = np.exp(lp - olp, dtype=F32)
    s1 = ratio * a
    s2 = np.minimum(np.maximum(ratio, F32(1) - clip), F32(1) + clip) * a
    inside = (ratio >= F32(1) - clip) & (ratio <= F32(1) + clip)
    gl = np.where((s1 <= s2) | inside, -a * ratio, F32(0))
    if row["clipped"]:
        dv = v - ov
        vc = ov + np.minimum(np.maximum(dv, -clip), clip)
        l1, l2 = (v - R) * (v - R), (vc - R) * (vc - R)
        vl = np.where(l1 >= l2, l1, l2)
        gv = np.where(l1 >= l2, F32(2) * (v - R), np.where((dv >= -clip) & (dv <= clip), F32(2) * (vc - R), F32(0)))
    else:
        vl, gv = (R - v) * (R - v), F32(2) * (v - R)

    def one_block(t):        # thread i: elements i, i + 256, ... in order; block_sum
        k_ = cdiv(n, 256)
        pad = np.zeros(k_ * 256, dtype=F32)
        pad[:n] = t
        s = np.zeros(256, dtype=F32)
        for i in range(k_):
            s = s + pad[256 * i:256 * i + 256]
        return F32(block_sum256(s))
    fn = F32(n)
    o0, o1, o2 = F32(0.5) * one_block(vl) / fn, -one_block(np.minimum(s1, s2)) / fn, one_block(ent) / fn
    o3 = o0 * F32(PPO_VCOEF) + o1 - o2 * F32(PPO_ECOEF)
    return {"out": np.array([o0, o1, o2, o3], dtype=F32), "g_values": (F32(0.5) * gv / fn * F32(PPO_VCOEF)).astype(F32), "g_logp": (gl / fn).astype(F32)}


# ----------------------------------------------------------------------------------------------------------------------------------
# Gradient clipping + Adam (optim.hip sumsq_kernel, clip_coef_kernel, adam_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 2.5e-4, 0.9, 0.999, 1e-5
ADAM_CAP = 2048       # adam_kernel's block cap
ADAM_VARIANTS = {"clip active": dict(max_norm=0.5, gscale=1.0), "clip inactive": dict(max_norm=1e9, gscale=1.0),
                 "max_norm 0": dict(max_norm=0.0, gscale=1.0), "max_norm -1": dict(max_norm=-1.0, gscale=1.0),
                 "gscale 0.5": dict(max_norm=1e9, gscale=0.5), "clip active, gscale 0.5": dict(max_norm=0.5, gscale=0.5)}
ADAM_ROWS = [dict(id="adam.n%d.%s" % (n, v.replace(" ", "_").replace(",", "")), family="adam", n=n, variant=v, **ADAM_VARIANTS[v])
             for n in (1, 2129, 2048 * 256 + 5) for v in ADAM_VARIANTS]
ADAM_STEPS = 3
ADAM_MUTANTS = ("eps added inside the square root", "bias correction of step - 1", "the clip coefficient applied to m and not to g")


def adam_cells(row):
    n = row["n"]
    return {"n=%d" % n, row["variant"], "sumsq: grid-stride loop" if enters_grid_stride_loop(n, PARTS) else "sumsq: one element per thread",
            "adam: grid-stride loop" if enters_grid_stride_loop(n, ADAM_CAP) else "adam: one element per thread", "g = 0 and v = 0 elements"}


def adam_all_cells():
    return ({"n=%d" % n for n in (1, 2129, 2048 * 256 + 5)} | set(ADAM_VARIANTS) |
            {"sumsq: grid-stride loop", "sumsq: one element per thread", "adam: grid-stride loop", "adam: one element per thread", "g = 0 and v = 0 elements"})


def adam_inputs(row):
    """p and one gradient per step; m = v = 0 before step 1 (so v is zero wherever the first gradients are), every 5th gradient element zero in
    every step (g = 0 with v at zero throughout), every 5th + 1 zero in step 1 only."""
    g = _gen(row["id"])
    n = row["n"]
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.3 if n > 1 else 3.0) for _ in range(ADAM_STEPS)]
    for s, gr in enumerate(grads):
        gr[0::5] = 0.0
        if s == 0:
            gr[1::5] = 0.0
    if n == 1:
        grads[1][0] = 0.7
    return dict(p=p, grads=grads)


def adam_hyper(step, dtype=F32):
    """Host arithmetic of m2h_adam_step / m2h_adam_hyper: (1 - beta1^t, sqrt(1 - beta2^t)) in float32 (float64 for the reference)."""
    if dtype is F32:
        return F32(1) - np.power(F32(ADAM_B1), F32(step)), np.sqrt(F32(1) - np.power(F32(ADAM_B2), F32(step)))
    return 1.0 - float(F32(ADAM_B1)) ** step, (1.0 - float(F32(ADAM_B2)) ** step) ** 0.5


def clip_reference(row, g):
    """coef[0] = clip coefficient, coef[1] = ||g||: the sum of squares is a same-sign sum (s = itself)."""
    g = g.double()
    ss = (g * g).sum()
    norm = torch.sqrt(ss)
    s_norm = 0.5 * norm + norm              # |d sqrt / d ss| s(ss) + |norm|
    mx = float(F32(row["max_norm"]))
    if mx > 0 and float(mx / (norm + float(F32(1e-6)))) < 1.0:
        c = mx / (norm + float(F32(1e-6)))
        s_c = c * s_norm / (norm + float(F32(1e-6))) + c
    else:
        c, s_c = torch.tensor(1.0).double(), torch.tensor(0.0).double()
    return {"coef": (torch.stack((c, norm)), torch.stack((s_c, s_norm)))}


def adam_reference(row, step, p, g, m, v, coef):
    """One step in float64 from the float32 state (p, g, m, v) and the float32 clip coefficient the kernel was handed."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    b1, b2, eps, lr = (float(F32(x)) for x in (ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_LR))
    bc1, bc2s = adam_hyper(step, float)
    c = float(coef) * float(F32(row["gscale"]))
    gi = g * c
    m1 = b1 * m + (1 - b1) * gi
    s_m = (b1 * m).abs() + ((1 - b1) * gi).abs()
    v1 = b2 * v + (1 - b2) * gi * gi
    s_v = v1.clone()
    sq = torch.sqrt(v1)
    denom = sq / bc2s + eps
    upd = lr / bc1 * (m1 / denom)
    d_m = lr / bc1 / denom
    d_v = torch.where(v1 > 0, (lr / bc1 * m1 / denom ** 2).abs() / (2 * sq.clamp_min(1e-300) * bc2s), torch.zeros_like(v1))
    s_p = p.abs() + upd.abs() + d_m * s_m + d_v * s_v
    return {"p": (p - upd, s_p), "g": (gi, gi.abs()), "m": (m1, s_m), "v": (v1, s_v)}


def clip_fp32(row, g):
    g = _np(g)
    ss = grid_sum(g * g, PARTS)
    norm = np.sqrt(ss, dtype=F32)
    c = F32(1)
    if F32(row["max_norm"]) > 0:
        c = min(F32(row["max_norm"]) / (norm + F32(1e-6)), F32(1))
    return np.array([c, norm], dtype=F32)


def adam_fp32(row, step, p, g, m, v, coef, mutant=None):
    p, g, m, v = (_np(t) for t in (p, g, m, v))
    b1, b2, eps, lr = F32(ADAM_B1), F32(ADAM_B2), F32(ADAM_EPS), F32(ADAM_LR)
    with np.errstate(all="ignore"):
        bc1, bc2s = adam_hyper(step - 1 if mutant == ADAM_MUTANTS[1] else step)
        c = F32(coef) * F32(row["gscale"])
        one = F32(1)
        if mutant == ADAM_MUTANTS[2]:
            gi = g
            m1 = ((b1 * m + (one - b1) * gi) * c).astype(F32)
        else:
            gi = (g * c).astype(F32)
            m1 = (b1 * m + (one - b1) * gi).astype(F32)
        v1 = (b2 * v + (one - b2) * gi * gi).astype(F32)
        if mutant == ADAM_MUTANTS[0]:
            denom = np.sqrt(v1 / (bc2s * bc2s) + eps)
        else:
            denom = np.sqrt(v1) / bc2s + eps
        p1 = (p - (lr / bc1) * (m1 / denom)).astype(F32)
    return {"p": p1, "g": gi.astype(F32), "m": m1, "v": v1}


# ----------------------------------------------------------------------------------------------------------------------------------
# the families together
# ----------------------------------------------------------------------------------------------------------------------------------
ROWS = {"bn": BN_ROWS, "gru": GRU_ROWS, "gru_seq": SEQ_ROWS, "lstm": LSTM_ROWS, "heads": HEADS_ROWS, "loss": LOSS_ROWS, "adam": ADAM_ROWS}
ROWS_BY_ID = {r["id"]: r for rows in ROWS.values() for r in rows}
CELLS = {"bn": bn_cells, "gru": gru_cells, "gru_seq": seq_cells, "lstm": lstm_cells, "heads": heads_cells, "loss": loss_cells, "adam": adam_cells}


def all_cells(family):
    if family == "bn":
        return set(BN_CELLS)
    if family == "gru":
        return gru_all_cells()
    if family == "gru_seq":
        return seq_all_cells()
    if family == "lstm":
        return {("M=14", "H=64"), ("M=3", "H=5")} | set(LSTM_VARIANTS)
    if family == "heads":
        return heads_all_cells()
    if family == "loss":
        return loss_all_cells()
    return adam_all_cells()


# mutant -> (family, predicate on the row: the rows the bound must reject the mutant on)
MUTANT_ROWS = {
    BN_MUTANTS[0]: ("bn", lambda r: r["M"] >= 33),                           # (two rows of a large-mean channel can lie closer than sqrt(eps))
    BN_MUTANTS[1]: ("bn", lambda r: True),
    BN_MUTANTS[2]: ("bn", lambda r: r["M"] <= 257),
    BN_MUTANTS[3]: ("bn", lambda r: True),
    GRU_MUTANTS[0]: ("gru", lambda r: r["kernel"] in ("gru_gates", "gru_step", "gru_cell") and r["mask"] == "mixed"),
    GRU_MUTANTS[1]: ("gru", lambda r: r["kernel"] in ("gru_gates", "gru_step", "gru_cell") and not r["sat"]),
    GRU_MUTANTS[2]: ("gru", lambda r: r["kernel"] in GRU_WAVES and not r["sat"] and                # (a zero mask on the only row hides the product)
                     not (r["kernel"] in ("gru_bwd_rec", "gru_bwd_step") and r["M"] == 1 and r["mask"] == "mixed")),
    GRU_MUTANTS[3]: ("gru", lambda r: r["kernel"] == "gru_bwd_step"),
    ("seq", GRU_MUTANTS[0]): ("gru_seq", lambda r: True),                    # (every sequence row has a zero mask row)
    ("seq", GRU_MUTANTS[1]): ("gru_seq", lambda r: True),
    ("seq", GRU_MUTANTS[3]): ("gru_seq", lambda r: gru_route(r["N"], r["H"], r["T"])["fused"] and r["T"] >= 2 and r["N"] > 1),
    LSTM_MUTANTS[0]: ("lstm", lambda r: r["variant"] == "zero-mask rows"),
    HEADS_MUTANTS[0]: ("heads", lambda r: r["kind"] == "heads" and r["A"] > 1 and r["variant"] != "no g_ent"),
    HEADS_MUTANTS[1]: ("heads", lambda r: (r["kind"] == "wgrad" or heads_route(r["H"], r["A"])["ZS"] in (4, 8)) and r["M"] > 1 and
                       (r["kind"] == "wgrad" or r["variant"] != "no g_value" or r["A"] > 1)),
    HEADS_MUTANTS[2]: ("heads", lambda r: (r["kind"] == "wgrad" or heads_route(r["H"], r["A"])["ZS"] in (4, 8)) and r["M"] > 1 and
                       (r["kind"] == "wgrad" or r["variant"] != "no g_value" or r["A"] > 1)),
    LOSS_MUTANTS[0]: ("loss", lambda r: r["kernel"] == "bin_l1_loss"),
    LOSS_MUTANTS[1]: ("loss", lambda r: r["kernel"] in ("l1_loss", "l1_loss_nhwc16")),
    ADAM_MUTANTS[0]: ("adam", lambda r: r["n"] > 1),                         # (shows where sqrt(v) is of eps's size: the zero-gradient elements)
    ADAM_MUTANTS[1]: ("adam", lambda r: True),
    ADAM_MUTANTS[2]: ("adam", lambda r: r["variant"] in ("clip active", "gscale 0.5", "clip active, gscale 0.5")),
}
