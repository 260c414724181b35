"""The rollout kernels (TEST INFRASTRUCTURE): csrc/advantage.hip, the reward / distance kernels of csrc/losses.hip (sq_stats,
rewards_from_stats, stft_l2), csrc/rollout_fused.hip, csrc/acoustic_mem.hip and csrc/rollout_ops.hip -- the table of test rows per family,
the cells the rows must reach, seeded inputs, the float64 reference of every output with its element-wise error scale, float32 numpy
restatements of each kernel's algorithm in the kernel's own summation order, and named mutants of those restatements.

tests/test_gpu_rollout_kernels.py runs every row through the public m2h.ops function against ``reference``;
tests/test_rollout_kernels_cpu.py checks without a GPU that the rows reach every cell, that every restatement stays inside the family's
tau on every row, that every mutant leaves it on the rows named for it (by a margin of at least MIN_MARGIN), and that the restated launch
geometry is the sources'.

The scale rule is the one of tests/train_kernels.py, unchanged: a mixed-sign sum sqrt(sum t^2); a same-sign sum sum |t|; a function of
sums sum |df/dsigma| s(sigma) plus the magnitudes of the final expression's terms.  Checks are LOCAL: a kernel handed another kernel's
float32 output (adv_apply its gmean / gvar, the variance its own float32 mean, the episode statistics the kernel's own float32 reward and
losses) is referenced from those float32 values.  An output that must be exact has s = 0.  No element is left out.

The least-squares scale of elem_bound.bound is asked for where it can say more than the element bound does (LSQ_COND): on an output
whose scales exceed its values many times over -- a reward that is a difference of near-equal ratios, a return of cancelling terms --
<g, r> / <r, r> - 1 is bounded by tau <s, |r|> / <r, r> and no better, so there the element bound stands alone.

Mutant margins on this table (worst |g - r| / (tau s) over a mutant's named rows, the smallest over those rows; inf = an exact output
differs or a value is not finite; printed by tests/test_rollout_kernels_cpu.py::test_mutant_margins):
  gae         mask of step s 9.0e+03, tau dropped 2.6e+03, value_preds[T] kept inf
  adv         biased variance in mode 1 3.9e+01, one-pass variance 2.9e+01, eps inside the square root 1.1e+03, tail dropped 6.2e+01
  reward      L for 2L 8.2e+03, not_done ignored inf, quality term added 2.5e+04, tail past the last 4096 dropped 7.4e+00 (one element of
              4097), ground truth at gt_off + 1 4.6e+02
  step_stats  last slice dropped 5.6e+02, right channel at offset 1 1.1e+01 (the bin loss's scale carries 2 |d| s(d) of the exp / mask
              product), no 2L division 5.0e+04
  mem         hidden rows outside hold conv outputs 6.2e+03, halo columns (the four of them) 5.0e+03 at the least, not_done on
              pred_mono 1.7e+04, de-slice rows swapped 2.7e+04
  glue        op 1 without the clamp inf, slice rows swapped inf, bscale on a inf, multiplication by 1/255 inf
"""
import itertools

import numpy as np
import torch

import train_kernels as K
from elem_bound import TAU_FP32
from train_kernels import FLUSH, F32, _gen, block_sum256, cdiv, enters_grid_stride_loop, grid_for, seed_of, wave_tree  # noqa: F401

FAMILIES = ("gae", "adv", "reward", "step_stats", "mem", "glue", "copy")
# Every family is single kernels: TAU_FP32.  (A wider bound would need a float32 restatement above TAU_FP32 on some row; none is: the
# worst restatement ratio is the mean of the advantages at n = 4097, offset 100 -- the rounding of a mean near 100 against
# sqrt(sum s(a)^2) / n, as for BatchNorm's mean in tests/train_kernels.py -- and the CPU test holds it to TAU_FP32 / 2.)
TAU = {f: TAU_FP32 for f in FAMILIES}
MIN_MARGIN = 4.0
LSQ_COND = 4.0
# launch geometry restated (tests/test_rollout_kernels_cpu.py holds it against the sources)
GAE_BLOCK, ADV_BLOCK, REWARD_BLOCK, REWARD_UNROLL, REWARDS_BLOCK = 64, 256, 1024, 4, 64
STEP_STATS_CHUNKS, STEP_STATS_BLOCK = 16, 256
ROWS_COPY_MAX, ROWS_COPY_GX, OBSERVE_GX, GATHER_CAP, GLUE_CAP = 32, 256, 64, 8192, 4096
MEM_R = 2


def check(g, r, s, tau):
    """(worst |g - r| / s, least-squares scale, holds): train_kernels.check's element bound; its scale condition where the output is
    well conditioned (module docstring)."""
    g, r, s = (torch.as_tensor(np.asarray(t)).double().reshape(-1) for t in (g, r, s))
    worst, scale, _ = K.check(g, r, s, tau)
    rr = float((r * r).sum())
    cond = float((s * r.abs()).sum()) / rr if rr > 0 else float("inf")
    return worst, scale, worst <= tau and (cond > LSQ_COND or abs(scale - 1.0) <= tau)


def _f(t):
    return t.detach().cpu().numpy().astype(F32) if torch.is_tensor(t) else np.asarray(t, dtype=F32)


def _d(t):
    return _f(t).astype(np.float64)


def _z(a):
    return np.zeros_like(np.asarray(a, dtype=np.float64))


def thread_strided_sum(terms, threads=256):
    """Thread i of one block takes elements i, i + threads, ... in order -> the per-thread float32 sums."""
    terms = np.asarray(terms, dtype=F32).reshape(-1)
    k = max(1, cdiv(terms.size, threads))
    pad = np.zeros(k * threads, dtype=F32)
    pad[:terms.size] = terms
    s = np.zeros(threads, dtype=F32)
    for i in range(k):
        s = s + pad[i * threads:(i + 1) * threads]
    return s


def block_sum_of(terms):
    """advantage.hip's single-block reductions: the strided thread sums, then rl_common.h block_sum."""
    return F32(block_sum256(thread_strided_sum(terms)))


# ----------------------------------------------------------------------------------------------------------------------------------
# gae (advantage.hip gae_returns_kernel: one thread per env, blocks of 64, T steps backwards)
# ----------------------------------------------------------------------------------------------------------------------------------
GAE_T, GAE_N = (1, 2, 9), (1, 63, 64, 65)
GAE_GT = {"g0.99t0.95": (0.99, 0.95), "g1t1": (1.0, 1.0), "g0.99t0": (0.99, 0.0)}
GAE_MASKS = ("ones", "random", "ends", "zeros")
GAE_SENTINEL = -7.25
GAE_MUTANTS = ("the mask of step s in place of s + 1", "tau dropped from the recursion", "value_preds[T] not replaced by next_value")


def _gae_rows():
    R = []
    for (iT, T), (iN, N), gae, (ig, gt), (im, mask) in itertools.product(enumerate(GAE_T), enumerate(GAE_N), (1, 0), enumerate(GAE_GT),
                                                                          enumerate(GAE_MASKS)):
        if (iT + iN + ig + im) % 2 == 0:        # half of the cross: every (T, N, mode) with every mask and every (gamma, tau)
            R.append(dict(id="gae.T%d.N%d.%s.%s.%s" % (T, N, "gae" if gae else "disc", gt, mask), family="gae", T=T, N=N, gae=gae, gt=gt, mask=mask))
    return R


GAE_ROWS = _gae_rows()


def gae_cells(row):
    mode = "gae" if row["gae"] else "discounted"
    out = {("T=%d" % row["T"], "N=%d" % row["N"], mode), (mode, row["gt"]), (mode, "mask " + row["mask"]),
           "one block" if row["N"] <= GAE_BLOCK else "second block (N > 64)"}
    out.add("returns[T] keeps its sentinel" if row["gae"] else "value_preds untouched, returns[T] = next_value")
    return out


def gae_all_cells():
    out = {("T=%d" % T, "N=%d" % N, m) for T in GAE_T for N in GAE_N for m in ("gae", "discounted")}
    out |= {(m, gt) for m in ("gae", "discounted") for gt in GAE_GT} | {(m, "mask " + k) for m in ("gae", "discounted") for k in GAE_MASKS}
    return out | {"one block", "second block (N > 64)", "returns[T] keeps its sentinel", "value_preds untouched, returns[T] = next_value"}


def gae_inputs(row):
    g = _gen(row["id"])
    T, N = row["T"], row["N"]
    rn = lambda *s: torch.randn(*s, generator=g)
    if row["mask"] == "ones":
        m = torch.ones(T + 1, N, 1)
    elif row["mask"] == "zeros":
        m = torch.zeros(T + 1, N, 1)
    elif row["mask"] == "random":
        m = (torch.rand(T + 1, N, 1, generator=g) > 0.3).float()
    else:                                       # a zero at step 1 and at step T on every second env, ones elsewhere
        m = torch.ones(T + 1, N, 1)
        m[1, ::2] = 0.0
        m[T, ::2] = 0.0
    return dict(rewards=rn(T, N, 1), value_preds=rn(T + 1, N, 1), masks=m, next_value=rn(N, 1), returns=torch.full((T + 1, N, 1), GAE_SENTINEL))


def gae_reference(row, inp):
    T, N = row["T"], row["N"]
    gamma, tau = (float(F32(x)) for x in GAE_GT[row["gt"]])
    r, v, m, nv = _d(inp["rewards"]).reshape(T, N), _d(inp["value_preds"]).reshape(T + 1, N), _d(inp["masks"]).reshape(T + 1, N), _d(inp["next_value"]).reshape(N)
    ret, sc = np.full((T + 1, N), GAE_SENTINEL), np.zeros((T + 1, N))
    if row["gae"]:
        v = v.copy()
        v[T] = nv
        gae, q = np.zeros(N), np.zeros(N)
        for s in range(T - 1, -1, -1):
            mm = m[s + 1]
            gae = r[s] + gamma * v[s + 1] * mm - v[s] + gamma * tau * mm * gae
            q = r[s] ** 2 + (gamma * v[s + 1] * mm) ** 2 + v[s] ** 2 + (gamma * tau * mm) ** 2 * q
            ret[s], sc[s] = gae + v[s], np.sqrt(q + v[s] ** 2)
    else:
        ret[T] = nv
        q = nv ** 2
        for s in range(T - 1, -1, -1):
            ret[s] = ret[s + 1] * gamma * m[s + 1] + r[s]
            q = r[s] ** 2 + (gamma * m[s + 1]) ** 2 * q
            sc[s] = np.sqrt(q)
    return {"returns": (ret, sc), "value_preds": (v, _z(v))}


def gae_fp32(row, inp, mutant=None):
    T, N = row["T"], row["N"]
    gamma, tau = (F32(x) for x in GAE_GT[row["gt"]])
    r, v, m, nv = _f(inp["rewards"]).reshape(T, N), _f(inp["value_preds"]).reshape(T + 1, N).copy(), _f(inp["masks"]).reshape(T + 1, N), _f(inp["next_value"]).reshape(N)
    ret = _f(inp["returns"]).reshape(T + 1, N).copy()
    mk = (lambda s: m[s]) if mutant == GAE_MUTANTS[0] else (lambda s: m[s + 1])
    if row["gae"]:
        if mutant != GAE_MUTANTS[2]:
            v[T] = nv
        gae = np.zeros(N, dtype=F32)
        for s in range(T - 1, -1, -1):
            delta = r[s] + gamma * v[s + 1] * mk(s) - v[s]
            gae = delta + (gamma if mutant == GAE_MUTANTS[1] else gamma * tau) * mk(s) * gae
            ret[s] = gae + v[s]
    else:
        ret[T] = nv
        for s in range(T - 1, -1, -1):
            ret[s] = ret[s + 1] * gamma * mk(s) + r[s]
    return {"returns": ret.astype(F32), "value_preds": v}


# ----------------------------------------------------------------------------------------------------------------------------------
# adv (advantage.hip advantages_kernel modes 0 / 1 / 2, adv_sqdiff_kernel, adv_apply_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
ADV_N = (2, 255, 256, 257, 4097)
ADV_DISTS = {"std": (0.0, 1.0), "off100s1": (100.0, 1.0), "off100s0.01": (100.0, 0.01)}
ADV_EPS = 1e-5
ADV_ROWS = [dict(id="adv.n%d.%s" % (n, d), family="adv", n=n, dist=d) for n in ADV_N for d in ADV_DISTS]
ADV_MUTANTS = ("biased variance in mode 1", "one-pass variance E[a^2] - mean^2", "eps inside the square root", "the tail i >= 256 floor(n / 256) dropped")


def adv_cells(row):
    n = row["n"]
    return {"n=%d" % n, row["dist"], ("n=%d" % n, row["dist"]), "one element per thread at the most" if n <= ADV_BLOCK else "a thread takes a second element",
            "ragged last stride" if n % ADV_BLOCK else "whole strides", "adv_apply: one block" if n <= 256 else "adv_apply: more blocks"}


def adv_all_cells():
    return ({"n=%d" % n for n in ADV_N} | set(ADV_DISTS) | {("n=%d" % n, d) for n in ADV_N for d in ADV_DISTS} |
            {"one element per thread at the most", "a thread takes a second element", "ragged last stride", "whole strides", "adv_apply: one block",
             "adv_apply: more blocks"})


def adv_inputs(row):
    """Two shards of n advantages (rank a is the row's own call, rank b the other member of the simulated world of 2): value_preds and
    returns [n + 1, 1, 1] with returns[:n] = fl(value + advantage)."""
    g = _gen(row["id"])
    n = row["n"]
    off, spread = ADV_DISTS[row["dist"]]
    out = {}
    for k in ("a", "b"):
        val = torch.randn(n + 1, 1, 1, generator=g)
        ret = torch.randn(n + 1, 1, 1, generator=g)
        ret[:n] = val[:n] + (off + spread * torch.randn(n, 1, 1, generator=g))
        out["val_" + k], out["ret_" + k] = val, ret
    return out


def adv_combine(x, y):
    """The host step of the distributed recipe at world size 2: the float64 average of two float32 values, rounded to float32."""
    return F32((float(x) + float(y)) / 2.0)


def adv_reference(row, inp, state):
    """state: the implementation's own float32 stats (mean, mean1 -- the mode-1 call's --, mean_b, sqdiff_a, sqdiff_b): the variance is
    about the mean it was handed, gmean / gvar come from the handed means / squared differences."""
    n, eps = row["n"], float(F32(ADV_EPS))
    ret, val = _d(inp["ret_a"]).reshape(-1)[:n], _d(inp["val_a"]).reshape(-1)[:n]
    a = (_f(inp["ret_a"]).reshape(-1)[:n] - _f(inp["val_a"]).reshape(-1)[:n]).astype(np.float64)       # the float32 difference: exact by row "adv0"
    out = {"adv0": (a, _z(a)), "adv2": (a, _z(a)), "mean": ((ret - val).sum() / n, np.sqrt((ret ** 2 + val ** 2).sum()) / n)}

    def var_about(x, m):
        v = ((x - m) ** 2).sum() / x.size
        return v, v
    out["var"] = var_about(a, float(state["mean"]))
    m1 = float(state["mean1"])
    ss = ((a - m1) ** 2).sum()
    sd = np.sqrt(ss / (n - 1))
    o = (a - m1) / (sd + eps)
    out["adv1"] = (o, np.abs(o) * (sd / (2 * (sd + eps)) + 2.0))
    ab = (_f(inp["ret_b"]).reshape(-1)[:n] - _f(inp["val_b"]).reshape(-1)[:n]).astype(np.float64)
    retb, valb = _d(inp["ret_b"]).reshape(-1)[:n], _d(inp["val_b"]).reshape(-1)[:n]
    out["mean_b"] = ((retb - valb).sum() / n, np.sqrt((retb ** 2 + valb ** 2).sum()) / n)
    gm = float(adv_combine(state["mean"], state["mean_b"]))
    out["sqdiff_a"], out["sqdiff_b"] = var_about(a, gm), var_about(ab, gm)
    gv = float(adv_combine(state["sqdiff_a"], state["sqdiff_b"]))
    for k, x in (("a", a), ("b", ab)):
        o = (x - gm) / (np.sqrt(gv) + eps)
        out["apply_" + k] = (o, 2.0 * np.abs(o))
    return out


def adv_fp32(row, inp, mutant=None):
    n, eps = row["n"], F32(ADV_EPS)
    keep = (n // 256) * 256 if mutant == ADV_MUTANTS[3] else n
    fn = F32(n)

    def stats(a):
        mean = F32(block_sum_of(a[:keep]) / fn)
        if mutant == ADV_MUTANTS[1]:
            ss = F32(max(block_sum_of((a * a)[:keep]) - fn * mean * mean, F32(0)))
        else:
            d = a - mean
            ss = block_sum_of((d * d)[:keep])
        return mean, ss
    a = (_f(inp["ret_a"]).reshape(-1)[:n] - _f(inp["val_a"]).reshape(-1)[:n]).astype(F32)
    ab = (_f(inp["ret_b"]).reshape(-1)[:n] - _f(inp["val_b"]).reshape(-1)[:n]).astype(F32)
    mean, ss = stats(a)
    with np.errstate(all="ignore"):
        if mutant == ADV_MUTANTS[2]:
            den = np.sqrt(ss / F32(n - 1) + eps, dtype=F32)
        else:
            den = np.sqrt(ss / F32(n if mutant == ADV_MUTANTS[0] else n - 1), dtype=F32) + eps
        out = {"adv0": a, "adv2": a, "mean": mean, "mean1": mean, "var": F32(ss / fn), "adv1": ((a - mean) / den).astype(F32)}
        out["mean_b"] = stats(ab)[0]
        gm = adv_combine(out["mean"], out["mean_b"])
        for k, x in (("a", a), ("b", ab)):
            d = x - gm
            out["sqdiff_" + k] = F32(block_sum_of((d * d)[:keep]) / fn)
        gv = adv_combine(out["sqdiff_a"], out["sqdiff_b"])
        den = np.sqrt(gv + eps, dtype=F32) if mutant == ADV_MUTANTS[2] else np.sqrt(gv, dtype=F32) + eps
        for k, x in (("a", a), ("b", ab)):
            out["apply_" + k] = ((x - gm) / den).astype(F32)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# reward (losses.hip sq_stats_kernel, stft_l2_kernel: 1024 threads, four loads in flight, stride 4096; rewards_from_stats_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
REWARD_L = (1, 1023, 1024, 1025, 4096, 4097, 16384)
REWARD_MUTANTS = ("L in place of 2L", "not_done ignored", "the quality term added instead of subtracted", "elements past the last full 4096 dropped",
                  "the ground truth read at gt_off + 1")


def _reward_rows():
    R = [dict(id="sq_stats.L%d.N%d.off%d" % (L, N, off), family="reward", kernel="sq_stats", L=L, N=N, off=off) for L in REWARD_L for N in (1, 3) for off in (0, 2)]
    R += [dict(id="stft_l2.L%d.%s" % (L, "bin" if mix else "mono"), family="reward", kernel="stft_l2", L=L, N=2, mix=mix, nch=2 if mix else 1,
               Cp=2 if mix else 1, Cg=8 if mix else 4) for L in REWARD_L for mix in (False, True)]
    for N in (1, 64, 65):
        for q, mult in ((True, 10.0), (False, 10.0), (False, 20.0)):
            R.append(dict(id="rewards.N%d.%s.mult%d" % (N, "quality" if q else "plain", mult), family="reward", kernel="rewards_from_stats", N=N,
                          quality=q, mult=mult, near=False))
    R.append(dict(id="rewards.N65.quality.near_equal", family="reward", kernel="rewards_from_stats", N=65, quality=True, mult=10.0, near=True))
    return R


REWARD_ROWS = _reward_rows()
REWARDS_L = 512 * 32


def reward_cells(row):
    k = row["kernel"]
    if k == "rewards_from_stats":
        out = {(k, "N=%d" % row["N"]), (k, "quality improvement" if row["quality"] else "plain, mult %d" % row["mult"]),
               (k, "one block") if row["N"] <= REWARDS_BLOCK else (k, "second block")}
        if row["N"] > 1:
            out.add((k, "finished envs"))
        if row["near"]:
            out.add((k, "difference of near-equal ratios"))
        return out
    L = row["L"]
    out = {(k, "L=%d" % L), (k, "L below the block") if L < REWARD_BLOCK else (k, "a ragged stride") if L % 4096 else (k, "whole strides"),
           (k, "second stride") if L > 4096 else (k, "one stride")}
    out |= {(k, "N=%d" % row["N"]), (k, "gt_off=%d" % row["off"])} if k == "sq_stats" else {(k, "with mix, nch=2" if row["mix"] else "without mix, nch=1")}
    return out


def reward_all_cells():
    out = set()
    for k in ("sq_stats", "stft_l2"):
        out |= {(k, "L=%d" % L) for L in REWARD_L} | {(k, "L below the block"), (k, "a ragged stride"), (k, "whole strides"), (k, "second stride"), (k, "one stride")}
    out |= {("sq_stats", "N=1"), ("sq_stats", "N=3"), ("sq_stats", "gt_off=0"), ("sq_stats", "gt_off=2"), ("stft_l2", "with mix, nch=2"), ("stft_l2", "without mix, nch=1")}
    k = "rewards_from_stats"
    return out | {(k, "N=%d" % N) for N in (1, 64, 65)} | {(k, "quality improvement"), (k, "plain, mult 10"), (k, "plain, mult 20"), (k, "one block"),
                                                          (k, "second block"), (k, "finished envs"), (k, "difference of near-equal ratios")}


def reward_inputs(row):
    g = _gen(row["id"])
    k = row["kernel"]
    if k == "sq_stats":
        N, L = row["N"], row["L"]
        pred, gt = torch.rand(N, L, 1, 1, generator=g), torch.rand(N, L, 1, 4, generator=g) + 0.05
        pred[:, L - 1], gt[:, L - 1] = 3.0, torch.tensor([0.5, 1.5, 1.0, 2.0])      # the last element carries weight: a dropped tail shows
        return dict(pred=pred, gt=gt)
    if k == "stft_l2":
        N, L, Cp, Cg = row["N"], row["L"], row["Cp"], row["Cg"]
        pred = torch.randn(N, L, 1, Cp, generator=g) if row["mix"] else torch.rand(N, L, 1, Cp, generator=g)
        gt = torch.rand(N, L, 1, Cg, generator=g)
        gt[:, L - 1] = 3.0
        return dict(pred=pred, gt=gt, mix=torch.rand(N, L, 1, Cp, generator=g) * 1.5 if row["mix"] else None)
    N = row["N"]
    nxt = torch.stack((torch.rand(N, generator=g) * 0.9 + 0.1, torch.rand(N, generator=g) * 1.5 + 0.5), 1) * REWARDS_L
    cur = torch.stack((torch.rand(N, generator=g) * 0.9 + 0.1, torch.rand(N, generator=g) * 1.5 + 0.5), 1) * REWARDS_L
    if row["near"]:                             # the memory hardly moved: the two ratios agree to about 1e-6
        cur = nxt * (1.0 + 1e-6 * torch.randn(N, 2, generator=g))
    nd = (torch.rand(N, 1, generator=g) > 0.3).float()
    if N > 1:
        nd[0], nd[N - 1] = 1.0, 0.0
    else:
        nd[0] = 1.0
    return dict(next_stats=nxt, cur_stats=cur, not_done=nd)


def _stft_terms64(pred, gt, mix, ch):
    """(d^2, its scale) per element of channel ch: d = g - p, p = (exp(mix) - 1) mask or the tensor itself."""
    g = gt[..., 2 * ch]
    if mix is None:
        d = g - pred[..., ch]
        return d * d, d * d
    em = np.exp(mix[..., ch])
    d = g - (em - 1) * pred[..., ch]
    s_d = np.abs(g) + (em + 1) * np.abs(pred[..., ch])
    return d * d, d * d + 2 * np.abs(d) * s_d


def _rewards64(nxt, cur, nd, quality, mult, s_ratio):
    """r and s from the four sums; s_ratio: the scale of one ratio in units of itself (1: the sums are exact inputs; 3: they are same-sign
    sums the kernel made itself -- d/dn0 and d/dn1 give the ratio each, the quotient's own rounding once more)."""
    rn, rc = nxt[:, 0] / nxt[:, 1], cur[:, 0] / cur[:, 1]
    if quality:
        r, s = -rn + rc, s_ratio * (rn + rc) + (rn + rc)
    else:
        r, s = -rn * mult, (s_ratio + 1) * rn * mult
    live = nd.reshape(-1) != 0
    return np.where(live, r, 0.0), np.where(live, s, 0.0)


def reward_reference(row, inp):
    k = row["kernel"]
    if k == "sq_stats":
        p, g = _d(inp["pred"]).reshape(row["N"], -1), _d(inp["gt"]).reshape(row["N"], -1, 4)[..., row["off"]]
        st = np.stack((((p - g) ** 2).sum(1), (g * g).sum(1)), 1)
        return {"stats": (st, st)}
    if k == "stft_l2":
        N, L = row["N"], row["L"]
        pred, gt = _d(inp["pred"]).reshape(N, L, -1), _d(inp["gt"]).reshape(N, L, -1)
        mix = _d(inp["mix"]).reshape(N, L, -1) if row["mix"] else None
        r, s = np.zeros(N), np.zeros(N)
        for ch in range(row["nch"]):
            t, st = _stft_terms64(pred, gt, mix, ch)
            r, s = r + t.sum(1) / (2 * L), s + st.sum(1) / (2 * L)
        return {"out": (r, s + (r if row["nch"] > 1 else 0.0))}
    r, s = _rewards64(_d(inp["next_stats"]), _d(inp["cur_stats"]), _d(inp["not_done"]), row["quality"], float(F32(row["mult"])), 1.0)
    return {"rewards": (r, s)}


def sum1024x4(terms, drop_tail=False):
    """sq_stats / stft_l2: thread t takes i0 = t, t + 4096, ... and of each the four elements i0 + 1024 u into four accumulators,
    (s0 + s1) + (s2 + s3), the wave trees, then losses.hip block_sum16's sixteen waves in order."""
    terms = np.asarray(terms, dtype=F32).reshape(-1)
    if drop_tail:
        terms = terms[:(terms.size // 4096) * 4096]
    it = max(1, cdiv(terms.size, 4096))
    pad = np.zeros(it * 4096, dtype=F32)
    pad[:terms.size] = terms
    pad = pad.reshape(it, REWARD_UNROLL, REWARD_BLOCK)
    acc = np.zeros((REWARD_UNROLL, REWARD_BLOCK), dtype=F32)
    for i in range(it):
        acc = acc + pad[i]
    t = (acc[0] + acc[1]) + (acc[2] + acc[3])
    tot = F32(0)
    for w in range(16):
        tot = F32(tot + wave_tree(t[64 * w:64 * w + 64]))
    return tot


def _rewards32(nxt, cur, nd, quality, mult, L, mutant=None):
    Lf = F32(L)
    with np.errstate(all="ignore"):
        r = -(nxt[:, 0] / Lf) / (nxt[:, 1] / Lf)
        if quality:
            q = -(cur[:, 0] / Lf) / (cur[:, 1] / Lf)
            r = r + q if mutant == REWARD_MUTANTS[2] else r - q
        else:
            r = r * F32(mult)
    return r.astype(F32) if mutant == REWARD_MUTANTS[1] else np.where(nd.reshape(-1) != 0, r, F32(0)).astype(F32)


def _stft32(pred, gt, mix, nch, L, mutant=None):
    tot = np.zeros(pred.shape[0], dtype=F32)
    for ch in range(nch):
        p = pred[..., ch] if mix is None else ((np.exp(mix[..., ch], dtype=F32) - F32(1)) * pred[..., ch]).astype(F32)
        d = gt[..., 2 * ch] - p
        part = np.array([sum1024x4(x, mutant == REWARD_MUTANTS[3]) for x in (d * d).astype(F32)], dtype=F32)
        tot = tot + part / F32(L if mutant == REWARD_MUTANTS[0] else 2 * L)
    return tot.astype(F32)


def reward_fp32(row, inp, mutant=None):
    k = row["kernel"]
    if k == "sq_stats":
        N = row["N"]
        p, g = _f(inp["pred"]).reshape(N, -1), _f(inp["gt"]).reshape(N, -1, 4)[..., row["off"] + (1 if mutant == REWARD_MUTANTS[4] else 0)]
        d = p - g
        drop = mutant == REWARD_MUTANTS[3]
        return {"stats": np.array([[sum1024x4(d[e] * d[e], drop), sum1024x4(g[e] * g[e], drop)] for e in range(N)], dtype=F32)}
    if k == "stft_l2":
        N, L = row["N"], row["L"]
        return {"out": _stft32(_f(inp["pred"]).reshape(N, L, -1), _f(inp["gt"]).reshape(N, L, -1), _f(inp["mix"]).reshape(N, L, -1) if row["mix"] else None,
                               row["nch"], L, mutant)}
    return {"rewards": _rewards32(_f(inp["next_stats"]), _f(inp["cur_stats"]), _f(inp["not_done"]), row["quality"], row["mult"], REWARDS_L, mutant)}


# ----------------------------------------------------------------------------------------------------------------------------------
# step_stats (rollout_fused.hip: env e reduced by 16 blocks of 256 threads over slices of ceil(L / 16) bins, the partials added in slice
# order by the env's last block, which also does the scalar work)
# ----------------------------------------------------------------------------------------------------------------------------------
STEP_N, STEP_L, STEP_A = (1, 3, 14), (1, 15, 17, 16 * 256 + 1, 16384), (1, 3)
STEP_OE = {"override": (1, 0), "override+extra": (1, 1), "env rewards": (0, 0)}
STEP_MULT = 20.0
STEP_MUTANTS = ("the last slice dropped when L % 16 != 0", "the right binaural channel read at offset 1 in place of 2", "partials added without the 2L division")


def _step_rows():
    R = []
    for (iL, L), (io, oe) in itertools.product(enumerate(STEP_L), enumerate(STEP_OE)):
        N, A = STEP_N[(iL + io) % 3], STEP_A[(iL + io // 2) % 2]
        dgs, nd = iL % 2 == 0, "all done" if (iL * 3 + io) % 5 == 4 else "some done"
        R.append(dict(id="step.N%d.L%d.A%d.%s.%s.%s" % (N, L, A, oe.replace(" ", "_"), "dgs" if dgs else "nodgs", nd.replace(" ", "_")), family="step_stats",
                      N=N, L=L, A=A, oe=oe, dgs=dgs, nd=nd))
    return R


STEP_ROWS = _step_rows()


def step_slices(L):
    """(bins per slice, number of non-empty slices) of the 16-way split."""
    per = cdiv(L, STEP_STATS_CHUNKS)
    return per, cdiv(L, per)


def step_cells(row):
    L = row["L"]
    per, used = step_slices(L)
    out = {"N=%d" % row["N"], "L=%d" % L, "A=%d" % row["A"], row["oe"], ("L=%d" % L, row["oe"]), "ndgs / dgs present" if row["dgs"] else "ndgs / dgs absent",
           "not_done: " + row["nd"]}
    if used < STEP_STATS_CHUNKS:
        out.add("empty slices")
    if L % STEP_STATS_CHUNKS:
        out.add("ragged last slice")
    if per > STEP_STATS_BLOCK:
        out.add("a thread takes a second bin")
    return out


def step_all_cells():
    return ({"N=%d" % N for N in STEP_N} | {"L=%d" % L for L in STEP_L} | {"A=%d" % A for A in STEP_A} | set(STEP_OE) |
            {("L=%d" % L, oe) for L in STEP_L for oe in STEP_OE} | {"ndgs / dgs present", "ndgs / dgs absent", "not_done: some done", "not_done: all done",
                                                                    "empty slices", "ragged last slice", "a thread takes a second bin"})


STATS_FIELDS = ("episode_rewards", "episode_counts", "episode_steps", "episode_dist_probs", "episode_bin_losses_allSteps", "episode_mono_losses_lastStep",
                "episode_mono_losses_allSteps", "episode_monoFromMem_losses_lastStep", "episode_monoFromMem_losses_allSteps", "current_episode_reward",
                "current_episode_step", "current_episode_dist_probs", "current_episode_bin_losses", "current_episode_mono_losses",
                "current_episode_monoFromMem_losses", "episode_ndgs", "episode_dgs")


def step_inputs(row):
    g = _gen(row["id"])
    N, L, A = row["N"], row["L"], row["A"]
    ru = lambda *s: torch.rand(*s, generator=g)
    nd = torch.zeros(N, 1) if row["nd"] == "all done" else (ru(N, 1) > 0.3).float()
    if row["nd"] == "some done":
        nd[0] = 0.0 if N > 1 else 1.0
        nd[N - 1] = 1.0
    d = dict(next_mem=ru(N, L, 1, 1), next_gt_mono_comps=ru(N, L, 1, 4) + 0.1, mem=ru(N, L, 1, 1), gt_mono_comps=ru(N, L, 1, 4) + 0.1,
             masks=torch.randn(N, L, 1, 2, generator=g), mix=ru(N, L, 1, 2) * 1.5, gt_bin_comps=ru(N, L, 1, 8), mono=ru(N, L, 1, 1), not_done=nd,
             probs=torch.softmax(torch.randn(N, A, generator=g), 1), env_rewards=torch.randn(N, 1, generator=g),
             ndgs=torch.randn(N, 1, generator=g) if row["dgs"] else None, dgs=torch.randn(N, 1, generator=g) if row["dgs"] else None)
    d["stats"] = {n: ru(N, A if "dist_probs" in n else 1) + 1.0 for n in STATS_FIELDS}
    return d


def step_reference(row, inp):
    """Rewards and the three losses: the sums as in reward_reference, the reward's ratios with the sums made by the kernel itself."""
    N, L = row["N"], row["L"]
    ov, extra = STEP_OE[row["oe"]]
    x = {k: _d(inp[k]).reshape(N, L, -1) for k in ("next_mem", "next_gt_mono_comps", "mem", "gt_mono_comps", "masks", "mix", "gt_bin_comps", "mono")}
    gt = x["gt_mono_comps"]
    if ov:
        ng = x["next_gt_mono_comps"][..., 0]
        nxt = np.stack((((x["next_mem"][..., 0] - ng) ** 2).sum(1), (ng * ng).sum(1)), 1)
        cur = np.stack((((x["mem"][..., 0] - gt[..., 0]) ** 2).sum(1), (gt[..., 0] ** 2).sum(1)), 1)
        r, s = _rewards64(nxt, cur, _d(inp["not_done"]), not extra, float(F32(STEP_MULT)), 3.0)
    else:
        r = _d(inp["env_rewards"]).reshape(N)
        s = np.zeros(N)
    losses, sc = np.zeros((3, N)), np.zeros((3, N))
    for ch in range(2):
        t, st = _stft_terms64(x["masks"], x["gt_bin_comps"], x["mix"], ch)
        losses[0], sc[0] = losses[0] + t.sum(1) / (2 * L), sc[0] + st.sum(1) / (2 * L)
    sc[0] = sc[0] + losses[0]
    for j, p in ((1, x["mono"]), (2, x["mem"])):
        t, st = _stft_terms64(p, gt, None, 0)
        losses[j], sc[j] = t.sum(1) / (2 * L), st.sum(1) / (2 * L)
    return {"rewards": (r, s), "losses": (losses, sc)}


def chunk_sums(terms, drop_last=False):
    """One env's sum of `terms` [L] as rollout_step_stats_kernel makes it: per slice the strided thread sums, the wave trees, (w0 + w1) +
    (w2 + w3); then the sixteen partials in slice order from zero."""
    terms = np.asarray(terms, dtype=F32).reshape(-1)
    L = terms.size
    per, used = step_slices(L)
    t = F32(0)
    for c in range(STEP_STATS_CHUNKS):
        seg = terms[c * per:min(L, c * per + per)] if c * per < L else terms[:0]
        th = thread_strided_sum(seg)
        w = [wave_tree(th[64 * i:64 * i + 64]) for i in range(4)]
        part = F32((w[0] + w[1]) + (w[2] + w[3]))
        if drop_last and c == used - 1:
            part = F32(0)
        t = F32(t + part)
    return t


def step_fp32(row, inp, mutant=None):
    N, L = row["N"], row["L"]
    ov, extra = STEP_OE[row["oe"]]
    x = {k: _f(inp[k]).reshape(N, L, -1) for k in ("next_mem", "next_gt_mono_comps", "mem", "gt_mono_comps", "masks", "mix", "gt_bin_comps", "mono")}
    drop = mutant == STEP_MUTANTS[0]
    tot = lambda t: np.array([chunk_sums(t[e], drop) for e in range(N)], dtype=F32)
    gt, mem = x["gt_mono_comps"][..., 0], x["mem"][..., 0]
    with np.errstate(all="ignore"):
        if ov:
            ng = x["next_gt_mono_comps"][..., 0]
            dn, dc = x["next_mem"][..., 0] - ng, mem - gt
            r = _rewards32(np.stack((tot(dn * dn), tot(ng * ng)), 1), np.stack((tot(dc * dc), tot(gt * gt)), 1), _f(inp["not_done"]), not extra, STEP_MULT, L)
        else:
            r = _f(inp["env_rewards"]).reshape(N)
        L2 = F32(1) if mutant == STEP_MUTANTS[2] else F32(2 * L)
        e = (np.exp(x["mix"], dtype=F32) - F32(1)) * x["masks"]
        dl = x["gt_bin_comps"][..., 0] - e[..., 0]
        dr = x["gt_bin_comps"][..., 1 if mutant == STEP_MUTANTS[1] else 2] - e[..., 1]
        dm, df = gt - x["mono"][..., 0], gt - mem
        losses = np.stack((tot(dl * dl) / L2 + tot(dr * dr) / L2, tot(dm * dm) / L2, tot(df * df) / L2)).astype(F32)
    return {"rewards": r.astype(F32), "losses": losses}


def episode_bookkeeping(stats, rewards, losses, probs, not_done, ndgs, dgs):
    """The elementwise float32 bookkeeping of one step (tests/test_gpu_rl.py test_episode_stats_update_matches_the_elementwise_bookkeeping)
    on CPU float32 tensors: -> the statistics after the step.  rewards [N,1], losses [3,N]."""
    r = {n: t.clone().float() for n, t in stats.items()}
    N = rewards.numel()
    bl, ml, fl = (losses[j].reshape(N, 1).float() for j in range(3))
    m = not_done.reshape(N, 1).float()
    nd = 1 - m
    r["current_episode_reward"] += rewards.reshape(N, 1).float()
    r["current_episode_step"] += 1
    r["current_episode_dist_probs"] += probs.float()
    r["current_episode_bin_losses"] += bl
    r["current_episode_mono_losses"] += ml
    r["current_episode_monoFromMem_losses"] += fl
    r["episode_rewards"] += nd * r["current_episode_reward"]
    if ndgs is not None:
        r["episode_ndgs"] += nd * ndgs.reshape(N, 1).float()
    if dgs is not None:
        r["episode_dgs"] += nd * dgs.reshape(N, 1).float()
    r["episode_steps"] += nd * r["current_episode_step"]
    r["episode_counts"] += nd
    r["episode_dist_probs"] += nd * (r["current_episode_dist_probs"] / r["current_episode_step"])
    r["episode_bin_losses_allSteps"] += nd * (r["current_episode_bin_losses"] / r["current_episode_step"])
    r["episode_mono_losses_lastStep"] += nd * ml
    r["episode_mono_losses_allSteps"] += nd * (r["current_episode_mono_losses"] / r["current_episode_step"])
    r["episode_monoFromMem_losses_lastStep"] += nd * fl
    r["episode_monoFromMem_losses_allSteps"] += nd * (r["current_episode_monoFromMem_losses"] / r["current_episode_step"])
    for n in ("current_episode_reward", "current_episode_step", "current_episode_bin_losses", "current_episode_mono_losses",
              "current_episode_monoFromMem_losses", "current_episode_dist_probs"):
        r[n].mul_(m)
    return r


# ----------------------------------------------------------------------------------------------------------------------------------
# mem (acoustic_mem.hip: slice + concat, conv3x3 + ReLU, conv3x3, de-slice in one launch; a workgroup owns two output rows of one image)
# ----------------------------------------------------------------------------------------------------------------------------------
MEM_ND = ("absent", "ones", "mixed", "zero")
MEM_W = ("he", "positive")
MEM_IN = ("random", "impulse")
MEM_MUTANTS = ("hidden rows outside the image hold conv outputs", "the left halo column of the input patch is not zero",
               "the right halo column of the input patch is not zero", "the left halo column of the hidden patch is not zero",
               "the right halo column of the hidden patch is not zero", "not_done also scales pred_mono", "de-slice rows band * 32 + r swapped to r * 16 + band")


def _mem_rows():
    combos = [(nd, w, x) for nd in MEM_ND for w in MEM_W for x in MEM_IN]
    R = [(2, c) for c in combos] + [(1, combos[i]) for i in (0, 5, 12, 15)] + [(15, combos[i]) for i in (3, 6, 9, 12)]
    return [dict(id="mem.B%d.nd_%s.w_%s.x_%s" % (B, nd, w, x), family="mem", B=B, nd=nd, w=w, x=x) for B, (nd, w, x) in R]


MEM_ROWS = _mem_rows()


def mem_cells(row):
    return {"B=%d" % row["B"], "not_done " + row["nd"], "weights " + row["w"], "inputs " + row["x"], (row["w"], row["x"]), ("not_done " + row["nd"], row["w"])}


def mem_all_cells():
    return ({"B=%d" % B for B in (1, 2, 15)} | {"not_done " + k for k in MEM_ND} | {"weights " + k for k in MEM_W} | {"inputs " + k for k in MEM_IN} |
            {(w, x) for w in MEM_W for x in MEM_IN} | {("not_done " + k, w) for k in MEM_ND for w in MEM_W})


def mem_inputs(row):
    g = _gen(row["id"])
    B = row["B"]
    mono, prev = torch.rand(B, 512, 32, 1, generator=g) * 2, torch.rand(B, 512, 32, 1, generator=g) * 2
    if row["x"] == "impulse":       # non-zero only at frequency rows {0, 31} of each band and time frames {0, 31}: every output they reach sits on a border
        keep = torch.zeros(16, 32, 32)
        for r in (0, 31):
            for t in (0, 31):
                keep[:, r, t] = 1.0
        keep = keep.reshape(1, 512, 32, 1)
        mono, prev = (mono + 0.5) * keep, (prev + 0.5) * keep
    w0 = torch.randn(32, 32, 3, 3, generator=g) * (2.0 / 288) ** 0.5      # kaiming_normal_, gain of relu, fan_in 32 x 9
    w1 = torch.randn(16, 32, 3, 3, generator=g) * (2.0 / 288) ** 0.5
    if row["w"] == "positive":      # first-conv outputs all positive on the non-negative inputs: the ReLU hides nothing
        w0 = w0.abs()
    nd = {"absent": None, "ones": torch.ones(B), "zero": torch.zeros(B), "mixed": (torch.arange(B) % 2 == 0).float()}[row["nd"]]
    return dict(pred_mono=mono, prev_mem=prev, not_done=nd, w0=w0, w1=w1)


def mem_sliced(mono, prev, nd, scale_mono=False):
    """[B,512,32,1] x 2 -> NCHW [B,32,32,32]: channel c < 16 band c of pred_mono, c >= 16 band c - 16 of the previous memory x not-done."""
    B = mono.shape[0]
    a, b = mono.reshape(B, 16, 32, 32), prev.reshape(B, 16, 32, 32)
    if nd is not None:
        b = b * nd.reshape(B, 1, 1, 1)
        if scale_mono:
            a = a * nd.reshape(B, 1, 1, 1)
    return torch.cat((a, b), 1) if torch.is_tensor(a) else np.concatenate((a, b), 1)


def mem_reference(row, inp, tau=None):
    tau = TAU["mem"] if tau is None else tau
    F_ = torch.nn.functional
    B = row["B"]
    nd = inp["not_done"].double() if inp["not_done"] is not None else None
    x = mem_sliced(inp["pred_mono"].double(), inp["prev_mem"].double(), nd)
    w0, w1 = inp["w0"].double(), inp["w1"].double()
    h0 = F_.conv2d(x, w0, None, 1, 1)
    s_h = torch.sqrt(F_.conv2d(x * x, w0 * w0, None, 1, 1))
    h = torch.relu(h0)
    y = F_.conv2d(h, w1, None, 1, 1)
    live = (h0 > -tau * s_h).double()
    s_y = torch.sqrt(F_.conv2d(h * h, w1 * w1, None, 1, 1)) + F_.conv2d(s_h * live, w1.abs(), None, 1, 1)
    return {"out": (y.reshape(B, 512, 32, 1).numpy(), s_y.reshape(B, 512, 32, 1).numpy())}     # [b][band][r][t] -> row band * 32 + r


def _conv3x3_mfma(xp, w):
    """xp [B, H + 2, W + 2, 32] float32 with its halo, w [Co, 32, 3, 3] -> [B, H, W, Co]: the kernel's k order -- tap by tap, the two 16-channel
    halves, and of each four v_mfma_f32_16x16x4_f32: MFMA e adds channels 4 kq + e, kq = 0 .. 3, to the accumulator."""
    B, H, W = xp.shape[0], xp.shape[1] - 2, xp.shape[2] - 2
    acc = np.zeros((B, H, W, w.shape[0]), dtype=F32)
    for tap in range(9):
        th, tw = divmod(tap, 3)
        for half in range(2):
            for e in range(4):
                ch = [half * 16 + 4 * kq + e for kq in range(4)]
                p = xp[:, th:th + H, tw:tw + W, None, ch] * w[None, None, None, :, ch, th, tw]
                acc = acc + (((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])
    return acc


def mem_fp32(row, inp, mutant=None):
    B = row["B"]
    nd = _f(inp["not_done"]) if inp["not_done"] is not None else None
    x = mem_sliced(_f(inp["pred_mono"]), _f(inp["prev_mem"]), nd, mutant == MEM_MUTANTS[5]).transpose(0, 2, 3, 1)      # NHWC [B,32,32,32]
    w0, w1 = _f(inp["w0"]), _f(inp["w1"])

    def halo(a, rows, left, right):
        p = np.zeros((a.shape[0], a.shape[1] + 2 * rows, a.shape[2] + 2, a.shape[3]), dtype=F32)
        p[:, rows:rows + a.shape[1], 1:-1] = a
        if left:                                # a stale column stands in for the zeros: the edge pixel's values
            p[:, :, 0] = p[:, :, 1]
        if right:
            p[:, :, -1] = p[:, :, -2]
        return p
    # hidden rows -1 .. 32 (the tiles at the image's top and bottom compute one row outside it): input rows -2 .. 33
    h = np.maximum(_conv3x3_mfma(halo(x, 2, mutant == MEM_MUTANTS[1], mutant == MEM_MUTANTS[2]), w0), F32(0))      # [B,34,32,32]
    if mutant != MEM_MUTANTS[0]:
        h[:, 0], h[:, -1] = 0, 0
    y = _conv3x3_mfma(halo(h, 0, mutant == MEM_MUTANTS[3], mutant == MEM_MUTANTS[4]), w1)                          # [B,32,32,16] = [b][r][t][band]
    if mutant == MEM_MUTANTS[6]:
        return {"out": y.transpose(0, 1, 3, 2).reshape(B, 512, 32, 1)}                                            # row r * 16 + band
    return {"out": np.ascontiguousarray(y.transpose(0, 3, 1, 2)).reshape(B, 512, 32, 1)}


# ----------------------------------------------------------------------------------------------------------------------------------
# glue (rollout_ops.hip slice_concat_kernel, visual_input_kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
GLUE_MUTANTS = ("op 1 without the clamp", "slice row s * Hs + h swapped to h * 16 + s", "bscale applied to a", "multiplication by a float32 1/255 in place of the division")
VIS_NPIX = (1, 255, 257, 4096 * 256 + 1)


def _glue_rows():
    R = []
    sizes = [(F, T, B) for F in (16, 32, 512) for T in (1, 3, 32) for B in (1, 3)]
    variants = [(0, 1, 0, False), (0, 1, 1, False), (0, 1, 1, True), (0, 1, 2, False), (0, 1, 2, True), (1, 2, 0, False), (2, 1, 1, False)]
    for i, (F, T, B) in enumerate(sizes):
        for j in (0, 1):                        # two variants per size, all seven over the sizes, each with several
            op, Ca, Cb, bs = variants[(2 * i + j) % 7]
            R.append(dict(id="slice.op%d.Ca%d.Cb%d.%s.F%d.T%d.B%d" % (op, Ca, Cb, "bscale" if bs else "plain", F, T, B), family="glue", kernel="slice_concat_input",
                          op=op, Ca=Ca, Cb=Cb, bscale=bs, F=F, T=T, B=B))
    R.append(dict(id="slice.op0.Ca1.Cb1.bscale.F512.T32.B129", family="glue", kernel="slice_concat_input", op=0, Ca=1, Cb=1, bscale=True, F=512, T=32, B=129))
    R += [dict(id="visual.npix%d.%s" % (n, "depth" if d else "rgb"), family="glue", kernel="visual_input", npix=n, depth=d) for n in VIS_NPIX for d in (False, True)]
    return R


GLUE_ROWS = _glue_rows()


def glue_total(row):
    """Work items of the launch (16-byte groups of the output, or pixels)."""
    if row["kernel"] == "visual_input":
        return row["npix"]
    return row["B"] * (row["F"] // 16) * row["T"] * (16 * (row["Ca"] + row["Cb"]) // 4)


def glue_cells(row):
    k = row["kernel"]
    loop = (k, "grid-stride second pass") if enters_grid_stride_loop(glue_total(row), GLUE_CAP) else (k, "one item per thread")
    if k == "visual_input":
        return {(k, "npix=%d" % row["npix"]), (k, "depth present" if row["depth"] else "depth absent"), loop}
    return {(k, "op %d, Ca=%d, Cb=%d, %s" % (row["op"], row["Ca"], row["Cb"], "bscale" if row["bscale"] else "no bscale")), (k, "F=%d" % row["F"]),
            (k, "T=%d" % row["T"]), (k, "B=%d" % row["B"]) if row["B"] <= 3 else (k, "B * C > 256"), loop}


def glue_all_cells():
    k = "slice_concat_input"
    out = {(k, "op 0, Ca=1, Cb=%d, %s" % (cb, b)) for cb, b in ((0, "no bscale"), (1, "no bscale"), (1, "bscale"), (2, "no bscale"), (2, "bscale"))}
    out |= {(k, "op 1, Ca=2, Cb=0, no bscale"), (k, "op 2, Ca=1, Cb=1, no bscale"), (k, "B * C > 256"), (k, "grid-stride second pass"), (k, "one item per thread")}
    out |= {(k, "F=%d" % F) for F in (16, 32, 512)} | {(k, "T=%d" % T) for T in (1, 3, 32)} | {(k, "B=1"), (k, "B=3")}
    k = "visual_input"
    return out | {(k, "npix=%d" % n) for n in VIS_NPIX} | {(k, "depth present"), (k, "depth absent"), (k, "grid-stride second pass"), (k, "one item per thread")}


def glue_inputs(row):
    g = _gen(row["id"])
    if row["kernel"] == "visual_input":
        n = row["npix"]
        rgb = torch.randint(0, 256, (1, n, 1, 3), generator=g).float()
        rgb.view(-1)[:min(256, 3 * n)] = torch.arange(min(256, 3 * n)).float()       # every value 0 .. 255 where there is room
        return dict(rgb=rgb, depth=torch.rand(1, n, 1, 1, generator=g) if row["depth"] else None)
    B, F, T, Ca, Cb = (row[k] for k in ("B", "F", "T", "Ca", "Cb"))
    op = row["op"]
    a = torch.rand(B, F, T, Ca, generator=g) * 1.5 if op == 1 else torch.randn(B, F, T, Ca, generator=g)
    return dict(a=a, b=torch.randn(B, F, T, Cb, generator=g) if Cb else None, mul=torch.randn(B, F, T, Ca, generator=g) if op == 1 else None,
                bscale=torch.rand(B, generator=g) + 0.5 if row["bscale"] else None)


def _slice_layout(v, swapped=False):
    """virtual [B, F, T, C] -> [B, F/16, T, C * 16]: out[b][h][t][c * 16 + s] = v[b][s * Hs + h][t][c]."""
    B, F, T, C = v.shape
    Hs = F // 16
    if swapped:                                 # MUTANT: frequency row h * 16 + s
        v5 = v.reshape(B, Hs, 16, T, C).transpose(0, 2, 1, 3, 4)
    else:
        v5 = v.reshape(B, 16, Hs, T, C)
    return np.ascontiguousarray(v5.transpose(0, 2, 3, 4, 1)).reshape(B, Hs, T, C * 16)


def glue_reference(row, inp, tau=None):
    """-> {"out": (r, s)} and, for ops 1 and 2, "near_clamp": the elements whose float64 argument lies within tau s of the clamp (log1p(max(0, .))
    is continuous there: either side is within tau s of the other, which is what their scale says)."""
    tau = TAU["glue"] if tau is None else tau
    if row["kernel"] == "visual_input":
        n = row["npix"]
        rgb = _f(inp["rgb"]).reshape(n, 3)
        out = np.zeros((n, 4), dtype=F32)
        out[:, :3] = rgb / F32(255)             # float32 division, correctly rounded
        if row["depth"]:
            out[:, 3] = _f(inp["depth"]).reshape(n)
        return {"out": (out.astype(np.float64).reshape(1, n, 1, 4), np.zeros((1, n, 1, 4)))}
    op = row["op"]
    a = _d(inp["a"])
    s_a = _z(a)
    near = np.zeros(a.shape, dtype=bool)
    if op == 1:
        u = np.exp(a)
        mul = _d(inp["mul"])
        p = mul * (u - 1)
        s_p = np.abs(mul) * (u + 1) + np.abs(p)
        near = np.abs(p) <= tau * s_p
        a = np.log1p(np.maximum(p, 0))
        s_a = np.where((p > 0) | near, s_p / (1 + np.maximum(p, 0)) + a, 0.0)
    v, s_v = a, s_a
    if row["Cb"]:
        b = _d(inp["b"])
        s_b = _z(b)
        if row["bscale"]:
            b = b * _d(inp["bscale"]).reshape(-1, 1, 1, 1)
            s_b = np.abs(b)
        v, s_v = np.concatenate((a, b), 3), np.concatenate((s_a, s_b), 3)
        near = np.concatenate((near, np.zeros(b.shape, dtype=bool)), 3)
    if op == 2:
        near = np.abs(v) <= tau * s_v
        y = np.log1p(np.maximum(v, 0))
        s_v = np.where((v > 0) | near, s_v / (1 + np.maximum(v, 0)) + y, 0.0)
        v = y
    return {"out": (_slice_layout(v), _slice_layout(s_v)), "near_clamp": _slice_layout(near)}


def glue_fp32(row, inp, mutant=None):
    if row["kernel"] == "visual_input":
        n = row["npix"]
        rgb = _f(inp["rgb"]).reshape(n, 3)
        out = np.zeros((n, 4), dtype=F32)
        out[:, :3] = rgb * (F32(1) / F32(255)) if mutant == GLUE_MUTANTS[3] else rgb / F32(255)
        if row["depth"]:
            out[:, 3] = _f(inp["depth"]).reshape(n)
        return {"out": out.reshape(1, n, 1, 4)}
    op = row["op"]
    a = _f(inp["a"])
    with np.errstate(all="ignore"):
        if mutant == GLUE_MUTANTS[2] and row["bscale"]:
            a = a * _f(inp["bscale"]).reshape(-1, 1, 1, 1)
        if op == 1:
            p = _f(inp["mul"]) * (np.exp(a, dtype=F32) - F32(1))
            a = np.log1p(p if mutant == GLUE_MUTANTS[0] else np.maximum(p, F32(0)), dtype=F32)
        v = a
        if row["Cb"]:
            b = _f(inp["b"])
            if row["bscale"] and mutant != GLUE_MUTANTS[2]:
                b = b * _f(inp["bscale"]).reshape(-1, 1, 1, 1)
            v = np.concatenate((a, b), 3)
        if op == 2:
            v = np.log1p(np.maximum(v, F32(0)), dtype=F32)
    return {"out": _slice_layout(v.astype(F32), mutant == GLUE_MUTANTS[1])}


# ----------------------------------------------------------------------------------------------------------------------------------
# copy (rollout_ops.hip gather_envs, rows_copy, synth_env_step, synth_env_observe, step_index_advance): exact equality with indexing
# ----------------------------------------------------------------------------------------------------------------------------------
def gather_items(T, nsel, Lw):
    """Items of gather_envs_kernel's loop: 16-byte words where the row is whole ones, else 4-byte words."""
    return T * nsel * (Lw // 4 if Lw % 4 == 0 else Lw)


def rows_copy_threads(big_bytes, cap):
    """Threads along x of rows_copy_kernel (cap 256 blocks) / rows_gather_kernel (cap 64), sized by the largest row in 16-byte words."""
    return 256 * max(1, min(cap, cdiv(big_bytes // 16, 256)))


def rows_copy_second_pass(row_bytes, big_bytes, cap):
    """A thread of the launch copies a second word of this row (16-byte words when the size allows them -- the tests' rows are then
    16-byte aligned --, else 4-byte words)."""
    words = row_bytes // 16 if row_bytes % 16 == 0 else row_bytes // 4
    return words > rows_copy_threads(big_bytes, cap)


def nbytes(n, dtype):
    return n * (8 if dtype == "int64" else 4)


def _copy_rows():
    R = []
    perms = ("one", "all", "repeats")
    i = 0
    for Lw in (1, 3, 4, 6, 8):
        for T in (1, 3):
            for N in (1, 14):
                for dt in ("float32", "int64"):
                    if dt == "int64" and Lw % 2:
                        continue
                    perm = perms[i % 3]
                    i += 1
                    R.append(dict(id="gather.Lw%d.T%d.N%d.%s.%s" % (Lw, T, N, perm, dt), family="copy", kernel="gather_envs", Lw=Lw, T=T, N=N, perm=perm, dtype=dt, nsel=0))
    R += [dict(id="gather.Lw3.T1.N14.big.float32", family="copy", kernel="gather_envs", Lw=3, T=1, N=14, perm="repeats", dtype="float32", nsel=699100),
          dict(id="gather.Lw4.T1.N14.big.float32", family="copy", kernel="gather_envs", Lw=4, T=1, N=14, perm="repeats", dtype="float32", nsel=GATHER_CAP * 256 + 3)]
    R += [dict(id="rows_copy.%s" % k, family="copy", kernel="rows_copy", kind=k) for k in ("words257", "over1MiB", "items33")]
    R += [dict(id="env_step.N%d.nodes%d" % (N, n), family="copy", kernel="synth_env_step", N=N, n_nodes=n) for N in (1, 64, 65) for n in (1, 7)]
    R += [dict(id="env_observe.%s" % k, family="copy", kernel="synth_env_observe", kind=k) for k in ("small", "second_pass")]
    R += [dict(id="step_index.%s" % k, family="copy", kernel="step_index_advance", kind=k, **v) for k, v in STEP_INDEX_CASES.items()]
    return R


# (elements of a row, dtype) per item / (elements, dtype, index kind) per pool
# idx before -> T_pol, T_sep, rng increment (None: the entry without the RNG state)
STEP_INDEX_CASES = {"T1": dict(idx=(0, 1, 1), T_pol=1, T_sep=1, rng_inc=None), "wrap": dict(idx=(4, 5, 5), T_pol=5, T_sep=5, rng_inc=None),
                    "mid": dict(idx=(1, 2, 2), T_pol=5, T_sep=5, rng_inc=7), "T_pol_ne_T_sep": dict(idx=(2, 3, 6), T_pol=3, T_sep=6, rng_inc=2 ** 40 + 5)}
COPY_ROWS = _copy_rows()
ROWS_COPY_SHAPES = {"words257": [(257, "float32")], "over1MiB": [(ROWS_COPY_GX * 256 * 4 + 8, "float32")],
                    "items33": [((4, 1, 6, 8, 257)[i % 5], "int64" if i % 4 == 3 else "float32") for i in range(33)]}
OBSERVE_POOLS = {"small": [(257, "float32", 0), (8, "float32", 1), (3, "int64", 0), (2, "int64", 1)],
                 "second_pass": [(257, "float32", 1), (OBSERVE_GX * 256 * 4 + 4, "float32", 0), (4, "int64", 1)]}


def step_index_reference(case):
    i0, _i1, i2 = case["idx"]
    p = (i0 + 1) % case["T_pol"]
    return (p, p + 1, i2 % case["T_sep"] + 1)


def synth_env_step_reference(actions, node, angle, n_nodes):
    a = np.asarray(actions)
    return (node + (a == 0)) % n_nodes, (angle + (a == 1) + 3 * (a == 2)) % 4


def env_step_inputs(row):
    g = _gen(row["id"])
    N, n = row["N"], row["n_nodes"]
    actions = torch.randint(-1, 4, (N,), generator=g)          # 0, 1, 2 and the values outside them (nothing moves)
    node, angle = torch.randint(0, n, (N,), generator=g), torch.randint(0, 4, (N,), generator=g)
    pre = [(0, n - 1, 0), (1, 0, 3), (2, 0, 1), (2, 0, 3), (3, n - 1, 3), (-1, 0, 0)]      # wrap of the node and of the angle by either turn
    for e, (a, nd, an) in enumerate(pre[:N]):
        actions[e], node[e], angle[e] = a, nd, an
    return dict(actions=actions, node=node, angle=angle)


def copy_cells(row):
    k = row["kernel"]
    if k == "gather_envs":
        nsel = row["nsel"] or {"one": 1, "all": row["N"], "repeats": row["N"] + 3}[row["perm"]]
        path = "16-byte path" if row["Lw"] % 4 == 0 else "4-byte path"
        out = {(k, "Lw=%d" % row["Lw"]), (k, "T=%d" % row["T"]), (k, "N=%d" % row["N"]), (k, "perm " + row["perm"]), (k, row["dtype"]), (k, path)}
        if enters_grid_stride_loop(gather_items(row["T"], nsel, row["Lw"]), GATHER_CAP):
            out.add((k, path + ", grid-stride second pass"))
        return out
    if k == "rows_copy":
        shapes = ROWS_COPY_SHAPES[row["kind"]]
        big = max(nbytes(n, dt) for n, dt in shapes)
        out = {(k, row["kind"])}
        for n, dt in shapes:
            if rows_copy_second_pass(nbytes(n, dt), big, ROWS_COPY_GX):
                out.add((k, "16-byte path, second pass" if nbytes(n, dt) % 16 == 0 else "4-byte path, second pass"))
        if len(shapes) > ROWS_COPY_MAX:
            out.add((k, "more than one launch"))
        return out
    if k == "synth_env_step":
        return {(k, "N=%d" % row["N"]), (k, "n_nodes=%d" % row["n_nodes"])}
    if k == "synth_env_observe":
        pools = OBSERVE_POOLS[row["kind"]]
        big = max(nbytes(n, dt) for n, dt, _ in pools)
        out = {(k, row["kind"])}
        for n, dt, kind in pools:
            nb = nbytes(n, dt)
            out |= {(k, "index kind %d" % kind), (k, dt), (k, "16-byte rows" if nb % 16 == 0 else "4-byte rows")}
            if rows_copy_second_pass(nb, big, OBSERVE_GX):
                out.add((k, "16-byte path, second pass" if nb % 16 == 0 else "4-byte path, second pass"))
        return out
    return {(k, row["kind"]), (k, "rng advanced" if row["rng_inc"] is not None else "no rng")}


def copy_all_cells():
    k = "gather_envs"
    out = {(k, "Lw=%d" % w) for w in (1, 3, 4, 6, 8)} | {(k, "T=1"), (k, "T=3"), (k, "N=1"), (k, "N=14"), (k, "float32"), (k, "int64"), (k, "16-byte path"),
                                                         (k, "4-byte path"), (k, "16-byte path, grid-stride second pass"), (k, "4-byte path, grid-stride second pass")}
    out |= {(k, "perm " + p) for p in ("one", "all", "repeats")}
    out |= {("rows_copy", x) for x in ("words257", "over1MiB", "items33", "16-byte path, second pass", "4-byte path, second pass", "more than one launch")}
    out |= {("synth_env_step", "N=%d" % N) for N in (1, 64, 65)} | {("synth_env_step", "n_nodes=1"), ("synth_env_step", "n_nodes=7")}
    k = "synth_env_observe"
    out |= {(k, x) for x in ("small", "second_pass", "index kind 0", "index kind 1", "float32", "int64", "16-byte rows", "4-byte rows", "16-byte path, second pass",
                             "4-byte path, second pass")}
    return out | {("step_index_advance", x) for x in tuple(STEP_INDEX_CASES) + ("rng advanced", "no rng")}


# ----------------------------------------------------------------------------------------------------------------------------------
# the families together
# ----------------------------------------------------------------------------------------------------------------------------------
ROWS = {"gae": GAE_ROWS, "adv": ADV_ROWS, "reward": REWARD_ROWS, "step_stats": STEP_ROWS, "mem": MEM_ROWS, "glue": GLUE_ROWS, "copy": COPY_ROWS}
ROWS_BY_ID = {r["id"]: r for rows in ROWS.values() for r in rows}
CELLS = {"gae": gae_cells, "adv": adv_cells, "reward": reward_cells, "step_stats": step_cells, "mem": mem_cells, "glue": glue_cells, "copy": copy_cells}
_ALL = {"gae": gae_all_cells, "adv": adv_all_cells, "reward": reward_all_cells, "step_stats": step_all_cells, "mem": mem_all_cells, "glue": glue_all_cells,
        "copy": copy_all_cells}
INPUTS = {"gae": gae_inputs, "adv": adv_inputs, "reward": reward_inputs, "step_stats": step_inputs, "mem": mem_inputs, "glue": glue_inputs}
FP32 = {"gae": gae_fp32, "adv": adv_fp32, "reward": reward_fp32, "step_stats": step_fp32, "mem": mem_fp32, "glue": glue_fp32}


def cells(row):
    return CELLS[row["family"]](row)


def all_cells(family):
    return _ALL[family]()


def inputs(row):
    return INPUTS[row["family"]](row)


def reference(row, inp, state=None):
    """{output: (r, s)} in float64.  state: the float32 values another step handed on (adv only)."""
    f = row["family"]
    if f == "adv":
        return adv_reference(row, inp, state)
    return {"gae": gae_reference, "reward": reward_reference, "step_stats": step_reference, "mem": mem_reference, "glue": glue_reference}[f](row, inp)


def _gae_live(r):
    """Some env's recursion runs through a non-zero mask."""
    return r["mask"] == "ones" or (r["mask"] in ("random", "ends") and r["N"] >= 63)


# mutant -> (family, predicate on the row: the rows the bound must reject the mutant on)
MUTANT_ROWS = {
    GAE_MUTANTS[0]: ("gae", lambda r: r["mask"] == "ends"),
    GAE_MUTANTS[1]: ("gae", lambda r: r["gae"] and r["gt"] != "g1t1" and r["T"] >= 2 and _gae_live(r)),
    GAE_MUTANTS[2]: ("gae", lambda r: r["gae"]),
    ADV_MUTANTS[0]: ("adv", lambda r: r["n"] <= 257),          # (at n = 4097 the two variances differ by 1.2e-4 relative: 2.4 tau s)
    ADV_MUTANTS[1]: ("adv", lambda r: r["dist"] != "std"),
    ADV_MUTANTS[2]: ("adv", lambda r: r["dist"] == "off100s0.01"),     # (sd = 1: sqrt(1 + eps) and 1 + eps differ by 5e-6)
    ADV_MUTANTS[3]: ("adv", lambda r: r["n"] % 256 != 0),
    REWARD_MUTANTS[0]: ("reward", lambda r: r["kernel"] == "stft_l2"),
    REWARD_MUTANTS[1]: ("reward", lambda r: r["kernel"] == "rewards_from_stats" and r["N"] > 1),
    REWARD_MUTANTS[2]: ("reward", lambda r: r["kernel"] == "rewards_from_stats" and r["quality"]),
    REWARD_MUTANTS[3]: ("reward", lambda r: r["kernel"] in ("sq_stats", "stft_l2") and r["L"] % 4096 != 0),
    REWARD_MUTANTS[4]: ("reward", lambda r: r["kernel"] == "sq_stats"),
    STEP_MUTANTS[0]: ("step_stats", lambda r: r["L"] % 16 != 0),
    STEP_MUTANTS[1]: ("step_stats", lambda r: True),
    STEP_MUTANTS[2]: ("step_stats", lambda r: True),
    MEM_MUTANTS[0]: ("mem", lambda r: r["B"] <= 2),
    MEM_MUTANTS[1]: ("mem", lambda r: r["B"] <= 2),
    MEM_MUTANTS[2]: ("mem", lambda r: r["B"] <= 2),
    MEM_MUTANTS[3]: ("mem", lambda r: r["B"] <= 2),
    MEM_MUTANTS[4]: ("mem", lambda r: r["B"] <= 2),
    MEM_MUTANTS[5]: ("mem", lambda r: r["B"] <= 2 and r["nd"] in ("mixed", "zero")),
    MEM_MUTANTS[6]: ("mem", lambda r: r["B"] <= 2),
    GLUE_MUTANTS[0]: ("glue", lambda r: r["kernel"] == "slice_concat_input" and r["op"] == 1),
    GLUE_MUTANTS[1]: ("glue", lambda r: r["kernel"] == "slice_concat_input" and r["F"] > 16),
    GLUE_MUTANTS[2]: ("glue", lambda r: r["kernel"] == "slice_concat_input" and r["bscale"] and r["B"] <= 3),
    GLUE_MUTANTS[3]: ("glue", lambda r: r["kernel"] == "visual_input" and r["npix"] >= 255),
}
