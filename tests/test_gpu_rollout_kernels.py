"""GPU: the rollout kernels -- csrc/advantage.hip (gae_returns, advantages modes 0 / 1 / 2, adv_sqdiff, adv_apply), the reward and distance
kernels of csrc/losses.hip (sq_stats, rewards_from_stats, stft_l2), csrc/rollout_fused.hip (rollout_step_stats), csrc/acoustic_mem.hip and
csrc/rollout_ops.hip (slice_concat_input, visual_input, gather_envs, rows_copy, synth_env_step, synth_env_observe, step_index_advance) -- on
every row of tests/rollout_kernels.py's table through the public m2h.ops function, every output element against the float64 reference of
the same float32 inputs: |g_e - r_e| <= tau * s_e (the scales and their one rule: tests/rollout_kernels.py, pinned on the CPU by
tests/test_rollout_kernels_cpu.py together with the mutants the bound must reject).  Every row also: all outputs finite, the library's
label of the launch, bit-identical results on a second call; copies, the pose update and the step counters by exact equality with indexing.

Calibrated on an MI355X (worst |g - r| / s over each family's rows, per output kind; test_zz_report_worst_ratios prints them with -s):
  gae         returns 2.8e-7 (gae), 4.6e-7 (discounted); value_preds exact
  adv         mean 3.1e-6 (the second shard's; the first's 2.4e-6), var 1.0e-7, mode-1 output 6.0e-8, sqdiff 1.4e-7, adv_apply 7.3e-8; modes 0 and 2 exact
  reward      sq_stats 1.5e-7, stft_l2 1.4e-7, rewards_from_stats 4.3e-8
  step_stats  rewards 4.1e-8, losses 2.2e-7 (fused); 4.6e-8 / 2.2e-7 (the separate kernels against the same reference)
  mem         out 1.6e-6
  glue        slice_concat_input 6.0e-8 (op 0 with bscale), 4.5e-8 (op 1), 6.1e-8 (op 2), exact for op 0 without bscale; visual_input exact
  copy        exact
Every family keeps TAU_FP32 = 2e-5 (the mean of the advantages and the memory's output are the figures above TAU_FP32 / 40: the float32
rounding of a mean near 100 against sqrt(sum s(a)^2) / n, under the constant for the rows' n <= 4097; two chained 288-term MFMA sums).
The 345 tests of this file take 4 s on an MI355X; no row found a kernel defect.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rollout_kernels as R
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
WORST = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _d(t):
    return t.to(_dev()).contiguous() if t is not None else None


def _ids(family, pred=lambda r: True):
    return [r["id"] for r in R.ROWS[family] if pred(r)]


def _check_row(family, row, route, got, ref, again=None, kind=None):
    """Every output of the row against (r, s); one printed line per row: route, worst ratio, scale - 1."""
    tau = R.TAU[family]
    line_w, line_s, fails, seen = 0.0, 0.0, [], 0
    for name, rs in ref.items():
        if name == "near_clamp" or name not in got:
            continue
        r, s = rs
        seen += 1
        g = got[name].detach().cpu()
        assert g.numel() == np.size(r), (row["id"], name, tuple(g.shape), np.shape(r))
        assert bool(torch.isfinite(g).all()), (row["id"], name, "not finite")
        worst, scale, ok = R.check(g, r, s, tau)
        key = (family, kind or row.get("kernel", family), name)
        WORST[key] = max(WORST.get(key, 0.0), worst)
        line_w = max(line_w, worst)
        line_s = scale - 1.0 if abs(scale - 1.0) > abs(line_s) else line_s
        if not ok:
            fails.append((name, worst, scale))
        if again is not None:
            assert torch.equal(g, again[name].detach().cpu()), (row["id"], name, "second call differs")
    assert seen
    print("%-58s %-28s worst |g-r|/s %.2e  scale-1 %+.1e" % (row["id"], route, line_w, line_s))
    assert not fails, (row["id"], fails)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_gae(row, inp):
    d = {k: _d(v.clone()) for k, v in inp.items()}
    gamma, tau = R.GAE_GT[row["gt"]]
    ops.gae_returns(d["rewards"], d["value_preds"], d["masks"], d["next_value"], d["returns"], bool(row["gae"]), gamma, tau)
    assert ops.last_kernel() == "gae_returns"
    torch.cuda.synchronize()
    return dict(returns=d["returns"], value_preds=d["value_preds"])


@pytest.mark.parametrize("row_id", _ids("gae"))
def test_gae_returns_match_fp64(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp = R.inputs(row)
    got, again = _run_gae(row, inp), _run_gae(row, inp)
    T = row["T"]
    ret, vp = got["returns"].cpu(), got["value_preds"].cpu()
    if row["gae"]:          # what the scan must write and what it must leave
        assert torch.equal(vp[T], inp["next_value"]) and torch.equal(vp[:T], inp["value_preds"][:T]) and bool((ret[T] == R.GAE_SENTINEL).all())
    else:
        assert torch.equal(vp, inp["value_preds"]) and torch.equal(ret[T], inp["next_value"])
    _check_row("gae", row, "gae" if row["gae"] else "discounted", got, R.reference(row, inp), again, kind="gae" if row["gae"] else "discounted")


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_adv(row, inp):
    dev = _dev()
    d = {k: _d(v) for k, v in inp.items()}
    one = lambda x: torch.tensor([float(x)], dtype=torch.float32, device=dev)      # noqa: E731
    adv0, st0 = ops.advantages(d["ret_a"], d["val_a"], 0)
    assert ops.last_kernel() == "advantages"
    adv1, st1 = ops.advantages(d["ret_a"], d["val_a"], 1, R.ADV_EPS)
    adv2, st2 = ops.advantages(d["ret_a"], d["val_a"], 2)
    advb, stb = ops.advantages(d["ret_b"], d["val_b"], 2)
    assert torch.equal(st0, st1) and torch.equal(st0, st2)         # the statistics do not depend on the mode
    # the distributed recipe at a simulated world of 2: the means, then the squared differences, averaged on the host in float64
    gm = one(R.adv_combine(st2[0].item(), stb[0].item()))
    sq_a, sq_b = ops.adv_sqdiff(adv2, gm), ops.adv_sqdiff(advb, gm)
    assert ops.last_kernel() == "adv_sqdiff"
    gv = one(R.adv_combine(sq_a.item(), sq_b.item()))
    ap_a, ap_b = ops.adv_apply(adv2.clone(), gm, gv, R.ADV_EPS), ops.adv_apply(advb.clone(), gm, gv, R.ADV_EPS)
    assert ops.last_kernel() == "adv_apply"
    torch.cuda.synchronize()
    return dict(adv0=adv0, adv2=adv2, mean=st0[0], var=st0[1], mean1=st1[0], adv1=adv1, mean_b=stb[0], sqdiff_a=sq_a, sqdiff_b=sq_b, apply_a=ap_a, apply_b=ap_b)


@pytest.mark.parametrize("row_id", _ids("adv"))
def test_advantages_match_fp64(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp = R.inputs(row)
    got, again = _run_adv(row, inp), _run_adv(row, inp)
    state = {k: got[k].item() for k in ("mean", "mean1", "mean_b", "sqdiff_a", "sqdiff_b")}
    assert got["adv0"].shape == (row["n"], 1, 1)
    _check_row("adv", row, "modes 0 / 1 / 2, sqdiff, apply", got, R.reference(row, inp, state), again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_reward(row, inp):
    d = {k: _d(v) for k, v in inp.items()}
    k = row["kernel"]
    if k == "sq_stats":
        out = {"stats": ops.sq_stats(d["pred"], d["gt"], row["off"])}
    elif k == "stft_l2":
        out = {"out": ops.stft_l2(d["pred"], d["gt"], row["nch"], mix=d["mix"])}
    else:
        out = {"rewards": ops.rewards_from_stats(d["next_stats"], d["cur_stats"] if row["quality"] else None, d["not_done"], R.REWARDS_L, row["quality"], row["mult"])}
    assert ops.last_kernel() == k
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("row_id", _ids("reward"))
def test_reward_kernels_match_fp64(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp = R.inputs(row)
    got, again = _run_reward(row, inp), _run_reward(row, inp)
    if row["kernel"] == "rewards_from_stats":
        done = inp["not_done"].reshape(-1) == 0
        assert got["rewards"].shape == (row["N"], 1) and float(got["rewards"].cpu().reshape(-1)[done].abs().sum()) == 0.0      # a finished env: exactly 0
    _check_row("reward", row, row["kernel"], got, R.reference(row, inp), again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_step(row, inp, scratch):
    dev = _dev()
    d = {k: _d(v) for k, v in inp.items() if k != "stats"}
    stats = SimpleNamespace(**{n: inp["stats"][n].clone().to(dev) for n in R.STATS_FIELDS})
    ov, extra = R.STEP_OE[row["oe"]]
    r, losses = ops.rollout_step_stats(stats, d["next_mem"], d["next_gt_mono_comps"], d["mem"], d["gt_mono_comps"], d["masks"], d["mix"], d["gt_bin_comps"],
                                       d["mono"], d["not_done"], d["probs"], env_rewards=d["env_rewards"], ndgs=d["ndgs"], dgs=d["dgs"], override=bool(ov),
                                       extra=bool(extra), extra_mult=R.STEP_MULT, scratch=scratch)
    assert ops.last_kernel() == "rollout_step_stats"
    torch.cuda.synchronize()
    assert int(scratch[1].abs().sum()) == 0                        # the tickets are back at zero
    return dict(rewards=r, losses=losses), stats, d


@pytest.mark.parametrize("row_id", _ids("step_stats"))
def test_rollout_step_stats_match_fp64(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp = R.inputs(row)
    N, L = row["N"], row["L"]
    scratch = ops.step_stats_scratch(N, _dev())                    # the test's own, used by both launches
    (got, stats, d), (again, stats2, _) = _run_step(row, inp, scratch), _run_step(row, inp, scratch)
    ov, extra = R.STEP_OE[row["oe"]]
    ref = R.reference(row, inp)
    _check_row("step_stats", row, "%d slices of %d" % R.step_slices(L)[::-1], got, ref, again, kind="fused")
    r, losses = got["rewards"].cpu(), got["losses"].cpu()
    if not ov:
        assert torch.equal(r, inp["env_rewards"])
    else:
        assert float(r.reshape(-1)[inp["not_done"].reshape(-1) == 0].abs().sum()) == 0.0
    # the episode statistics: the elementwise float32 bookkeeping on the kernel's own float32 reward and losses, bit for bit
    want = R.episode_bookkeeping(inp["stats"], r, losses, inp["probs"], inp["not_done"], inp["ndgs"], inp["dgs"])
    for n in R.STATS_FIELDS:
        assert torch.equal(getattr(stats, n).cpu(), want[n]), (row_id, n)
        assert torch.equal(getattr(stats, n), getattr(stats2, n)), (row_id, n, "second launch differs")
    # one reference, two implementations: the separate kernels on the same inputs, inside the same bound
    sep = {"losses": torch.stack((ops.stft_l2(d["masks"], d["gt_bin_comps"], 2, mix=d["mix"]).reshape(N), ops.stft_l2(d["mono"], d["gt_mono_comps"], 1).reshape(N),
                                  ops.stft_l2(d["mem"], d["gt_mono_comps"], 1).reshape(N)))}
    if ov:
        nxt = ops.sq_stats(d["next_mem"], d["next_gt_mono_comps"], 0)
        cur = None if extra else ops.sq_stats(d["mem"], d["gt_mono_comps"], 0)
        sep["rewards"] = ops.rewards_from_stats(nxt, cur, d["not_done"], L, not extra, R.STEP_MULT)
    _check_row("step_stats", row, "separate kernels", sep, ref, kind="separate")


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_mem(inp, w0p, w1p):
    out = ops.acoustic_mem_small(_d(inp["pred_mono"]), _d(inp["prev_mem"]), _d(inp["not_done"]), w0p, w1p)
    assert ops.last_kernel() == "acoustic_mem_small"
    torch.cuda.synchronize()
    return {"out": out}


@pytest.mark.parametrize("row_id", _ids("mem"))
def test_acoustic_mem_small_matches_fp64(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp = R.inputs(row)
    B = row["B"]
    w0p, w1p = (ops.pack_conv_weight_ex(_d(inp[k]), 32, 32) for k in ("w0", "w1"))       # as memory_nets.py packs them (_PackMemo.get(w, 32))
    assert tuple(w0p.shape) == (32, 288) and tuple(w1p.shape) == (16, 288)
    got, again = _run_mem(inp, w0p, w1p), _run_mem(inp, w0p, w1p)
    _check_row("mem", row, "%d workgroups" % (B * 32 // R.MEM_R), got, R.reference(row, inp), again)
    for b in sorted({0, B - 1}):        # image b of the batch == the same image alone
        one = {k: (v[b:b + 1] if k in ("pred_mono", "prev_mem") or (k == "not_done" and v is not None) else v) for k, v in inp.items()}
        assert torch.equal(_run_mem(one, w0p, w1p)["out"][0], got["out"][b]), (row_id, b)
    if row["nd"] == "zero":             # a finished env's previous memory does not reach the output
        assert float(inp["prev_mem"].abs().sum()) > 0
        assert torch.equal(_run_mem(dict(inp, prev_mem=torch.zeros_like(inp["prev_mem"])), w0p, w1p)["out"], got["out"]), row_id


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_glue(row, inp):
    d = {k: _d(v) for k, v in inp.items()}
    if row["kernel"] == "visual_input":
        out = ops.visual_input(d["rgb"], d["depth"])
    else:
        out = ops.slice_concat_input(d["a"], d["b"], mul=d["mul"], bscale=d["bscale"], op=row["op"])
    assert ops.last_kernel() == row["kernel"]
    torch.cuda.synchronize()
    return {"out": out}


@pytest.mark.parametrize("row_id", _ids("glue"))
def test_input_glue_matches_fp64(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp = R.inputs(row)
    got, again = _run_glue(row, inp), _run_glue(row, inp)
    ref = R.reference(row, inp)
    if row["kernel"] == "visual_input":     # bit-equal to the correctly rounded float32 rgb / 255, and to depth or 0
        assert got["out"].shape == (1, row["npix"], 1, 4) and np.array_equal(got["out"].cpu().numpy().astype(np.float64), ref["out"][0]), row_id
    else:
        assert tuple(got["out"].shape) == ref["out"][0].shape
    _check_row("glue", row, "%d items" % R.glue_total(row), got, ref, again,
               kind=row["kernel"] if row["kernel"] == "visual_input" else "slice op %d%s" % (row["op"], " bscale" if row["bscale"] else ""))


# ----------------------------------------------------------------------------------------------------------------------------------
def _rand(shape, dtype, g):
    return torch.randint(-2 ** 40, 2 ** 40, shape, generator=g) if dtype == "int64" else torch.randn(*shape, generator=g)


def _copy_gather(row, g):
    T, N, Lw = row["T"], row["N"], row["Lw"]
    per = Lw // 2 if row["dtype"] == "int64" else Lw
    src = _rand((T, N, per), row["dtype"], g)
    if row["nsel"]:
        perm = torch.randint(0, N, (row["nsel"],), generator=g)
    else:
        perm = {"one": torch.tensor([N - 1]), "all": torch.randperm(N, generator=g), "repeats": torch.cat((torch.randperm(N, generator=g), torch.tensor([0, N - 1, 0])))}[row["perm"]]
    want = src[:, perm].reshape(T * perm.numel(), per)
    for _ in range(2):
        got = ops.gather_envs(_d(src), _d(perm))
        assert ops.last_kernel() == "gather_envs"
        assert got.dtype == src.dtype and torch.equal(got.cpu(), want)


def _copy_rows_copy(row, g):
    dev = _dev()
    idx = torch.tensor([2, 3, 1], dtype=torch.int64)
    items, checks = [], []
    for i, (n, dt) in enumerate(R.ROWS_COPY_SHAPES[row["kind"]]):
        sentinel = -5 if dt == "int64" else -5.0
        if i % 3 == 0:          # row idx[0] of src -> row idx[1] of dst
            src, dst = _rand((4, n), dt, g), torch.full((6, n), sentinel, dtype=torch.int64 if dt == "int64" else torch.float32)
            want = dst.clone()
            want[3] = src[2]
            sd, dd = _d(src), _d(dst)
            items.append((sd, dd, 0, 1))
        elif i % 3 == 1:        # a whole tensor as the row -> row idx[2] of dst
            src, dst = _rand((n,), dt, g), torch.full((6, n), sentinel, dtype=torch.int64 if dt == "int64" else torch.float32)
            want = dst.clone()
            want[1] = src
            sd, dd = _d(src), _d(dst)
            items.append((sd, dd, -1, 2))
        else:                   # row idx[2] of src -> a row given by its own pointer, a guard row on each side
            src, dst = _rand((4, n), dt, g), torch.full((3, n), sentinel, dtype=torch.int64 if dt == "int64" else torch.float32)
            want = dst.clone()
            want[1] = src[1]
            sd, dd = _d(src), _d(dst)
            items.append((sd, dd[1], 2, -1))
        checks.append((dd, want))
    ops.rows_copy(items, idx.to(dev))
    assert ops.last_kernel() == "rows_copy"
    torch.cuda.synchronize()
    for i, (dd, want) in enumerate(checks):     # the written row, and every other row (its neighbours the guards) untouched
        assert torch.equal(dd.cpu(), want), (row["id"], i)


def _copy_env_step(row, g):
    inp = R.env_step_inputs(row)
    a, node, angle = (_d(inp[k].clone()) for k in ("actions", "node", "angle"))
    ops.synth_env_step(a, node, angle, row["n_nodes"])
    assert ops.last_kernel() == "synth_env_step"
    n1, a1 = R.synth_env_step_reference(inp["actions"].numpy(), inp["node"].numpy(), inp["angle"].numpy(), row["n_nodes"])
    assert np.array_equal(node.cpu().numpy(), n1) and np.array_equal(angle.cpu().numpy(), a1) and torch.equal(a.cpu(), inp["actions"])


def _copy_env_observe(row, g):
    N, n_nodes, n_audio = 5, 2, 3
    node, angle = torch.tensor([1, 0, 1, 1, 0]), torch.tensor([3, 0, 3, 2, 0])      # repeated frame rows (envs 0 and 2, 1 and 4)
    audio = torch.tensor([2, 2, 0, 1, 2])
    pools = [(_rand((n_nodes * 4 if kind == 0 else n_audio, n), dt, g), kind) for n, dt, kind in R.OBSERVE_POOLS[row["kind"]]]
    for _ in range(2):
        outs = ops.synth_env_observe([(_d(p), kind) for p, kind in pools], _d(node), _d(angle), _d(audio))
        assert ops.last_kernel() == "synth_env_observe"
        for (p, kind), o in zip(pools, outs):
            assert o.dtype == p.dtype and torch.equal(o.cpu(), p[node * 4 + angle] if kind == 0 else p[audio]), (row["id"], kind, tuple(p.shape))


def _copy_step_index(row, g):
    idx = _d(torch.tensor(row["idx"], dtype=torch.int64))
    seed, counter = 0x1234567890ABCDE, 2 ** 33 + 11
    rng = _d(torch.tensor([seed, counter], dtype=torch.int64)) if row["rng_inc"] is not None else None
    ops.step_index_advance(idx, row["T_pol"], row["T_sep"], rng=rng, rng_inc=row["rng_inc"] or 0)
    assert ops.last_kernel() == "step_index_advance"
    assert tuple(idx.cpu().tolist()) == R.step_index_reference(row)
    if rng is not None:         # the counter moved on, the seed word untouched
        assert rng.cpu().tolist() == [seed, counter + row["rng_inc"]]


@pytest.mark.parametrize("row_id", _ids("copy"))
def test_copies_and_counters_are_exact(row_id):
    row = R.ROWS_BY_ID[row_id]
    {"gather_envs": _copy_gather, "rows_copy": _copy_rows_copy, "synth_env_step": _copy_env_step, "synth_env_observe": _copy_env_observe,
     "step_index_advance": _copy_step_index}[row["kernel"]](row, R._gen(row_id))
    print("%-58s exact" % row_id)


# ----------------------------------------------------------------------------------------------------------------------------------
def test_zz_report_worst_ratios():
    """(summary of the rows above: worst |g - r| / s per family, kernel and output kind, for the record)"""
    for (family, kernel, name), v in sorted(WORST.items()):
        print("worst |g-r|/s  %-10s %-24s %-12s %.2e  (tau %.1e)" % (family, kernel, name, v, R.TAU[family]))
    assert _lib.ROWS_COPY_MAX == R.ROWS_COPY_MAX
