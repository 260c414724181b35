"""GPU: the training kernels beyond the convolutions -- csrc/bn.hip and the training units csrc/rnn.hip, policy_heads.hip, losses.hip and optim.hip (GRU step / cell / BPTT kernels, the
LSTM cell, the policy heads with their backward and weight gradient, the L1 / binaural / PPO losses, gradient clipping and Adam) -- on every
route and edge of tests/train_kernels.py's table, every output element against the float64 reference of the same float32 inputs:
|g_e - r_e| <= tau * s_e (elem_bound.bound; the scales and their one rule: tests/train_kernels.py, pinned on the CPU by
tests/test_train_kernels_cpu.py together with the mutants the bound must reject).  Every row also: all outputs finite, the library's label
of the launch where it names one, and bit-identical results on a second call.

Calibrated on an MI355X (worst |g - r| / s over each family's rows, per output kind; test_zz_report_worst_ratios prints them with -s):
  bn       y 2.2e-7, mean 5.5e-6, invstd 1.5e-7, running_mean 1.4e-7, running_var 9.8e-8, dgamma 4.9e-7, dbeta 3.0e-7, dz 2.4e-7
  gru      gru_gates 9.1e-8, gru_step 9.4e-7 (gh_raw) / 2.8e-7 (hout), gru_cell 3.5e-7, gru_gates_bwd 1.2e-6, gru_bwd_rec 5.8e-7,
           gru_bwd_step 6.3e-7 (the rewritten dhp; out 5.6e-7), gru_bwd_combine 7.4e-8
  gru_seq  out 6.5e-7, hT 6.3e-7, g_x 1.5e-6, g_h0 1.1e-6, g_whh 1.2e-5, g_wih 2.56e-5, g_bih / g_bhh 2.53e-5
  lstm     gates 2.8e-7, c / h 3.9e-7, dpre 2.1e-7, dcprev 6.9e-8
  heads    value 2.4e-7, logp_all 1.1e-7, probs 1.4e-7, entropy 5.0e-7, dz 1.0e-7, dfeats 2.7e-7, dw 1.3e-6, db 5.1e-7
  loss     l1 5.6e-8 / 5.9e-8 (loss / gradient), l1_nhwc16 1.5e-7 / 3.0e-8, bin_l1 2.0e-8 / 7.1e-8, ppo 2.8e-7 (sums), 1.1e-7 (gradients)
  adam     clip coefficient and norm 5.3e-8, p 1.4e-6, m 1.5e-7, v 2.6e-7, g 6.0e-8
Every family of single kernels keeps TAU_FP32 = 2e-5 (bn's mean is the one figure above TAU_FP32 / 6: the float32 rounding of a mean near 100
against sqrt(sum x^2) / M; it is under the constant for the rows' M <= 5000).  gru_seq has its own constant, 2e-4 = 8 x 2.56e-5: its outputs
are held against the scale of the step that makes them, without the error that step's inputs carry (tests/train_kernels.py TAU).
"""
import pytest
import torch

import m2h_oracle as O
import train_kernels as K
from m2h import _lib, functional as MF, ops

pytestmark = pytest.mark.gpu
WORST = {}
P = ops._ptr


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _d(t):
    return t.to(_dev()).contiguous() if t is not None else None


def _call(name, *args):
    """One C-ABI call on the current stream."""
    lib = _lib.load()
    with torch.cuda.device(_dev()):
        _lib.check(getattr(lib, "m2h_" + name)(*args, ops._stream(torch.empty(0, device=_dev()))), "m2h_" + name)


def _ids(family):
    return [r["id"] for r in K.ROWS[family]]


def _check_row(family, row, route, got, ref, again=None):
    """Every output of the row against (r, s); one printed line per row: route, worst ratio, scale - 1, rel-L1 (over the outputs)."""
    tau = K.TAU[family]
    line_w, line_s, line_l = 0.0, 0.0, 0.0
    fails = []
    for name, (r, s) in ref.items():
        if name not in got:
            continue
        g = got[name].detach().cpu()
        assert bool(torch.isfinite(g).all()), (row["id"], name, "not finite")
        lsq = K.bn_lsq(name, row["C"]) if family == "bn" else None
        worst, scale, ok = K.check(g.reshape(r.shape), r, s, tau, lsq)
        key = (family, row.get("kernel", row.get("kind", family)), name)
        WORST[key] = max(WORST.get(key, 0.0), worst)
        line_w, line_l = max(line_w, worst), max(line_l, O.rel_l1(g.double().reshape(r.shape), r) if float(r.abs().sum()) > 0 else 0.0)
        line_s = scale - 1.0 if abs(scale - 1.0) > abs(line_s) else line_s
        if not ok:
            fails.append((name, worst, scale))
        if again is not None:
            assert torch.equal(g, again[name].detach().cpu()), (row["id"], name, "second call differs")
    assert any(n in got for n in ref), row["id"]
    print("%-46s %-34s worst |g-r|/s %.2e  scale-1 %+.1e  rel-L1 %.1e" % (row["id"], route, line_w, line_s, line_l))
    assert not fails, (row["id"], fails)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_bn(row, inp):
    dev = _dev()
    M, C, slope = row["M"], row["C"], row["slope"]
    rt = K.bn_route(M, C, row["knob"])
    z, ga, be, dy, rm, rv = (_d(inp[k].clone()) for k in ("z", "gamma", "beta", "dy", "running_mean", "running_var"))
    y, dz = torch.empty_like(z), torch.empty_like(z)
    mean, invstd, dga, dbe = (torch.empty(C, device=dev) for _ in range(4))
    ws, _ = ops._workspace(_lib.load().m2h_bn_workspace_bytes(M, C), dev)
    ops.debug_set(37, row["knob"])
    try:
        _call("bn_train_fwd", P(z), P(ga), P(be), K.BN_EPS, K.BN_MOMENTUM, slope, P(rm), P(rv), P(mean), P(invstd), P(y), M, C, P(ws))
        assert ops.last_kernel() == rt["kernel"] % "fwd", (ops.last_kernel(), rt)
        _call("bn_train_bwd", P(dy), P(y), P(z), P(mean), P(invstd), P(ga), slope, P(dga), P(dbe), P(dz), M, C, P(ws))
        assert ops.last_kernel() == rt["kernel"] % "bwd", (ops.last_kernel(), rt)
    finally:
        ops.debug_set(37, 0)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dgamma=dga, dbeta=dbe, dz=dz)


@pytest.mark.parametrize("row_id", _ids("bn"))
def test_bn_matches_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.bn_inputs(row)
    got, again = _run_bn(row, inp), _run_bn(row, inp)
    rt = K.bn_route(row["M"], row["C"], row["knob"])
    route = "%s R=%d splits=%d rps=%d empty=%d" % (rt["label"], rt["R"], rt["splits"], rt["rps"], rt["empty"])
    ref = K.bn_reference(row, inp, {k: got[k].cpu() for k in ("y", "mean", "invstd")})
    _check_row("bn", row, route, got, ref, again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_gru(row, inp):
    dev = _dev()
    k, M, H = row["kernel"], row["M"], row["H"]
    d = {n: _d(v) if torch.is_tensor(v) else v for n, v in inp.items()}
    e = lambda *s: torch.empty(*s, device=dev)
    if k == "gru_gates":
        out = {"hout": ops.gru_gates(d["gi"], d["gh"], d["bhh"], d["hprev"], d["mask"])}
    elif k == "gru_step":
        hout, gh = ops.gru_step(d["gi"], d["whh"], d["bhh"], d["hprev"], d["mask"])
        out = {"hout": hout, "gh_raw": gh}
    elif k == "gru_cell":
        out = {"hout": ops.gru_cell(d["x"], d["wih"], d["bih"], d["whh"], d["bhh"], d["hprev"], d["mask"])}
    elif k == "gru_gates_bwd":
        dgi, dpre, dhp, hpm = e(M, 3 * H), e(M, 3 * H), e(M, H), e(M, H)
        _call(k, P(d["gi"]), P(d["gh"]), P(d["bhh"]), P(d["hprev"]), P(d["mask"]), P(d["dh"]), P(dgi), P(dpre), P(dhp), P(hpm), M, H)
        out = dict(dgi=dgi, dpre=dpre, dhp=dhp, hpm=hpm)
    elif k == "gru_bwd_combine":
        o = e(M, H)
        _call(k, P(d["a"]), P(d["rec"]), P(d["dhp"]), P(d["mask"]), P(o), M, H)
        out = {"out": o}
    else:
        whh_t = d["whh"].t().contiguous()           # W_hh^T as an [H][3H] row-major matrix: the recurrent input-gradient product's weight
        o, dhp = e(M, H), d["dhp"].clone()
        if k == "gru_bwd_rec":
            _call(k, P(d["dpre"]), P(whh_t), P(d["a"]), P(dhp), P(d["mask"]), P(o), M, H)
            assert torch.equal(dhp, d["dhp"])       # (read only without the epilogue)
            out = {"out": o}
        else:
            dgi, dpre, hpm = e(M, 3 * H), e(M, 3 * H), e(M, H)
            _call(k, P(d["dpre"]), P(whh_t), P(d["a"]), P(dhp), P(d["mask"]), P(o), P(d["gi"]), P(d["gh"]), P(d["bhh"]), P(d["hprev_p"]),
                  P(d["mask_p"]), P(dgi), P(dpre), P(hpm), M, H)
            out = dict(out=o, dgi_p=dgi, dpre_p=dpre, dhp_new=dhp, hpm_p=hpm)
    assert ops.last_kernel() == k, (ops.last_kernel(), k)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("row_id", _ids("gru"))
def test_gru_kernels_match_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.gru_inputs(row)
    got, again = _run_gru(row, inp), _run_gru(row, inp)
    _check_row("gru", row, row["kernel"], got, K.gru_reference(row, inp), again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_seq(row, inp):
    d = {n: _d(v) for n, v in inp.items()}
    leaves = [d[n].requires_grad_(True) for n in ("x", "h0", "w_ih", "w_hh", "b_ih", "b_hh")]
    out, hT = MF.GRUSequence.apply(leaves[0], leaves[1], d["masks"], leaves[2], leaves[3], leaves[4], leaves[5], row["T"])
    fused = K.gru_route(row["N"], row["H"], row["T"])["fused"]
    assert ops.last_kernel() == ("gru_step" if fused else "gru_gates"), (ops.last_kernel(), fused)
    outs, gouts = ([out, hT], [d["g_out"], d["g_hT"]]) if row["ghT"] else ([out], [d["g_out"]])
    gs = torch.autograd.grad(outs, leaves, gouts)
    torch.cuda.synchronize()
    return dict(out=out.detach(), hT=hT.detach(), g_x=gs[0], g_h0=gs[1], g_wih=gs[2], g_whh=gs[3], g_bih=gs[4], g_bhh=gs[5])


@pytest.mark.parametrize("row_id", _ids("gru_seq"))
def test_gru_sequence_matches_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.seq_inputs(row)
    got, again = _run_seq(row, inp), _run_seq(row, inp)
    rt = K.gru_route(row["N"], row["H"], row["T"])
    _check_row("gru_seq", row, "%s; %s" % (rt["forward"], " ".join(rt["backward"])), got, K.seq_reference(row, inp), again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_lstm(row, inp):
    dev = _dev()
    M, H = row["M"], row["H"]
    d = {n: _d(v) for n, v in inp.items()}
    h, c, gates = (torch.empty(M, H, device=dev), torch.empty(M, H, device=dev), torch.empty(M, 4 * H, device=dev))
    _call("lstm_cell", P(d["gi"]), P(d["gh"]), P(d["cprev"]), P(d["mask"]), P(h), P(c), P(gates), M, H)
    assert ops.last_kernel() == "lstm_cell"
    dpre, dcp = torch.empty(M, 4 * H, device=dev), torch.empty(M, H, device=dev)
    _call("lstm_cell_bwd", P(d["dh"]), P(d["dc"]), P(gates), P(d["cprev"]), P(d["mask"]), P(c), P(dpre), P(dcp), M, H)
    assert ops.last_kernel() == "lstm_cell_bwd"
    torch.cuda.synchronize()
    return dict(h=h, c=c, gates=gates, dpre=dpre, dcprev=dcp)


@pytest.mark.parametrize("row_id", _ids("lstm"))
def test_lstm_cell_matches_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.lstm_inputs(row)
    got, again = _run_lstm(row, inp), _run_lstm(row, inp)
    ref = K.lstm_reference(row, inp, {k: got[k].cpu() for k in ("gates", "c")})
    _check_row("lstm", row, "lstm_cell + lstm_cell_bwd", got, ref, again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _heads_wgrad(feats, dz, H, ZS):
    M = feats.shape[0]
    if K.heads_route(H, ZS - 1)["wgrad"] == "policy_heads_wgrad":
        dw, db = torch.empty(ZS, H, device=feats.device), torch.empty(ZS, device=feats.device)
        _call("policy_heads_wgrad", P(feats), P(dz), P(dw), P(db), M, H, ZS)
        assert ops.last_kernel() == "policy_heads_wgrad"
        return dw, db
    # the tiled weight-gradient engine + the bias-gradient kernel, as functional.PolicyHeads.backward takes them
    return MF.conv_wgrad(feats.reshape(M, 1, 1, H), None, dz.view(M, 1, 1, ZS), ZS, 1, 1, 1, 0).view(ZS, H), MF.bias_grad(dz)


def _run_heads(row, inp, flat):
    dev = _dev()
    M, H = row["M"], row["H"]
    if row["kind"] == "wgrad":
        dw, db = _heads_wgrad(_d(inp["feats"]), _d(inp["dz"]), H, row["ZS"])
        torch.cuda.synchronize()
        return dict(dw=dw, db=db)
    A = row["A"]
    ZS = K.heads_route(H, A)["ZS"]
    d = {n: _d(v) for n, v in inp.items()}
    if flat:        # Wa, ba, Wc, bc back to back in one buffer, as FlatAdam lays them out: Wc starts A H + A floats in (dword-aligned only unless A % 4 == 0)
        buf = torch.empty(A * H + A + H + 1, device=dev)
        o = 0
        for n in ("Wa", "ba", "Wc", "bc"):
            k = d[n].numel()
            buf[o:o + k].copy_(d[n].reshape(-1))
            d[n] = buf[o:o + k].view(d[n].shape)
            o += k
        assert (d["Wc"].data_ptr() - buf.data_ptr()) % 16 == (4 * (A * H + A)) % 16 and buf.data_ptr() % 16 == 0
    value, logp_all, probs, ent, logp_act = ops.policy_heads(d["feats"], d["Wa"], d["ba"], d["Wc"], d["bc"], d["actions"])
    assert ops.last_kernel() == "policy_heads"
    dz, dfeats = torch.empty(M, ZS, device=dev), torch.empty(M, H, device=dev)
    _call("policy_heads_bwd", P(logp_all), P(probs), P(d["actions"]), P(d["g_value"]), P(d["g_logp"]), P(d["g_ent"]), P(d["Wa"]), P(d["Wc"]),
          P(dz), P(dfeats), M, H, A, ZS)
    assert ops.last_kernel() == "policy_heads_bwd"
    dw, db = _heads_wgrad(d["feats"], dz, H, ZS)
    torch.cuda.synchronize()
    out = dict(value=value, logp_all=logp_all, probs=probs, entropy=ent, dz=dz, dfeats=dfeats, dw=dw, db=db)
    if logp_act is not None:
        out["logp_act"] = logp_act
    return out


@pytest.mark.parametrize("row_id", _ids("heads"))
def test_policy_heads_match_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.heads_inputs(row)
    got, again = _run_heads(row, inp, False), _run_heads(row, inp, True)     # separately allocated weights, then views into one flat buffer:
    if row["kind"] == "wgrad":                                                # bit for bit the same (and the second call of the row)
        route = "policy_heads_wgrad<%d>" % row["ZS"]
        ref = K.heads_reference(row, inp, None)
    else:
        rt = K.heads_route(row["H"], row["A"])
        route = "%s, ZS=%d, %s" % (rt["load"], rt["ZS"], rt["wgrad"])
        ref = K.heads_reference(row, inp, {k: got[k].cpu() for k in ("logp_all", "probs", "dz")})
    _check_row("heads", row, route, got, ref, again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _run_loss(row, inp):
    dev = _dev()
    k = row["kernel"]
    d = {n: _d(v) for n, v in inp.items()}
    if k == "l1_loss":
        loss, grad, scratch = torch.empty(1, device=dev), torch.empty_like(d["pred"]), torch.empty(1024, device=dev)
        _call(k, P(d["pred"]), P(d["gt"]), row["stride"], row["off"], P(loss), P(grad), P(scratch), row["n"])
        out = dict(loss=loss[0], grad=grad)
    elif k == "l1_loss_nhwc16":
        loss, grad = ops.l1_loss_nhwc16(d["y"], d["gt"], row["off"], want_grad=True)
        out = dict(loss=loss, grad=grad)
    elif k == "bin_l1_loss":
        loss, grad = ops.bin_l1_loss(d["mix"], d["masks"], d["gt"], cstep=row["cstep"], want_grad=True)
        out = dict(loss=loss, grad=grad)
    else:
        o, gv, gl = ops.ppo_loss(d["values"], d["logp"], d["old_values"], d["returns"], d["adv"], d["old_logp"], K.PPO_CLIP, K.PPO_VCOEF,
                                 row["clipped"], True, d["entropy"], K.PPO_ECOEF)
        out = dict(out=o, g_values=gv, g_logp=gl)
    assert ops.last_kernel() == k, (ops.last_kernel(), k)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("row_id", _ids("loss"))
def test_losses_match_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.loss_inputs(row)
    got, again = _run_loss(row, inp), _run_loss(row, inp)
    ref = K.loss_reference(row, inp, {n: v.cpu() for n, v in got.items()})
    _check_row("loss", row, ", ".join(sorted(c[1] for c in K.loss_cells(row))), got, ref, again)


# ----------------------------------------------------------------------------------------------------------------------------------
def _adam_steps(row, inp, dev_entry):
    """ADAM_STEPS steps of clip + Adam from m = v = 0; -> per step the state before, the clip coefficient and the state after (CPU tensors)."""
    dev = _dev()
    n = row["n"]
    p, m, v = _d(inp["p"].clone()), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    coef, scratch, hyper = torch.empty(2, device=dev), torch.empty(1024, device=dev), torch.zeros(4, device=dev)
    steps = []
    for step in range(1, K.ADAM_STEPS + 1):
        g = _d(inp["grads"][step - 1].clone())
        before = [t.cpu() for t in (p, g, m, v)]
        _call("grad_clip_coef", P(g), n, row["max_norm"], P(coef), P(scratch))
        assert ops.last_kernel() == "grad_clip_coef"
        if dev_entry:
            _call("adam_hyper", K.ADAM_LR, K.ADAM_B1, K.ADAM_B2, step, P(hyper))
            _call("adam_step_dev", P(p), P(g), P(m), P(v), n, P(hyper), K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, P(coef), row["gscale"])
            assert ops.last_kernel() == "adam_step_dev"
        else:
            _call("adam_step", P(p), P(g), P(m), P(v), n, K.ADAM_LR, K.ADAM_B1, K.ADAM_B2, K.ADAM_EPS, step, P(coef), row["gscale"])
            assert ops.last_kernel() == "adam_step"
        torch.cuda.synchronize()
        steps.append((before, coef.cpu(), dict(p=p.cpu(), g=g.cpu(), m=m.cpu(), v=v.cpu())))
    return steps


@pytest.mark.parametrize("row_id", _ids("adam"))
def test_clip_and_adam_match_fp64(row_id):
    row = K.ROWS_BY_ID[row_id]
    inp = K.adam_inputs(row)
    host, devs = _adam_steps(row, inp, False), _adam_steps(row, inp, True)
    for step, ((before, coef, after), (_b, coef_d, after_d)) in enumerate(zip(host, devs), 1):
        assert torch.equal(coef, coef_d) and all(torch.equal(after[k], after_d[k]) for k in after), (row_id, step)   # m2h_adam_step == hyper + step_dev
        p, g, m, v = before
        sub = dict(row, id="%s.step%d" % (row_id, step))
        _check_row("adam", dict(sub, kernel="grad_clip_coef"), "sumsq + clip_coef", {"coef": coef}, K.clip_reference(row, g))
        _check_row("adam", dict(sub, kernel="adam_step"), "adam_step == adam_hyper + adam_step_dev", after, K.adam_reference(row, step, p, g, m, v, coef[0]))
        if step == 1 and row["n"] > 1:
            assert bool(((g == 0) & (after["v"] == 0)).any())      # elements with g = 0 and v at zero


# ----------------------------------------------------------------------------------------------------------------------------------
def test_zz_report_worst_ratios():
    """(summary of the rows above: worst |g - r| / s per family, kernel and output kind, for the record)"""
    for (family, kernel, name), v in sorted(WORST.items()):
        print("worst |g-r|/s  %-8s %-18s %-14s %.2e  (tau %.1e)" % (family, kernel, name, v, K.TAU[family]))
