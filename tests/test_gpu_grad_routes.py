"""GPU: every weight-gradient route of csrc/conv_bwd.hip's dispatch (the tiled kernel of wgrad_tiled.hip: six block shapes x four split classes, the reduce / re-layout epilogues, the
shipped layer shapes of the passive step and of update_pol's encoders) and the input / bias gradients at the same shapes, element by
element against CPU float64 autograd from the same fp32 inputs.

Metric: |g_e - r_e| <= tau * s_e with s_e = sqrt(sum_m t_m^2) over the products t_m summed into element e (a weight gradient's s is
sqrt(wgrad(x^2, dy^2)): one more fp64 pass on squared operands).  s does not shrink when the terms cancel and it is the size of a
summation error, so one split's rows, a scale of (1 - 1/S) or one tap column cannot hide in it; each row with S > 1 checks on the host
that the bound rejects those three changes to the fp64 reference.  Also: the least-squares scale <g, r> / <r, r> = 1 +- tau and rel-L1.
The rows and the restated dispatch that names their routes are tests/grad_routes.py (tests/test_grad_routes_cpu.py pins them)."""
import zlib

import pytest
import torch
import torch.nn.functional as F

import grad_routes as G
import m2h_oracle as O
from elem_bound import TAU_BF16X3, TAU_FP32, bound   # (the bound and its constants: shared with the forward route test)
from m2h import functional as MF, ops

pytestmark = pytest.mark.gpu

# Calibrated on an MI355X (worst |g - r| / s over the whole table, printed per row with -s; test_zz_report_worst_ratios sums it up):
# fp32 weight gradients 2.2e-6, fp32 input gradients 3.5e-6, bias gradients 6.1e-7, bf16x3 input gradients 3.0e-5 (products carry ~16
# mantissa bits).  The bounds sit 6-10x above; one split's rows, a (1 - 1/S) scale or a tap column move the ratio by 1e-3 or more.
MODES = {"fp32": ops.MATH_FP32, "bf16x3": ops.MATH_BF16X3}
WORST = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).cpu()


def _check(name, row, mode, g, r, s, tau):
    worst, scale, ok = bound(g, r, s, tau)
    key = (name, mode)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("%-20s %-6s %-8s S=%-4s worst |g-r|/s %.2e  scale-1 %+.1e  rel-L1 %.1e" % (row["id"], mode, name, G.route(row)["S"], worst,
                                                                                      scale - 1.0, O.rel_l1(g.double().cpu(), r)))
    assert ok, (row["id"], mode, name, worst, scale)
    assert O.rel_l1(g.double().cpu(), r) < 5 * tau, (row["id"], mode, name)   # (measured: 3.4e-7 fp32, 4.5e-6 bf16x3)


def _seed(row):
    return zlib.crc32(row["id"].encode())


def _data(row):
    """fp32 inputs (NCHW), weight, bias and output gradient of a row, from the row's own seed."""
    g = torch.Generator().manual_seed(_seed(row))
    op, B, H, W, C0, C1, Co, k = (row[f] for f in ("op", "B", "H", "W", "C0", "C1", "Co", "k"))
    x = torch.randn(B, C0, H, W, generator=g)
    x2 = torch.randn(B, C1, H, W, generator=g) if C1 else None
    if op == "convT":
        w = torch.randn(C0 + C1, Co, 4, 4, generator=g) * (1.0 / (C0 + C1)) ** 0.5
        out_shape = (B, Co, 2 * H, 2 * W)
    else:
        ci = row.get("ci", C0 + C1)
        w = torch.randn(Co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        Ho, Wo = (H + 2 * row["p"] - k) // row["s"] + 1, (W + 2 * row["p"] - k) // row["s"] + 1
        out_shape = (B, Co, Ho, Wo)
    b = torch.randn(Co, generator=g) * 0.1 if row["bias"] else None
    gy = torch.randn(out_shape, generator=g)
    return x, x2, w, b, gy


def _fwd64(row):
    """The row's operation in float64 (no bias, no activation: the gate is applied to the output gradient)."""
    if row["op"] == "convT":
        return lambda xx, ww: F.conv_transpose2d(xx, ww, None, 2, 1)
    ci = row.get("ci", row["C0"] + row["C1"])
    return lambda xx, ww: F.conv2d(xx[:, :ci], ww, None, row["s"], row["p"])


def _grads64(f, x, w, dz):
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    gx, gw = torch.autograd.grad(f(xr, wr), (xr, wr), dz)
    xs, ws = (x.double() ** 2).requires_grad_(True), (w.double() ** 2).requires_grad_(True)
    sx, sw = torch.autograd.grad(f(xs, ws), (xs, ws), dz * dz)
    return gx, gw, sx.sqrt(), sw.sqrt()


def _packed(t4):
    """torch layout [N][C][KH][KW] -> the packed [N][(tap, channel)] layout of m2h_conv_wgrad_f32."""
    return t4.permute(0, 2, 3, 1).reshape(t4.shape[0], -1)


def _mutants(row, f, x, w, dz, r_w):
    """The fp64 reference after each of three changes the bound must reject: one split's rows removed (the last split, with the ragged tail:
    chunks [c0, c1) of wgrad_tiled.hip's split map), the gradient scaled by (1 - 1/S), the largest tap column zeroed."""
    rt = G.route(row)
    S, M = rt["S"], rt["M"]
    chunks = G.cdiv(M, G.WM)
    j = S - 1
    m0, m1 = chunks * j // S * G.WM, min(chunks * (j + 1) // S * G.WM, M)
    keep = torch.zeros(M, dtype=torch.float64)
    keep[m0:m1] = 1.0
    if rt["quad"]:          # phase (0, 0) of the transposed conv: its row m = (b, q, r) is output pixel (b, 2q, 2r)
        mask = torch.zeros(dz.shape[0], 1, dz.shape[2], dz.shape[3], dtype=torch.float64)
        mask[:, :, 0::2, 0::2] = keep.view(dz.shape[0], 1, dz.shape[2] // 2, dz.shape[3] // 2)
    else:
        mask = keep.view(dz.shape[0], 1, dz.shape[2], dz.shape[3])
    wr = w.double().requires_grad_(True)
    (part,) = torch.autograd.grad(f(x.double(), wr), (wr,), dz * mask)
    no_split = r_w - part
    taps = r_w.abs().sum((0, 1))
    t = int(taps.reshape(-1).argmax())
    no_tap = r_w.clone()
    no_tap[:, :, t // taps.shape[1], t % taps.shape[1]] = 0
    return {"split %d removed" % j: no_split, "scaled by 1-1/S": r_w * (1.0 - 1.0 / S), "tap column %d zeroed" % t: no_tap}


def _run_row(row, mode):
    dev = _dev()
    x, x2, w, b, gy = _data(row)
    op, slope, knobs = row["op"], row["slope"], row["knobs"]
    for kn, v in knobs.items():
        ops.debug_set(kn, v)
    try:
        with ops.math_scope(mode):
            if op == "wgrad":
                gw = MF.conv_wgrad(_nhwc(x, dev), _nhwc(x2, dev) if x2 is not None else None, _nhwc(gy, dev), row["Co"], row["k"], row["k"],
                                   row["s"], row["p"])
                torch.cuda.synchronize()
                return dict(gw=gw.cpu(), gate=None)
            xd = _nhwc(x, dev).requires_grad_(row["dx"])
            x2d = _nhwc(x2, dev).requires_grad_(True) if x2 is not None else None
            wd = w.to(dev).requires_grad_(True)
            bd = b.to(dev).requires_grad_(True) if b is not None else None
            if op == "convT":
                y = MF.conv_transpose2d(xd, wd, x2d)
            elif op == "linear":
                y = MF.linear(xd.view(row["B"], row["C0"]), wd.view(row["Co"], row["C0"]), bd, slope=slope)
                y = y.view(row["B"], 1, 1, row["Co"])
            else:
                y = MF.conv2d(xd, wd, bd, row["s"], row["p"], slope=slope)
            y.backward(_nhwc(gy, dev))
            torch.cuda.synchronize()
            return dict(gw=wd.grad.cpu(), gb=bd.grad.cpu() if bd is not None else None, gx=_nchw(xd.grad) if row["dx"] else None,
                        gx2=_nchw(x2d.grad) if x2d is not None else None, gate=_nchw(y) if slope != 1.0 else None)
    finally:
        for kn in knobs:
            ops.debug_set(kn, 0)


def _cases():
    out = []
    for row in G.ROWS:
        for name, mode in MODES.items():
            if name == "bf16x3" and (row["op"] == "wgrad" or not row["dx"]):
                continue      # no input gradient: the weight gradient's arithmetic is fp32 in every mode
            out.append(pytest.param(row["id"], name, id="%s-%s" % (row["id"], name)))
    return out


@pytest.mark.parametrize("row_id,mode", _cases())
def test_gradients_match_fp64(row_id, mode):
    row = G.ROWS_BY_ID[row_id]
    got = _run_row(row, MODES[mode])
    x, x2, w, b, gy = _data(row)
    dz = gy.double()
    if got["gate"] is not None:       # the activation's derivative from the GPU's own forward output (a gate near 0 cannot flip)
        dz = dz * torch.where(got["gate"] > 0, 1.0, row["slope"]).double()
    f = _fwd64(row)
    xin = x if x2 is None else torch.cat((x, x2), 1)
    r_x, r_w, s_x, s_w = _grads64(f, xin, w, dz)
    tau_x = TAU_FP32 if mode == "fp32" else TAU_BF16X3
    if row["op"] == "wgrad":
        _check("wgrad", row, mode, got["gw"], _packed(r_w), _packed(s_w), TAU_FP32)
    else:
        _check("wgrad", row, mode, got["gw"].view(r_w.shape), r_w, s_w, TAU_FP32)
        if got.get("gb") is not None:
            _check("bgrad", row, mode, got["gb"], dz.sum((0, 2, 3)), (dz * dz).sum((0, 2, 3)).sqrt(), TAU_FP32)
        if got.get("gx") is not None:
            C0 = row["C0"]
            _check("dgrad", row, mode, got["gx"], r_x[:, :C0], s_x[:, :C0], tau_x)
            if got.get("gx2") is not None:
                _check("dgrad.src1", row, mode, got["gx2"], r_x[:, C0:], s_x[:, C0:], tau_x)
    # sensitivity: the bound rejects the reference after each change (rows whose launch splits the reduction)
    if G.route(row)["S"] > 1 and mode == "fp32":
        for what, mut in _mutants(row, f, xin, w, dz, r_w).items():
            assert not bound(mut, r_w, s_w, TAU_FP32)[2], (row["id"], what)


@pytest.mark.parametrize("M,N,slope", G.BIAS_ROWS)
def test_bias_gradient_matches_fp64(M, N, slope):
    """m2h_bias_grad / m2h_act_bwd_bias: one stage (M <= 1024) and two (partials + ordered final), the narrow partial kernel (N divides 64)
    and the generic one (N does not), against the fp64 column sums; the gated output gradient is the exact fp32 select."""
    dev = _dev()
    g = torch.Generator().manual_seed(M * 131 + N)
    dy = torch.randn(M, N, generator=g)
    y = torch.randn(M, N, generator=g)
    if slope == 1.0:
        db = MF.bias_grad(dy.to(dev)).cpu()
        dz = dy
    else:
        out, db = MF.act_bwd_bias(dy.to(dev), y.to(dev), slope)
        dz = torch.where(y > 0, dy, dy * slope)
        assert torch.equal(out.cpu(), dz)
        db = db.cpu()
    r, s = dz.double().sum(0), (dz.double() ** 2).sum(0).sqrt()
    worst, scale, ok = bound(db, r, s, TAU_FP32)
    print("bias M=%-6d N=%-4d slope %.1f  worst |g-r|/s %.2e" % (M, N, slope, worst))
    assert ok, (worst, scale)
    # sensitivity: one row block of the two-stage split missing, or one column zeroed, is rejected
    assert not bound(r - dz[: max(1, M // 64)].double().sum(0), r, s, TAU_FP32)[2]
    r0 = r.clone()
    r0[N // 2] = 0
    assert not bound(r0, r, s, TAU_FP32)[2]


def test_zz_report_worst_ratios():
    """(summary of the table above: worst |g - r| / s per gradient kind and arithmetic, for the record)"""
    for (name, mode), v in sorted(WORST.items()):
        print("worst |g-r|/s  %-10s %-6s %.2e" % (name, mode, v))
