"""GPU: the image-row 3x3 kernels of update_sep (csrc/wgrad_row3x3.hip, csrc/conv_row3x3.hip) on every row of tests/row3x3_kernels.py's tables
through the public entry points (functional.conv_wgrad, functional.conv_wgrad_dgrad_fused, ops.conv2d_nhwc, functional.conv_dgrad,
ops.conv3x3_l1_nhwc16; the ldc > N rows through forward_routes.run_on, the one way to a strided destination), element by element against
float64 (rows, cells, references, taus, mutants: tests/row3x3_kernels.py, pinned on the CPU by tests/test_row3x3_kernels_cpu.py).
Per row: the outputs (and the workspace) are NaN before the call, so every element must be written; the label and the launch count are
asserted; |g - r| <= tau s on EVERY element, least-squares scale included (row3x3_kernels.check); two runs give the same bits.
  weight gradient   the label is the ordered reduce's and does not tell the image-row kernels from the tiled one: the route is stated by the
                    restated wgrad_row3x3_rule (held against the source on the CPU), and every row runs once more with knob 21 = -1 -- the
                    tiled kernel at the same shape and workspace -- under the same float64 bound; nothing is asserted between the two runs.
                    A gated row must also be bit-identical to act_bwd followed by the ungated call (its tiled run takes act_bwd's output: the
                    tiled kernel has no gate).  The fused kernel has no tiled form (its entry refuses every other route), so no second run.
  forward / dgrad   every image of every row, the multi-round rows included; an ldc > N row leaves everything outside its column block
                    unchanged bit for bit; bf16x3 with C0 = 16 and N <= 16 is asserted NOT to carry the engine's label (and holds the bound)
  L1                the loss within tau s, the gradient exact on every unflagged element and in {-inv, 0, +inv} on all, flagged share under
                    its cap.  y = g exactly cannot be planted (y is never stored): the gradient's 0 is admitted, never demanded.
That this file fails with any one named mutant in the kernel follows from the CPU margins (each >= 4 tau on the rows named for it, against
kernel ratios below): a mutant moves an element by its margin, the kernel's own error is under 1 tau.

Measured on an MI355X (test_zz_report prints them with -s): worst |g - r| / s in units of the row's tau, each held under 1
  kernel                              arithmetic   worst      worst row                         CPU stand-in
  wgrad3x3_row_kernel<16>             fp32         0.055      wg.fp32.n16.b3h7.k1.g0.2.t32      0.112
  wgrad3x3_row_kernel<32>             fp32         0.062      wg.fp32.n32.b3h7.k1.g0.2.t32      0.100
  wgrad3x3_row_bf16x3_kernel<16>      bf16x3       0.110      wg.x3.n12.b5h2.ld36.t32           0.111
  wgrad3x3_row_bf16x3_kernel<32>      bf16x3       0.108      wg.x3.n28.b5h2.ld48.t32           0.108
  wgrad3x3_row_dgrad_bf16x3_kernel    bf16x3       0.031      wg.fused.n32.b1h1.g0.t32          0.031   (0.004 at B 3, H 32: the bound's same-sign term grows with n)
  the same, second scale s_rms        bf16x3       0.073      wg.fused.n32.b3h32.g0.2.t29       0.069   (0.056 - 0.073 on every fused row)
  the tiled kernel at the same shapes fp32 / x3    0.219 / 0.017   wg.*.n32.b3h7.k1.g0.2.t32             (bf16x3 mode does not reach the tiled kernel: fp32 products)
  conv3x3_row_kernel, forward         fp32         0.175      fwd.fp32.n32c32.b65h32.deslice    0.130   (per instantiation 0.112 - 0.175)
  conv3x3_row_kernel, mirrored taps   fp32         0.196      dgrad.fp32.n16c32.b103h20         0.173   (0.122 - 0.196)
  conv3x3_row_bf16x3_kernel, forward  bf16x3       0.132      fwd.x3.n32c32.b512h4.deslice      0.132   (0.114 - 0.132)
  conv3x3_row_bf16x3_kernel, mirrored bf16x3       0.128      dgrad.x3.n32c16.b769h4            0.128   (0.111 - 0.128)
  fused L1, loss                      fp32 / x3    0.0025 / 0.0007  l1.fp32.b65 / l1.x3.b97       0.0025 / 0.0006
Multi-round rows sit with the one-round rows (two rounds 0.111 - 0.196, three rounds 0.161).  L1: no unflagged gradient element wrong and none
outside {-inv, 0, +inv}; flagged share 7.5e-6 - 8.8e-6 (fp32, cap 5e-5) and 5.3e-5 - 6.5e-5 (bf16x3, cap 5e-4); signs that differ from the
reference's over all elements: none in fp32, 0 / 9.4e-7 / 1.3e-6 in bf16x3 (B = 64 / 65 / 97).  bf16x3 with 16 -> 16 and 16 -> 12 channels carries
the label igemm_f32<128,16> (0.010 tau).  Every bit-identity held: two runs of every row, every gated row against act_bwd + the ungated call.
No row found a kernel defect.  The 106 tests of this file take 6.5 s on an MI355X (6.9 s with -s; the slowest, 0.35 s, is the first launch of the process).
"""
import contextlib
from unittest import mock

import pytest
import torch

import forward_routes as FRT
import row3x3_kernels as K
from m2h import _lib, functional as MF, ops

pytestmark = pytest.mark.gpu
WORST = {}
SENTINEL = -12345.678


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@contextlib.contextmanager
def _nan_outputs():
    """Inside the block every floating-point torch.empty is NaN: the ops allocate their outputs (and workspaces) with it, so an element the
    kernel does not write stays NaN."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    with mock.patch.object(torch, "empty", empty):
        yield


@contextlib.contextmanager
def _mode(math, knobs=None):
    knobs = knobs or {}
    for kn, v in knobs.items():
        ops.debug_set(kn, v)
    try:
        with ops.math_scope(ops.MATH_BF16X3 if math == "x3" else ops.MATH_FP32):
            yield
    finally:
        for kn in knobs:
            ops.debug_set(kn, 0)


def _counted(fn, launches, label):
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    with _nan_outputs():
        out = fn()
    assert lib.m2h_launch_count() - n0 == launches and ops.last_kernel() == label, (lib.m2h_launch_count() - n0, ops.last_kernel(), label)
    return out


def _record(name, kernel, math, g, ref):
    worst, scale, ok = K.check(g, ref)
    print("%-44s %-22s %-5s worst %.3f tau (tau %.0e)  scale-1 %+.1e" % (name, kernel, math, worst, ref["tau"], scale - 1.0))
    WORST[(kernel, math)] = max(WORST.get((kernel, math), (0.0, "")), (worst, name))
    assert ok, (name, kernel, worst, scale)


# ---------------------------------------------------------------------------------------------------------------------------------
# Weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad(row, x, dy, gate, knob21=0):
    knobs = {K.KNOB_WG_ROW: knob21}
    if row["knob11"]:
        knobs[K.KNOB_BLOCKS] = row["knob11"]
    with _mode(row["math"], knobs):
        return _counted(lambda: MF.conv_wgrad(x, None, dy, row["N"], 3, 3, 1, 1, gate=gate, gate_slope=1.0 if gate is None else row["gate"], torch_ci=row["ci"]),
                        2, K.WG_LABEL[row["ci"] is not None])


@pytest.mark.parametrize("name", [n for n, r in K.WG_ROWS.items() if not r["fused"]])
def test_weight_gradient_row_matches_fp64(name):
    row, dev = K.WG_ROWS[name], _dev()
    d = K.wg_data(row)
    ref = K.wg_reference(row, d)
    x, dy, gate = d["x"].to(dev), d["dy"].to(dev), None if d["gate"] is None else d["gate"].to(dev)
    assert K.wg_rule(row["N"], row["ldy"]) and not K.wg_rule(row["N"], row["ldy"], -1)
    out = _wgrad(row, x, dy, gate)
    assert out.shape == ref["r"].shape and not bool(torch.isnan(out).any()), (name, int(torch.isnan(out).sum()))     # every element written
    assert torch.equal(out, _wgrad(row, x, dy, gate)), name                                                          # two runs, the same bits
    _record(name, "wgrad3x3_row " + K.wg_kernel(row), row["math"], out.cpu(), ref)
    pre = dy
    if gate is not None:     # the gate folded into the load == act_bwd and the ungated call, bit for bit
        pre = MF.act_bwd(dy, gate, row["gate"])
        assert torch.equal(out, _wgrad(row, x, pre, None)), name
    tiled = _wgrad(row, x, pre, None, knob21=-1)
    assert not bool(torch.isnan(tiled).any()), name
    _record(name, "tiled at the same shape", row["math"], tiled.cpu(), ref)


@pytest.mark.parametrize("name", [n for n, r in K.WG_ROWS.items() if r["fused"]])
def test_fused_weight_gradient_row_matches_fp64(name):
    row, dev = K.WG_ROWS[name], _dev()
    d = K.wg_data(row)
    ref = K.wg_reference(row, d)
    x, dy2, gate = d["x"].to(dev), d["dy2"].to(dev), d["gate"].to(dev)
    w2p = ops.pack_conv_weight_ex(d["w2"].to(dev).contiguous(), 32, 32)

    def run():
        with _mode("x3", {K.KNOB_BLOCKS: row["knob11"]} if row["knob11"] else None):
            assert MF.conv_wgrad_dgrad_fused_supported(x)
            return _counted(lambda: MF.conv_wgrad_dgrad_fused(x, dy2, w2p, gate, row["gate"], row["ci"]), 2, K.WG_LABEL[True])

    out = run()
    assert out.shape == ref["r"].shape and not bool(torch.isnan(out).any()), (name, int(torch.isnan(out).sum()))
    assert torch.equal(out, run()), name
    _record(name, "wgrad3x3_row_dgrad", "x3", out.cpu(), ref)
    _record(name, "wgrad3x3_row_dgrad (s_rms)", "x3", out.cpu(), K.rms(ref))     # the second, tighter scale (row3x3_kernels.py's docstring)


# ---------------------------------------------------------------------------------------------------------------------------------
# Forward and input gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _forward(row, d, dev, label):
    """The row's launch into NaN (ldc: sentinel) memory; returns the output on the CPU in the reference's layout."""
    N, C0, B, H = (row[k] for k in ("N", "C0", "B", "H"))
    if row["ldc"]:
        ldc, c0 = row["ldc"], 8
        wide = torch.full((B * H * 32, ldc), SENTINEL, device=dev)
        fr_row = dict(id=row["id"], kind="c3", B=B, H=H, W=32, C0=C0, C1=0, N=N, math="bf16x3" if row["math"] == "x3" else "fp32", split=0)
        _, got_label, launches, wsb = FRT.run_on(fr_row, dev, d["x"], None, d["w"], None, None, dst=wide[:, c0:c0 + N], ldc=ldc)
        assert (got_label, launches, wsb) == (label, 1, 0)
        got = wide.cpu()
        outside = torch.ones(B * H * 32, ldc, dtype=torch.bool)
        outside[:, c0:c0 + N] = False
        assert bool((got.view(torch.int32)[outside] == torch.full((1,), SENTINEL).view(torch.int32)).all())       # bit for bit
        return got[:, c0:c0 + N].reshape(B, H, 32, N)
    x = d["x"].permute(0, 2, 3, 1).contiguous().to(dev)
    w = d["w"].to(dev).contiguous()
    with _mode(row["math"]):
        if row["dir"] == "fwd":
            wp = ops.pack_conv_weight_ex(w, C0, C0)
            bias = None if d["bias"] is None else d["bias"].to(dev)
            out = _counted(lambda: ops.conv2d_nhwc(x, wp, N, 3, 3, stride=1, pad=1, bias=bias, slope=row["slope"], deslice=row["deslice"]), 1, label)
        else:
            wp = MF.pack_dgrad_weight(w, 1, 1)
            out = _counted(lambda: MF.conv_dgrad(x, w, (H, 32), 1, 1, wp=wp), 1, label)
    return out.cpu()


@pytest.mark.parametrize("name", list(K.FW_ROWS_TABLE))
def test_forward_row_matches_fp64(name):
    row, dev = K.FW_ROWS_TABLE[name], _dev()
    d = K.fw_data(row)
    kernel = K.fw_kernel(row["math"], row["N"], row["C0"], row["B"], row["H"], row["deslice"])
    out = _forward(row, d, dev, K.FW_LABEL[row["math"]])
    ref = K.fw_reference(row, d)
    assert out.shape == ref["r"].shape and not bool(torch.isnan(out).any()), (name, int(torch.isnan(out).sum()))
    assert torch.equal(out, _forward(row, d, dev, K.FW_LABEL[row["math"]])), name
    _record(name, "conv3x3_row %s %s%s" % (row["dir"], kernel, ", %d rounds" % K.fw_rounds(row) if K.fw_rounds(row) > 1 else ""), row["math"], out, ref)


@pytest.mark.parametrize("name", list(K.OTHER_ROWS))
def test_bf16x3_16_to_16_channels_is_not_this_engines(name):
    row, dev = K.OTHER_ROWS[name], _dev()
    d = K.fw_data(row)
    x = d["x"].permute(0, 2, 3, 1).contiguous().to(dev)
    wp = ops.pack_conv_weight_ex(d["w"].to(dev).contiguous(), row["C0"], row["C0"])
    with _mode("x3"), _nan_outputs():
        out = ops.conv2d_nhwc(x, wp, row["N"], 3, 3, stride=1, pad=1)
        label = ops.last_kernel()
    assert "image-row" not in label, label
    _record(name, "other engine (%s)" % label, "x3", out.cpu(), K.fw_reference(row, d))


# ---------------------------------------------------------------------------------------------------------------------------------
# Fused L1
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.L1_ROWS))
def test_fused_l1_row_matches_fp64(name):
    row, dev = K.L1_ROWS[name], _dev()
    d = K.l1_data(row)
    ref = K.l1_reference(row, d)
    h, g = d["h"].to(dev), d["g"].to(dev)
    wp = ops.pack_conv_weight_ex(d["w"].to(dev).contiguous(), 32, 32)

    def run():
        with _mode(row["math"]):
            assert ops.conv3x3_l1_supported(h)
            return _counted(lambda: ops.conv3x3_l1_nhwc16(h, wp, g), 2, K.L1_LABEL[row["math"]])

    loss, grad = run()
    loss2, grad2 = run()
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2), name
    worst, wrong, outside, ok = K.l1_check(loss, grad, ref)
    differ = float((grad.cpu() != ref["grad"]).float().mean())
    print("%-44s loss worst %.4f tau  unflagged wrong %d  outside {-inv, 0, inv} %d  flagged share %.2e (cap %.0e)  signs that differ %.2e" % (
        name, worst, wrong, outside, ref["share"], K.FLAG_CAP[row["math"]], differ))
    WORST[("L1 loss", row["math"])] = max(WORST.get(("L1 loss", row["math"]), (0.0, "")), (worst, name))
    assert ref["share"] <= K.FLAG_CAP[row["math"]] and ok, (name, worst, wrong, outside, ref["share"])


def test_zz_report():
    """(summary of the runs above: the worst ratio per kernel and arithmetic)"""
    for (kernel, math), (worst, name) in sorted(WORST.items()):
        print("worst %-52s %-5s %.4f tau (%s)" % (kernel, math, worst, name))
