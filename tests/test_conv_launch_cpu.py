"""CPU: the launch forms of m2h/conv_launch.py.  (a) each form's struct against the route tables' own statement of the same launch
(forward_routes.conv_args, wgrad_routes.conv_args), field by field; (b) the input-gradient phases and (c) the two transposed forms, run
through the numpy model of the engine (tests/kernel_model.py), against float64 torch under the element bound of tests/elem_bound.py (the
model sums fp32 products: TAU_FP32, scales from the products); (d) the workspace helper."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import forward_routes as FR
import kernel_model as KM
import wgrad_routes as WR
from elem_bound import TAU_FP32, bound
from m2h import _lib, conv_launch

POINTERS = {n for n, t in _lib.ConvArgs._fields_ if t is ctypes.c_void_p}
# what wgrad_routes.conv_args leaves to its runner: the weight-gradient entries read the geometry only (include/m2h.h), the forms say "no activation"
WGRAD_UNSTATED = {"slope"}


def _fake(B, H, W, C):
    return types.SimpleNamespace(shape=(B, H, W, C), data_ptr=lambda: 0) if C else None


def _same(got, want, skip):
    return {n: (getattr(got, n), getattr(want, n)) for n, _ in _lib.ConvArgs._fields_ if n not in skip and getattr(got, n) != getattr(want, n)}


@pytest.mark.parametrize("row_id", [r["id"] for r in FR.ROWS])
def test_forward_rows_state_the_same_launch(row_id):
    row = next(r for r in FR.ROWS if r["id"] == row_id)
    want, Hi, Wi = FR.conv_args(row)[:3]
    B, H, W, C0, C1, N = (row[k] for k in ("B", "H", "W", "C0", "C1", "N"))
    x, x2 = _fake(B, Hi, Wi, C0), _fake(B, Hi, Wi, C1)
    epilogue = dict(slope=want.slope, operand_format=want.operand_format)   # operands, handed through: the geometry is what is compared
    if row["kind"] == "up":
        got = conv_launch.conv_transpose(x, x2, N, **epilogue)
    else:
        kh, kw, stride, pad = {"down": (4, 4, 2, 1), "c3": (3, 3, 1, 1)}.get(row["kind"], (H, W, 1, 0))   # lin / full: the window is the image
        got = conv_launch.conv(x, x2, N, kh, kw, stride, pad, **epilogue)
    assert not _same(got, want, POINTERS), row_id


@pytest.mark.parametrize("row_id", [r["id"] for r in WR.ROWS])
def test_wgrad_rows_state_the_same_launch(row_id):
    row = next(r for r in WR.ROWS if r["id"] == row_id)
    want = WR.conv_args(row)[0]
    B, H, W, C0, C1, N, k, s, p = (row[f] for f in ("B", "H", "W", "C0", "C1", "N", "k", "s", "p"))
    x, x2 = _fake(B, H, W, C0), _fake(B, H, W, C1)
    got = conv_launch.conv_transpose_phase(x, x2, N, 0, 0) if row["entry"] == "quad" else conv_launch.conv(x, x2, N, k, k, s, p)
    assert not _same(got, want, POINTERS | WGRAD_UNSTATED), row_id


def _model(a, src0, src1, wp):
    """The launch `a` describes, on NHWC arrays, by the numpy model of the engine."""
    assert (a.B, a.Hi, a.Wi, a.C0) == src0.shape and a.C1 == (src1.shape[3] if src1 is not None else 0) and not a.scale and not a.shift
    return KM.conv_igemm(src0, src1, wp, a.N, a.Hq, a.Wq, a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw, a.conv_transpose,
                         None, None, a.slope, None, None, a.Ho, a.Wo, a.os, a.ph, a.pw, a.out_mode)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pack_dgrad_weight(w, s, p):
    """include/m2h.h, m2h_pack_dgrad_weight: wp[ph*s+pw][ci][th][tw][co] = w[co][ci][(ph+p)%s + s*th][(pw+p)%s + s*tw]."""
    Co, Ci, KH, KW = w.shape
    wp = np.empty((s * s, Ci, KH // s, KW // s, Co), np.float32)
    for ph in range(s):
        for pw in range(s):
            for th in range(KH // s):
                for tw in range(KW // s):
                    wp[ph * s + pw, :, th, tw, :] = w[:, :, (ph + p) % s + s * th, (pw + p) % s + s * tw].T
    return wp.reshape(s * s, Ci, -1)


# (B, H, W, Ci, Co, k, s, p): odd sizes with unequal phase grids, input rows no window reaches, a 2x2 image under a 4x4 window, 1x1
DGRAD_SHAPES = [(2, 5, 7, 4, 8, 3, 1, 1), (2, 6, 10, 4, 8, 4, 2, 1), (1, 7, 9, 4, 8, 4, 2, 1), (2, 12, 16, 4, 8, 8, 4, 0), (1, 13, 18, 4, 8, 8, 4, 0),
                (2, 6, 8, 4, 8, 4, 2, 0), (3, 1, 1, 8, 4, 1, 1, 0), (1, 9, 11, 4, 8, 2, 1, 0), (1, 2, 2, 4, 4, 4, 2, 1)]


def _conv_input_grad(x_shape, w, dy, s, p):
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, w, stride=s, padding=p) * dy).sum().backward()
    return _nhwc(x.grad)


@pytest.mark.parametrize("B,H,W,Ci,Co,k,s,p", DGRAD_SHAPES)
def test_dgrad_phases_sum_to_the_input_gradient(B, H, W, Ci, Co, k, s, p):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + k)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    w = torch.randn(Co, Ci, k, k, generator=g)
    dy = torch.randn(B, Co, Ho, Wo, generator=g)
    ref = _conv_input_grad((B, Ci, H, W), w.double(), dy.double(), s, p)
    scale = _conv_input_grad((B, Ci, H, W), w.double() ** 2, dy.double() ** 2, s, p).sqrt()
    dy_nhwc, dx = _nhwc(dy), torch.zeros(B, H, W, Ci)
    wp = pack_dgrad_weight(w.numpy(), s, p)
    got = np.zeros((B, H, W, Ci), np.float32)
    for ph in range(s):
        for pw in range(s):
            a = conv_launch.conv_dgrad_phase(dy_nhwc, (H, W), Ci, k, k, s, p, ph, pw, dst=dx)
            assert (a is None) == (H <= ph or W <= pw)
            if a is not None:
                assert a.dst == dx.data_ptr() and a.src0 == dy_nhwc.data_ptr() and (a.Ho, a.Wo, a.ldc) == (H, W, Ci)
                got += _model(a, dy_nhwc.numpy(), None, wp[ph * s + pw])   # (each phase writes its own pixels of a zeroed image)
    worst, lsq, ok = bound(torch.from_numpy(got), ref, scale, TAU_FP32)
    print("dgrad %s: worst |g-r|/s %.2e  scale-1 %+.1e" % ((B, H, W, Ci, Co, k, s, p), worst, lsq - 1.0))
    assert ok, (worst, lsq)


def test_dgrad_phase_without_pixels_is_skipped():
    dy = _fake(1, 1, 2, 8)   # Conv2d(2, 2, 1) over a 1 x 3 image: no input row of phase ph = 1
    assert conv_launch.conv_dgrad_phase(dy, (1, 3), 4, 2, 2, 2, 1, 1, 0) is None
    a = conv_launch.conv_dgrad_phase(dy, (1, 3), 4, 2, 2, 2, 1, 0, 1)
    assert (a.Hq, a.Wq, a.offh, a.offw) == (1, 1, 0, 1)


def test_transposed_forms_match_conv_transpose2d():
    g = torch.Generator().manual_seed(7)
    B, H, W, C0, C1, N = 2, 3, 5, 8, 4, 8
    x, x2, w = torch.randn(B, C0, H, W, generator=g), torch.randn(B, C1, H, W, generator=g), torch.randn(C0 + C1, N, 4, 4, generator=g)
    xx = torch.cat([x, x2], 1).double()
    ref = _nhwc(F.conv_transpose2d(xx, w.double(), stride=2, padding=1))
    scale = _nhwc(F.conv_transpose2d(xx ** 2, w.double() ** 2, stride=2, padding=1)).sqrt()
    xn, x2n, wp = _nhwc(x), _nhwc(x2), KM.pack_convT_weight(w.numpy())
    whole = _model(conv_launch.conv_transpose(xn, x2n, N), xn.numpy(), x2n.numpy(), wp)
    phases = sum(_model(conv_launch.conv_transpose_phase(xn, x2n, N, ph, pw), xn.numpy(), x2n.numpy(), wp[2 * ph + pw]) for ph in (0, 1) for pw in (0, 1))
    for name, got in (("whole", whole), ("four phases", phases)):
        worst, lsq, ok = bound(torch.from_numpy(got), ref, scale, TAU_FP32)
        print("convT %s: worst |g-r|/s %.2e  scale-1 %+.1e" % (name, worst, lsq - 1.0))
        assert ok, (name, worst, lsq)


def test_workspace_rounds_up_to_whole_floats():
    cpu = torch.device("cpu")
    assert conv_launch.workspace(0, cpu) == (None, 0)
    for nbytes, floats in ((1, 1), (4, 1), (5, 2), (8, 2), (4099, 1025)):
        ws, n = conv_launch.workspace(nbytes, cpu)
        assert n == nbytes and ws.dtype == torch.float32 and ws.numel() == floats
