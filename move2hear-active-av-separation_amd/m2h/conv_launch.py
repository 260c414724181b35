"""The launch forms of the implicit-GEMM conv engine: each constructor below fills one ``m2h_conv_args`` (include/m2h.h) from tensors and
integers (only ``.shape`` and ``.data_ptr()`` are read: no GPU needed, tests/test_conv_launch_cpu.py; fields a form does not name stay
zero / null), and ``launch`` attaches the workspace and calls a C entry with it.  Every conv launch of the package states its geometry here."""
import ctypes

import torch

from . import _lib


def _args(x, x2, n_out, wp, dst, scale=None, shift=None, slope=1.0, operand_format=0):
    """Sources, weights, destination and epilogue (scale, shift, slope: 1 none, 0 ReLU; operand_format: FMT_* bits of m2h.ops)."""
    a = _lib.ConvArgs()
    a.B, a.Hi, a.Wi, a.C0 = x.shape
    a.src0, a.N, a.ldc, a.slope, a.operand_format = x.data_ptr(), n_out, n_out, slope, operand_format
    if x2 is not None:
        a.src1, a.C1 = x2.data_ptr(), x2.shape[3]
    if wp is not None:
        a.wp = wp.data_ptr()
    if dst is not None:
        a.dst = dst.data_ptr()
    if scale is not None:
        a.scale = scale.data_ptr()
    if shift is not None:
        a.shift = shift.data_ptr()
    return a


def conv(x, x2, n_out, kh, kw, stride=1, pad=0, wp=None, dst=None, scale=None, shift=None, slope=1.0, operand_format=0, ldc=None, out_mode=0):
    """Conv2d(kh x kw, stride, pad) over NHWC x [B,H,W,C0] (+ x2 [B,H,W,C1], concatenated on channels) -> n_out channels.  wp: packed
    [n_out, kh*kw*(C0+C1)] (the weight-gradient entries read the geometry only); dst rows are ldc floats apart (default n_out), out_mode
    ops.OUT_NHWC / OUT_DESLICE; the epilogue: as _args."""
    a = _args(x, x2, n_out, wp, dst, scale, shift, slope, operand_format)
    a.Ho = a.Hq = (a.Hi + 2 * pad - kh) // stride + 1
    a.Wo = a.Wq = (a.Wi + 2 * pad - kw) // stride + 1
    a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw, a.os, a.out_mode = stride, kh, kw, 1, -pad, 1, -pad, 1, out_mode
    if ldc is not None:
        a.ldc = ldc
    return a


def conv_transpose(x, x2, n_out, wp=None, dst=None, scale=None, shift=None, slope=1.0, operand_format=0):
    """The whole ConvTranspose2d(4, 2, 1) of cat(x, x2) -> NHWC [B,2H,2W,n_out] in one launch (conv_transpose = 1: the engine walks the
    four sub-pixel phases of 2x2 taps itself).  wp: ops.pack_convT_weight [4, n_out, 4*(C0+C1)]; the epilogue: as _args."""
    a = _args(x, x2, n_out, wp, dst, scale, shift, slope, operand_format)
    a.Hq, a.Wq, a.Ho, a.Wo = a.Hi, a.Wi, 2 * a.Hi, 2 * a.Wi
    a.stride, a.nth, a.ntw, a.conv_transpose, a.os = 1, 2, 2, 1, 2
    return a


def conv_transpose_phase(x, x2, n_out, ph, pw, wp=None, dst=None):
    """Sub-pixel phase (ph, pw) of it as an ordinary launch: taps step by 2*ph-1 / 2*pw-1, pixel (q, r) lands on output pixel (2q+ph, 2r+pw).
    wp: that phase's matrix of ops.pack_convT_weight.  (m2h_convT_wgrad_f32 takes phase (0, 0) and walks all four.)"""
    a = conv_transpose(x, x2, n_out, wp, dst)
    a.conv_transpose, a.mulh, a.mulw, a.ph, a.pw = 0, 2 * ph - 1, 2 * pw - 1, ph, pw
    return a


def conv_dgrad_phase(dy, in_hw, ci, kh, kw, stride, pad, ph, pw, wp=None, dst=None):
    """Phase (ph, pw) of the input gradient [B,H,W,ci] of a Conv2d(kh x kw, stride s, pad) from its NHWC output gradient dy (include/m2h.h,
    m2h_pack_dgrad_weight): input pixels (s*q+ph, s*r+pw) as a (kh/s x kw/s)-tap conv of dy whose taps step backwards.  wp: the phase's
    matrix wp[ph*s+pw] of m2h_pack_dgrad_weight; dst: the whole gradient.  None when the phase has no pixel: nothing to launch."""
    (H, W), s = in_hw, stride
    Hq, Wq = (H - ph + s - 1) // s, (W - pw + s - 1) // s
    if Hq <= 0 or Wq <= 0:
        return None
    a = _args(dy, None, ci, wp, dst)
    a.Hq, a.Wq, a.Ho, a.Wo = Hq, Wq, H, W
    a.stride, a.nth, a.ntw, a.mulh, a.mulw, a.os, a.ph, a.pw = 1, kh // s, kw // s, -1, -1, s, ph, pw
    a.offh, a.offw = (ph + pad) // s, (pw + pad) // s   # the header's (ph + p - (ph + p) % s) / s
    return a


def workspace(nbytes, dev):
    """(fp32 scratch of at least nbytes from the caching allocator, nbytes); (None, 0) when the launch needs none."""
    return (torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32), nbytes) if nbytes else (None, 0)


def launch(entry, a, size_fn, name, meta, dev, *extra):
    """Calls the C entry `entry`(&a, *extra, stream) on dev's current stream (the caller has made dev current and holds the tensors whose addresses
    it passes), with the workspace `size_fn`(&a) asks for attached to a and held until the call returns.  name, meta: as ops._timed (None: never timed)."""
    lib, ref = _lib.load(), ctypes.byref(a)
    ws, a.workspace_bytes = workspace(getattr(lib, size_fn)(ref), dev)
    if ws is not None:
        a.workspace = ws.data_ptr()
    fn, stream = getattr(lib, entry), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    return ops._timed(name, meta, dev, lambda: _lib.check(fn(ref, *extra, stream), entry))


from . import ops  # noqa: E402  (last: ops imports this module, whichever of the two is imported first)
