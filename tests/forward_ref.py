"""Float64 reference of a forward route row (tests/forward_routes.py) on normal data, and the bound's scale s beside it -- shared by
tests/test_gpu_forward_fp64.py (every row on the GPU) and tests/test_forward_routes_cpu.py (the bound discriminates; no GPU).

  z = conv2d(x, w, stride, pad)  or  conv_transpose2d(cat(x, x2), w, 2, 1)          in float64, from the same fp32 values
  r = act(z * scale + shift)                                                        the row's slope
  s = sqrt(conv(x^2, w^2)) * |scale| + |shift|                                      does not shrink when the terms cancel

The activations are 1-Lipschitz, so a bound on the pre-activation value carries over to r.  A `split` row's kernel never sees x and w
but hi + lo of ops.split32 (hi = bf16(x), lo = bf16(x - hi), round to nearest even): its reference is computed from those values.

The data are torch.randn: forward_routes.fill()'s integer formula is good for hashes, but its values are correlated (|r| / s reaches 41
at K = 2048 against ~5 for normal data; a plain fp32 CPU convolution then sits at 1.8e-5 * s, on the fp32 bound)."""
import zlib

import torch
import torch.nn.functional as F

import forward_routes as R


def geometry(row):
    """(Hi, Wi, Ho, Wo, K, slope, (kh, kw)) of the row: forward_routes.args_of without the struct."""
    a, Hi, Wi, Ho, Wo, K = R.args_of(row)
    kh, kw = (4, 4) if row["kind"] == "up" else (a.nth, a.ntw)
    return Hi, Wi, Ho, Wo, K, float(a.slope), (kh, kw)


def data(row, extra_in=0):
    """(x, x2, w, scale, shift) of the row in the torch layouts, fp32, from a generator seeded with crc32 of the row's id: x, x2 ~ N(0, 1),
    w ~ N(0, 1) * sqrt(2 / K); a `down` / `up` row (the kinds forward_routes.run() gives a folded BatchNorm) has scale = rand + 0.5 and
    shift = randn * 0.1.  extra_in: further input channels of the weight (the class plane of a first encoder stage)."""
    g = torch.Generator().manual_seed(zlib.crc32(row["id"].encode()))
    kind, B, C0, C1, N = (row[k] for k in ("kind", "B", "C0", "C1", "N"))
    Hi, Wi, _, _, K, _, (kh, kw) = geometry(row)
    x = torch.randn(B, C0, Hi, Wi, generator=g)
    x2 = torch.randn(B, C1, Hi, Wi, generator=g) if C1 else None
    shape = (C0 + C1, N, 4, 4) if kind == "up" else (N, C0 + C1 + extra_in, kh, kw)
    w = torch.randn(shape, generator=g) * (2.0 / K) ** 0.5
    scale = shift = None
    if kind in ("down", "up"):
        scale = torch.rand(N, generator=g) + 0.5
        shift = torch.randn(N, generator=g) * 0.1
    return x, x2, w, scale, shift


def hi_lo(t):
    """fp32 -> (hi, lo) of the split32 layout as fp32 tensors: hi = bf16(t), lo = bf16(t - hi), round to nearest even."""
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def seen(row, t):
    """The values the row's kernel reads, in float64: t itself, or hi + lo of a `split` row."""
    if not row["split"]:
        return t.double()
    hi, lo = hi_lo(t)
    return hi.double() + lo.double()


def conv(row, x, w):
    """The row's linear operation on NCHW x (both sources concatenated) and a torch-layout w, in their own dtype."""
    kind = row["kind"]
    if kind == "up":
        return F.conv_transpose2d(x, w, None, 2, 1)
    if kind == "down":
        return F.conv2d(x, w, None, 2, 1)
    if kind == "c3":
        return F.conv2d(x, w, None, 1, 1)
    return F.conv2d(x, w)   # lin / full: the window is the whole image; c1: a 1x1 conv


def act(v, slope):
    return torch.where(v > 0, v, v * slope)


def epilogue(row, z, scale, shift):
    """act(z * scale + shift) on an NCHW z, with the row's slope (scale / shift None: 1 / 0)."""
    if scale is not None:
        z = z * scale.to(z.dtype).view(1, -1, 1, 1) + shift.to(z.dtype).view(1, -1, 1, 1)
    return act(z, geometry(row)[5])


def sources(row, x, x2):
    return x if x2 is None else torch.cat((x, x2), 1)


def reference(row, x, x2, w, scale, shift):
    """(z, r, s) in float64, NCHW: the pre-epilogue sums, the reference output and the bound's scale (module docstring)."""
    xx, ww = seen(row, sources(row, x, x2)), seen(row, w)
    z = conv(row, xx, ww)
    q = conv(row, xx * xx, ww * ww).sqrt()
    if scale is None:
        return z, epilogue(row, z, None, None), q
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    return z, epilogue(row, z, scale.double(), shift.double()), q * sc.abs() + sh.abs()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()
