"""GPU: conv1_strip_kernel<MASKED, HI> and convT_last_strip_kernel<N, HI> (csrc/conv_strip.hip) on every row of tests/strip_kernels.py's table
through ops.strip_conv1_fwd / ops.strip_last_fwd themselves, element by element against float64 (rows, cells, references, taus, mutants:
tests/strip_kernels.py, pinned on the CPU by tests/test_strip_kernels_cpu.py).  Per row: the output buffer is NaN before the call, so every
element must be written; the call is one launch with the expected label; |g - r| <= tau s + extra on every element, least-squares scale
included (elem_bound.bound); two runs give the same bits.  A multi-round row (more job slots than the grid has workgroups) runs in both
walking directions (knob 39), bit-identical to each other, and EVERY image of it is bit-identical to the same image run in a batch of at
most 8, whose job runs in a first round; its second-round images, their workgroups' other images and a seeded sample are held to float64.
The HI rows (ops.MATH_BF16) are held to TAU_FP32 from the bf16-rounded operands, with the flagged-rounding allowance and its two conditions.

Measured on an MI355X (test_zz_report prints them with -s).  `asserted` is the worst |g - r| / (s + extra / tau) in units of tau, the figure
each row holds under 1; `beyond` is the worst (|g - r| - extra)+ / s, what the additive terms (pre-op, output rounding, flagged roundings)
do not cover; `CPU` is the three-product (HI: fp32) stand-in's asserted figure on the small rows:
  kernel                  arithmetic   asserted     beyond      CPU      worst row
  strip_conv1             bf16x3       0.159 tau    3.19e-5     0.157    c1.cls.b129.t256 (small rows: 0.156, c1.cls.b9.t256)
  strip_conv1<masked>     bf16x3       0.150 tau    2.38e-5     0.134    c1.msk.b513.t64 / c1.msk.tiny_mask.b2.t128
  strip_convT_last<32>    bf16x3       0.091 tau    1.82e-5     0.085    last32.b65.h2.w128
  strip_convT_last<16>    bf16x3       0.093 tau    1.87e-5     0.085    last16.b260.h2.w64
  strip_conv1             bf16 (HI)    0.525 tau    4.17e-7     0.236    hi.c1.cls.b513.t64 (the output's own split32 rounding: at most 0.5)
  strip_conv1<masked>     bf16 (HI)    0.982 tau    3.38e-7     0.330    hi.c1.msk.b513.t64
  strip_convT_last<32>    bf16 (HI)    0.983 tau    1.61e-7     0.322    hi.last32.b257.h2.w32
  strip_convT_last<16>    bf16 (HI)    0.787 tau    1.21e-7     0.317    hi.last16.b513.h2.w32
An HI row's asserted figure sits just under 1 by construction: a flagged rounding that does land on the other neighbour uses the whole
ulp it is allowed; beyond the allowances the fp32 accumulation is at 0.6 % to 2 % of TAU_FP32.  Flagged: 0.19 % - 0.21 % of the pre-op's
results (37 % - 39 % of the outputs carry no allowance), 1.7 % - 1.9 % of Y (N = 32: 56 % - 58 %, N = 16: 74 % - 76 %).  Per family (bf16x3):
H in {1, 2, 3, 4, 16} and W in {32 .. 128} 0.086, wide BatchNorm scales 0.132 / 0.082, identity head 0.053, multi-round 0.159 / 0.093,
quiet 0.042, loud 0.006, zero mix / mask 0.027 / 0.028, negative mix 0.132, mask = 1 0.134, tiny mask 0.140.  Every bit-identity held:
two runs, both walking directions, every image of a multi-round row against its batch of 8.  No row found a kernel defect.  The 56 tests of
this file take 6.2 s on an MI355X (the slowest row, c1.msk.b129.t256, 1.0 s).
"""
import contextlib
from unittest import mock

import pytest
import torch

import strip_kernels as K
from m2h import _lib, ops

pytestmark = pytest.mark.gpu
WORST = {}
CHUNK = 8


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@contextlib.contextmanager
def _nan_outputs():
    """Inside the block every floating-point torch.empty is NaN: the ops allocate their outputs with it, so an element the kernel does
    not write stays NaN."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    with mock.patch.object(torch, "empty", empty):
        yield


def _prepare(row, d, dev):
    """The row's operands on the GPU, packed by the library's own packers: (per-image inputs, the rest)."""
    if row["kernel"].startswith("conv1"):
        w = d["w"].to(dev).contiguous()
        per_image = [d["mix"].to(dev), None if d["masks"] is None else d["masks"].to(dev), None if d["cls_val"] is None else d["cls_val"].to(dev)]
        return per_image, (ops.pack_strip_conv1(w), d["scale"].to(dev), d["shift"].to(dev), ops.unet_class_table(w, 32) if row["cls"] else None)
    nhwc = lambda t: ops.split32(t.to(dev).permute(0, 2, 3, 1).contiguous())   # noqa: E731
    rest = (ops.split32(ops.pack_convT_weight(d["w"].to(dev).contiguous())), d["scale"].to(dev), d["shift"].to(dev), d["hw"].to(dev).contiguous(), d["hb"].to(dev))
    return [nhwc(d["x"]), nhwc(d["skip"])], rest


def _launch(row, per_image, rest, lo=None, hi=None):
    """One launch on images [lo, hi) (all by default) into a NaN buffer; the label and the launch count are checked."""
    a = [None if t is None else t[lo:hi] for t in per_image]
    lib = _lib.load()
    n0 = lib.m2h_launch_count()
    with _nan_outputs():
        if row["kernel"].startswith("conv1"):
            wreg, scale, shift, table = rest
            out = ops.strip_conv1_fwd(a[0], a[1], wreg, scale, shift, table, a[2])
        else:
            wp, scale, shift, hw, hb = rest
            out = ops.strip_last_fwd(a[0], a[1], wp, scale, shift, hw, hb, row["N"])
    assert ops.last_kernel() == K.LABEL[row["kernel"]] and lib.m2h_launch_count() == n0 + 1
    return out


@pytest.mark.parametrize("name", list(K.ROWS))
def test_strip_row_matches_fp64(name):
    row, dev = K.ROWS[name], _dev()
    d = K.data(row)
    per_image, rest = _prepare(row, d, dev)
    mode = ops.math_mode()
    ops.set_math_mode(ops.MATH_BF16 if row["hi"] else ops.MATH_BF16X3)
    try:
        outs = []
        for rev in (K.directions(row) if not row["hi"] else (K.default_rev(row),)):
            ops.debug_set(K.REV_KNOB, K.knob(row, rev))
            out = _launch(row, per_image, rest)
            assert not bool(torch.isnan(out).any()), (name, rev, int(torch.isnan(out).sum()))       # every element written
            assert torch.equal(out, _launch(row, per_image, rest)), (name, rev)                       # two runs, the same bits
            outs.append(out)
        ops.debug_set(K.REV_KNOB, 0)
        out = outs[0]
        assert all(torch.equal(out, o) for o in outs[1:]), name                                        # both walking directions, the same bits
        if row["multi"]:       # every image against itself in a batch of at most 8: its job then runs in the first round
            for b0 in range(0, row["B"], CHUNK):
                b1 = min(b0 + CHUNK, row["B"])
                same = torch.equal(out[b0:b1], _launch(row, per_image, rest, b0, b1))
                assert same, (name, b0, b1)
    finally:
        ops.debug_set(K.REV_KNOB, 0)
        ops.set_math_mode(mode)
    idx = K.compared_images(row) if row["multi"] else list(range(row["B"]))
    ref = K.reference(row, K.take(d, idx))
    g = out[torch.as_tensor(idx, device=dev)].cpu()
    if row["kernel"].startswith("conv1"):
        g = K.unsplit32(g)
    assert g.shape == ref["r"].shape
    worst, scale, ok = K.check(g, ref)
    mode_name = "bf16 (HI)" if row["hi"] else "bf16x3"
    extra = ""
    if "flagged" in ref:
        extra = "  flagged %.4f  outputs without allowance %.3f" % (ref["flagged"], ref["clean"])
        assert ref["flagged"] <= K.FLAG_SHARE_MAX and ref["clean"] >= K.CLEAN_SHARE_MIN, (name, ref["flagged"], ref["clean"])
    beyond = K.excess(g, ref)
    print("%-30s %-22s %-9s worst %.3f tau, beyond the additive terms %.3f tau (tau %.0e)  scale-1 %+.1e  images compared %d of %d%s" % (
        name, K.LABEL[row["kernel"]], mode_name, worst, beyond, ref["tau"], scale - 1.0, len(idx), row["B"], extra))
    WORST[name] = (K.LABEL[row["kernel"]], mode_name, row["family"], worst, beyond, ref["tau"])
    assert ok, (name, worst, scale)


def test_zz_report():
    """(summary of the runs above: the worst ratio per kernel and arithmetic, and per row family)"""
    by_kernel, by_family = {}, {}
    for name, (label, mode, family, worst, beyond, tau) in WORST.items():
        for table, key in ((by_kernel, (label, mode)), (by_family, (label.split("<")[0], mode, family))):
            w0, b0 = table.get(key, ((0.0, ""), (0.0, "")))
            table[key] = (max(w0, (worst, name)), max(b0, (beyond * tau, name)))
    for table, what in ((by_kernel, "kernel"), (by_family, "family")):
        for key, ((worst, wname), (beyond, bname)) in sorted(table.items()):
            print("worst per %-7s %-52s %.3f tau (%s)   (|g - r| - extra) / s %.2e (%s)" % (what, " / ".join(key), worst, wname, beyond, bname))
