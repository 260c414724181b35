"""GPU: the shared-patch engine's all-padding skip (csrc/conv_patch.hip, tuning knob 40) -- on the whole-image 256 x 128 tile with
pixel grids 2 x 16, 4 x 16 and 2 x 32 a (tap, fragment) pair that reads only the zero rows above / below its image issues no MFMAs.
The skipped products have an all-zero operand, so the values must be those of the kernels that multiply the
zeros (knob 40 = -1) BIT FOR BIT, under both patch-form knobs (36 = 2 / 3), on the two-K-halves route, on persistent grids whose
workgroups change phase from tile to tile, and in the hi-only arithmetic; and they must match torch on the CPU at the tolerances of
tests/test_gpu_patch.py.  Grids the rule leaves alone (2 x 8: a fragment holds top and bottom rows; the 512 x 64 tile) run too."""
import pytest
import torch
import torch.nn.functional as F

import m2h_oracle as O
from test_gpu_patch import LABEL, LABEL64, _dev, _layer

pytestmark = pytest.mark.gpu

SKIP_KNOB = 40

# (B, H, W of the input, C0, C1, Co, transposed)
CASES = [
    (9, 4, 32, 64, 0, 128, False),       # 2 x 16 outputs, 8 images per tile, ragged second tile
    (9, 2, 16, 128, 128, 256, True),     # up1's grid, two sources
    (3, 8, 32, 64, 0, 128, False),       # 4 x 16 outputs
    (2, 2, 32, 64, 0, 128, True),        # 2 x 32 grid
    (5, 4, 16, 64, 0, 128, False),       # 2 x 8 outputs: W < 16, a fragment holds top and bottom rows, nothing may be skipped
    (1, 8, 64, 128, 128, 64, True),      # 512 x 64 tile: not enabled, equal trivially, label unchanged
]


def _make(B, H, W, C0, C1, Co, transposed, seed, hi_only=False):
    """Random layer: (torch-CPU result NCHW, arguments of _layer on the GPU).  hi_only: the CPU result from the operands rounded to bf16."""
    from m2h import ops
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C0, H, W, generator=g)
    x2 = torch.randn(B, C1, H, W, generator=g) if C1 else None
    Ci = C0 + C1
    if transposed:
        w = torch.randn(Ci, Co, 4, 4, generator=g) * (1.0 / (4 * Ci) ** 0.5)
    else:
        w = torch.randn(Co, Ci, 4, 4, generator=g) * (1.0 / (16 * Ci) ** 0.5)
    scale = torch.rand(Co, generator=g) + 0.5
    shift = torch.randn(Co, generator=g) * 0.1
    slope = 0.0 if transposed else 0.2
    xin = torch.cat((x, x2), 1) if C1 else x
    wr = w
    if hi_only:
        xin, wr = xin.bfloat16().float(), w.bfloat16().float()
    y = F.conv_transpose2d(xin, wr, None, stride=2, padding=1) if transposed else F.conv2d(xin, wr, None, stride=2, padding=1)
    want = F.leaky_relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), slope)
    nhwc = lambda t: ops.split32(t.permute(0, 2, 3, 1).contiguous().to(dev))  # noqa: E731
    wp = ops.split32(ops.pack_convT_weight(w.to(dev)) if transposed else ops.pack_conv_weight(w.to(dev)))
    return want, (nhwc(x), nhwc(x2) if C1 else None, wp, Co, transposed, scale.to(dev), shift.to(dev), slope)


def _run(args, knobs):
    """One layer under tuning knobs {number: value}; every knob back at 0 afterwards.  Returns (NCHW values on the CPU, label)."""
    from m2h import ops
    try:
        for k, v in knobs.items():
            ops.debug_set(k, v)
        got, label = _layer(*args)
    finally:
        for k in knobs:
            ops.debug_set(k, 0)
    return got.cpu().permute(0, 3, 1, 2), label


def _check_against_torch(got, want):
    e, m = O.rel_l1(got, want), float((got - want).abs().max() / want.abs().max())
    print("rel-L1 %.3e  max error %.3e of the largest output" % (e, m))
    assert got.shape == want.shape
    assert e < 1e-5 and m < 2e-4


@pytest.mark.parametrize("knob", [2, 3])   # 2: the engine's own choice of patch form; 3: the whole-image form wherever it fits
@pytest.mark.parametrize("B,H,W,C0,C1,Co,transposed", CASES)
def test_skipping_padding_fragments_keeps_every_bit(B, H, W, C0, C1, Co, transposed, knob):
    from m2h import ops
    want, args = _make(B, H, W, C0, C1, Co, transposed, B * 1000 + H * 10 + W + C0)
    ops.set_math_mode(ops.MATH_BF16X3)
    try:
        got, label = _run(args, {36: knob, SKIP_KNOB: 0})
        again, _ = _run(args, {36: knob, SKIP_KNOB: 0})
        off, off_label = _run(args, {36: knob, SKIP_KNOB: -1})
    finally:
        ops.set_math_mode(ops.MATH_FP32)
    assert label == off_label == (LABEL if Co % 128 == 0 else LABEL64)
    assert torch.equal(got, off)
    _check_against_torch(got, want)
    assert torch.equal(again, got)


def test_skipping_on_the_two_k_halves_route():
    """The fourth encoder stage's route (no knob 36: the engine's own dispatch splits the window's classes into two K-halves)."""
    from m2h import ops
    want, args = _make(128, 4, 32, 128, 0, 1024, False, 77)
    ops.set_math_mode(ops.MATH_BF16X3)
    try:
        got, label = _run(args, {SKIP_KNOB: 0})
        again, _ = _run(args, {SKIP_KNOB: 0})
        off, off_label = _run(args, {SKIP_KNOB: -1})
    finally:
        ops.set_math_mode(ops.MATH_FP32)
    assert label == off_label == "igemm_patch<256,128> + split-K reduce"
    assert torch.equal(got, off)
    _check_against_torch(got, want)
    assert torch.equal(again, got)


def test_skipping_on_persistent_grids_that_change_phase():
    """Tuning knob 10 = 8 / 24 workgroups: a workgroup's consecutive tiles are other phases of the transposed conv, so the dead
    mask is rebuilt at tile boundaries; the values must be those of one workgroup per tile."""
    from m2h import ops
    want, args = _make(64, 2, 16, 64, 64, 256, True, 4242)
    ops.set_math_mode(ops.MATH_BF16X3)
    try:
        one, label = _run(args, {36: 2, 10: 1 << 20, SKIP_KNOB: 0})   # (more workgroups than tiles: one workgroup per tile)
        assert label == LABEL
        for grid in (8, 24):
            got, _ = _run(args, {36: 2, 10: grid, SKIP_KNOB: 0})
            off, _ = _run(args, {36: 2, 10: grid, SKIP_KNOB: -1})
            assert torch.equal(got, one), grid
            assert torch.equal(got, off), grid
    finally:
        ops.set_math_mode(ops.MATH_FP32)
    _check_against_torch(one, want)


def test_skipping_in_hi_only_arithmetic():
    """M2H_MATH_BF16: the hi halves only, one MFMA per fragment pair (instantiations of their own); against the knob-off kernel bit
    for bit.  The hi half is the operand rounded to bf16 and a product of two bf16 values is exact in fp32, so against torch ON THE
    ROUNDED OPERANDS what remains is fp32 summation order and the split32 output, as in bf16x3 mode: the same tolerances."""
    from m2h import ops
    want, args = _make(9, 2, 16, 128, 128, 256, True, 99, hi_only=True)
    ops.set_math_mode(ops.MATH_BF16)
    try:
        got, label = _run(args, {36: 2, SKIP_KNOB: 0})
        again, _ = _run(args, {36: 2, SKIP_KNOB: 0})
        off, off_label = _run(args, {36: 2, SKIP_KNOB: -1})
    finally:
        ops.set_math_mode(ops.MATH_FP32)
    assert label == off_label == LABEL
    assert torch.equal(got, off) and torch.equal(again, got)
    _check_against_torch(got, want)
